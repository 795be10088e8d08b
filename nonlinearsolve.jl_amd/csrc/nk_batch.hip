// Ensembles of small dense nonlinear systems, one system per GPU thread — the "kernel generation" use case of the
// reference (docs/src/tutorials/nonlinear_solve_gpus.md:70-176): `SimpleNewtonRaphson` (lib/SimpleNonlinearSolve/src/
// raphson.jl:39-83) called from inside a KernelAbstractions kernel over a vector of parameters. There the residual is
// Julia code that GPUCompiler specialises into the kernel; here it is HIP C++ source handed over as a string and
// compiled at run time with hiprtc together with the solver kernel for the given sizes (`-DNK_N`, `-DNK_NP`), so the
// residual, the forward-mode dual-number Jacobian (AutoForwardDiff is the reference's default, raphson.jl:28-33) and the
// pivoted LU are one straight-line register program per thread when N ≤ 8.
//
// Reference semantics kept (raphson.jl:50-82): `iszero(fx)` short cut; J evaluated at the current iterate; per iteration
// δx = J \ fx, x −= δx, THEN the termination check on the residual of the previous iterate (`check_termination` precedes
// `evaluate_f!!`), default mode AbsNormTerminationMode(maximum∘abs) (termination_conditions.jl:376-380), default abstol
// eps^(4/5) (common_defaults.jl:39-48), maxiters 1000; retcodes Success / MaxIters; a NaN residual never terminates.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)

static const char *k_kernel = R"NKSRC(
#if NK_N <= 8
#define NK_UNROLL _Pragma("unroll")
#else
#define NK_UNROLL _Pragma("nounroll")
#endif

__device__ inline void nk_jacobian(const nk_real *x, const nk_real *p, nk_real (*J)[NK_N]) {
#ifdef NK_HAS_JAC
  nk_jac(x, p, &J[0][0]);  // user-supplied analytic Jacobian, row-major N×N (SciMLBase.has_jac, utils.jl:98-99)
#else
  // AutoForwardDiff: NK_CH directions per sweep of the residual on dual numbers
  NK_UNROLL for (int c0 = 0; c0 < NK_N; c0 += NK_CH) {
    Dual xd[NK_N], fd[NK_N];
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      xd[i].v = x[i];
      NK_DUAL_LOOP xd[i].d[k] = (i == c0 + k) ? NK_R(1) : NK_R(0);
    }
    nk_f<Dual>(xd, p, fd);
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      NK_DUAL_LOOP if (c0 + k < NK_N) J[i][c0 + k] = fd[i].d[k];
    }
  }
#endif
}

// dx = A \ b by Gaussian elimination with partial pivoting (A and b are destroyed)
__device__ inline void nk_lu_solve(nk_real (*A)[NK_N], nk_real *b, nk_real *dx) {
  NK_UNROLL for (int c = 0; c < NK_N; ++c) {
    int piv = c;
    nk_real best = fabs(A[c][c]);
    NK_UNROLL for (int r = c + 1; r < NK_N; ++r) {
      const nk_real v = fabs(A[r][c]);
      if (v > best) { best = v; piv = r; }
    }
#if NK_N <= 8
    // row exchange by selects, so that every index stays a compile-time constant and the matrix lives in registers
    NK_UNROLL for (int r = c + 1; r < NK_N; ++r) {
      const bool s = (r == piv);
      NK_UNROLL for (int k = c; k < NK_N; ++k) {
        const nk_real t1 = A[c][k], t2 = A[r][k];
        A[c][k] = s ? t2 : t1;
        A[r][k] = s ? t1 : t2;
      }
      const nk_real b1 = b[c], b2 = b[r];
      b[c] = s ? b2 : b1;
      b[r] = s ? b1 : b2;
    }
#else
    if (piv != c) {
      for (int k = c; k < NK_N; ++k) { const nk_real t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
      const nk_real t = b[c]; b[c] = b[piv]; b[piv] = t;
    }
#endif
    const nk_real inv = NK_R(1) / A[c][c];
    NK_UNROLL for (int r = c + 1; r < NK_N; ++r) {
      const nk_real l = A[r][c] * inv;
      NK_UNROLL for (int k = c + 1; k < NK_N; ++k) A[r][k] -= l * A[c][k];
      b[r] -= l * b[c];
    }
  }
  NK_UNROLL for (int r = NK_N - 1; r >= 0; --r) {
    nk_real s = b[r];
    NK_UNROLL for (int k = r + 1; k < NK_N; ++k) s -= A[r][k] * dx[k];
    dx[r] = s / A[r][r];
  }
}

extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_newton(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                int maxiters, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], fx[NK_N], dx[NK_N], pp[NK_NP > 0 ? NK_NP : 1];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
  NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  bool allzero = true;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) allzero = allzero && (fx[i] == NK_R(0));
  int rc = 2 /* MaxIters */, it = 0;
  if (allzero) {
    rc = 1;  // Success (raphson.jl:55-56)
  } else {
    nk_real J[NK_N][NK_N], A[NK_N][NK_N], rhs[NK_N];
    nk_jacobian(x, pp, J);
    for (it = 1; it <= maxiters; ++it) {
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        rhs[i] = fx[i];
        NK_UNROLL for (int k = 0; k < NK_N; ++k) A[i][k] = J[i][k];
      }
      nk_lu_solve(A, rhs, dx);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] -= dx[i];
      // AbsNormTerminationMode(maximum∘abs) on the residual of the PREVIOUS iterate (the check precedes evaluate_f!!);
      // maximum propagates NaN, and NaN <= abstol is false
      nk_real nrm = NK_R(0);
      bool nan = false;
      NK_UNROLL for (int i = 0; i < NK_N; ++i) { const nk_real a = fabs(fx[i]); nan = nan || (a != a); nrm = a > nrm ? a : nrm; }
      if (!nan && nrm <= abstol) { rc = 1; break; }
      nk_f<nk_real>(x, pp, fx);
      nk_jacobian(x, pp, J);
    }
    if (it > maxiters) it = maxiters;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
  retcode[b] = rc;
  iters[b] = it;
}
// ---- SimpleTrustRegion (lib/SimpleNonlinearSolve/src/trust_region.jl:57-229, default update rule): dogleg step
// (Newton step if inside the region, else −g clipped to Δ, else the boundary point of the segment), ratio
// r = (f_{k+1} − f_k)/(δ·g + δ·Hδ/2) with H = JᵀJ, g = Jᵀf; shrink by t₁ when r < η₂ (ShrinkThresholdExceeded after
// max_shrink consecutive shrinks), accept when r ≥ η₁ (termination test on the NEW residual, then J, g at the new point,
// expand by t₂ up to Δmax when r > η₃). Δmax = max(‖f(u0)‖₂, max(u0) − min(u0)), Δ0 = Δmax/11.
__device__ inline nk_real nk_norm2(const nk_real *v) {
  nk_real s = NK_R(0);
  NK_UNROLL for (int i = 0; i < NK_N; ++i) s += v[i] * v[i];
  return sqrt(s);
}
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_trust_region(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                      int maxiters, nk_real eta1, nk_real eta2, nk_real eta3, nk_real t1, nk_real t2, int max_shrink,
                      nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode, int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], xo[NK_N], fx[NK_N], g[NK_N], dl[NK_N], dN[NK_N], dsd[NK_N], tmp[NK_N], pp[NK_NP > 0 ? NK_NP : 1];
  nk_real J[NK_N][NK_N], A[NK_N][NK_N];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { x[i] = u0[(u0_per_system ? b * NK_N : 0) + i]; xo[i] = x[i]; }
  NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  const nk_real norm_fx = nk_norm2(fx);
  nk_jacobian(x, pp, J);
  nk_real xmax = x[0], xmin = x[0];
  NK_UNROLL for (int i = 1; i < NK_N; ++i) { xmax = x[i] > xmax ? x[i] : xmax; xmin = x[i] < xmin ? x[i] : xmin; }
  const nk_real dmax = norm_fx > xmax - xmin ? norm_fx : xmax - xmin;
  nk_real delta = dmax / NK_R(11);
  nk_real fk = NK_R(0.5) * norm_fx * norm_fx;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { nk_real s = NK_R(0); NK_UNROLL for (int k = 0; k < NK_N; ++k) s += J[k][i] * fx[k]; g[i] = s; }
  int shrink = 0, rc = 2, it = 0;
  auto absmax_ok = [&](const nk_real *f) {
    nk_real nrm = NK_R(0); bool nan = false;
    NK_UNROLL for (int i = 0; i < NK_N; ++i) { const nk_real a = fabs(f[i]); nan = nan || (a != a); nrm = a > nrm ? a : nrm; }
    return !nan && nrm <= abstol;
  };
  if (absmax_ok(fx)) rc = 1;
  else {
    for (it = 1; it <= maxiters; ++it) {
      // dogleg
      NK_UNROLL for (int i = 0; i < NK_N; ++i) { tmp[i] = fx[i]; NK_UNROLL for (int k = 0; k < NK_N; ++k) A[i][k] = J[i][k]; }
      nk_lu_solve(A, tmp, dN);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) dN[i] = -dN[i];
      if (nk_norm2(dN) <= delta) {
        NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dN[i];
      } else {
        NK_UNROLL for (int i = 0; i < NK_N; ++i) dsd[i] = -g[i];
        const nk_real nsd = nk_norm2(dsd);
        if (nsd >= delta) {
          NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dsd[i] * (delta / nsd);
        } else {
          nk_real dNN = NK_R(0), dSN = NK_R(0), dSS = NK_R(0);
          NK_UNROLL for (int i = 0; i < NK_N; ++i) { const nk_real q = dN[i] - dsd[i]; dNN += q * q; dSN += dsd[i] * q; dSS += dsd[i] * dsd[i]; }
          const nk_real fact = dSN * dSN - dNN * (dSS - delta * delta);
          const nk_real tau = (-dSN + sqrt(fact)) / dNN;
          NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dsd[i] + tau * (dN[i] - dsd[i]);
        }
      }
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = xo[i] + dl[i];
      nk_f<nk_real>(x, pp, fx);
      const nk_real nf = nk_norm2(fx);
      const nk_real fk1 = nf * nf / NK_R(2);
      // Hδ = Jᵀ(Jδ)
      NK_UNROLL for (int i = 0; i < NK_N; ++i) { nk_real s = NK_R(0); NK_UNROLL for (int k = 0; k < NK_N; ++k) s += J[i][k] * dl[k]; tmp[i] = s; }
      nk_real dg = NK_R(0), dHd = NK_R(0);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        nk_real s = NK_R(0);
        NK_UNROLL for (int k = 0; k < NK_N; ++k) s += J[k][i] * tmp[k];
        dHd += dl[i] * s;
        dg += dl[i] * g[i];
      }
      const nk_real r = (fk1 - fk) / (dg + dHd / NK_R(2));
      if (r >= eta2) shrink = 0;
      else {
        delta = t1 * delta;
        if (++shrink > max_shrink) { rc = 6; break; }   // ShrinkThresholdExceeded
      }
      if (r >= eta1) {
        if (absmax_ok(fx)) { rc = 1; break; }
        NK_UNROLL for (int i = 0; i < NK_N; ++i) xo[i] = x[i];
        nk_jacobian(x, pp, J);
        if (r > eta3) delta = t2 * delta < dmax ? t2 * delta : dmax;
        fk = fk1;
        NK_UNROLL for (int i = 0; i < NK_N; ++i) { nk_real s = NK_R(0); NK_UNROLL for (int k = 0; k < NK_N; ++k) s += J[k][i] * fx[k]; g[i] = s; }
      }
    }
    if (it > maxiters) it = maxiters;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
  retcode[b] = rc;
  iters[b] = it;
}
)NKSRC";


// ----------------------------------------------------------------------------- one system per WAVEFRONT (8 < n ≤ 64)
// The per-thread kernel keeps the n×n Jacobian in registers only while n ≤ 8; beyond that it runs from scratch memory
// (measured ≈ 1 TFLOP/s against 16–27 TFLOP/s for n ≤ 8). Here a wavefront owns one system and lane j owns COLUMN j of the
// Jacobian: lane j evaluates the residual on dual numbers seeded with e_j (one partial), which gives it its column; the LU
// uses COLUMN pivoting — the pivot of row c is the largest entry of that row among the columns not used yet, found with a
// wave reduction, so no register ever moves; the multipliers l_r = a[r][p]/a[c][p] live in lane p and reach the others through
// v_readlane with a scalar lane index; every lane then updates its own column with register indices that are compile-time
// constants. The right-hand side, x and f(x) are replicated in all lanes. (nk_jac, if supplied, is not used by this kernel.)
// The lane helpers come first in the program text of both wavefront kernel sets (k_kernel_wave and k_kernel_wave_tr continue the
// text where this string ends, so that the Newton program reads exactly as it did as one string).
static const char *k_wave_helpers = R"NKSRC(
__device__ inline nk_real nk_rl(nk_real v, int lane) {
#ifdef NK_F32
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));   // one 32-bit readlane
#else
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
#endif
}
__device__ inline nk_real nk_wave_max(nk_real v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const nk_real w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}
)NKSRC";
static const char *k_kernel_wave = R"NKSRC(extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_newton_wave(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                     int maxiters, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                     int *__restrict__ iters) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * (NK_BLOCK_T / 64) + (threadIdx.x >> 6);
  if (b >= nbatch) return;   // whole wavefronts leave together
  nk_real x[NK_N], fx[NK_N], col[NK_N], pp[NK_NP > 0 ? NK_NP : 1];  // fx doubles as the right-hand side of the solve
#pragma unroll
  for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
#pragma unroll
  for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  bool allzero = true;
#pragma unroll
  for (int i = 0; i < NK_N; ++i) allzero = allzero && (fx[i] == NK_R(0));
  int rc = 2, it = 0;
  if (allzero) rc = 1;
  else {
    for (it = 1; it <= maxiters; ++it) {
      {  // column `lane` of J by one dual-number sweep (AutoForwardDiff with a single partial per lane)
        Dual xd[NK_N], fd[NK_N];
#pragma unroll
        for (int i = 0; i < NK_N; ++i) { xd[i].v = x[i]; xd[i].d[0] = (i == lane) ? NK_R(1) : NK_R(0); }
        nk_f<Dual>(xd, pp, fd);
#pragma unroll
        for (int i = 0; i < NK_N; ++i) col[i] = (lane < NK_N) ? fd[i].d[0] : NK_R(0);
      }
      // AbsNormTerminationMode(maximum∘abs) on the residual of the iterate the step starts from — the quantity the reference
      // tests AFTER the update (raphson.jl:72-75); taken here because the solve below overwrites fx
      nk_real nrm = NK_R(0);
      bool nan = false;
#pragma unroll
      for (int i = 0; i < NK_N; ++i) { const nk_real a = fabs(fx[i]); nan = nan || (a != a); nrm = a > nrm ? a : nrm; }
      const bool converged = !nan && nrm <= abstol;
      nk_real *rhs = fx;
      // ---- LU with column pivoting, applied to the right-hand side on the fly
      bool used = lane >= NK_N;   // lanes without a column never pivot
      int perm[NK_N];
#pragma unroll
      for (int c = 0; c < NK_N; ++c) {
        const nk_real mine = used ? -NK_R(1) : fabs(col[c]);
        const nk_real best = nk_wave_max(mine);
        const unsigned long long m = __ballot(!used && mine == best);
        const int pl = m ? (int)__ffsll((long long)m) - 1 : 0;   // (a NaN row: every compare fails — take lane 0, NaNs propagate)
        const int pv = __builtin_amdgcn_readfirstlane(pl);
        perm[c] = pv;
        const nk_real inv = NK_R(1) / nk_rl(col[c], pv);
        if (lane == pv) used = true;
        const nk_real cc = col[c];
#pragma unroll
        for (int r = c + 1; r < NK_N; ++r) {
          const nk_real l = nk_rl(col[r], pv) * inv;
          if (!used) col[r] -= l * cc;
          rhs[r] -= l * rhs[c];
        }
      }
      // ---- back substitution: the unknown of step c belongs to lane perm[c]
      nk_real mydx = NK_R(0);
#pragma unroll
      for (int c = NK_N - 1; c >= 0; --c) {
        const int pv = perm[c];
        const nk_real xc = rhs[c] / nk_rl(col[c], pv);
        if (lane == pv) mydx = xc;
#pragma unroll
        for (int r = 0; r < c; ++r) rhs[r] -= nk_rl(col[r], pv) * xc;
      }
#pragma unroll
      for (int i = 0; i < NK_N; ++i) x[i] -= nk_rl(mydx, i);
      if (converged) {  // the reference returns the residual of the iterate the last step started from: rebuild it (x + δ)
        rc = 1;
        nk_real xp[NK_N];
#pragma unroll
        for (int i = 0; i < NK_N; ++i) xp[i] = x[i] + nk_rl(mydx, i);
        nk_f<nk_real>(xp, pp, fx);
        break;
      }
      nk_f<nk_real>(x, pp, fx);
    }
    if (it > maxiters) it = maxiters;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
    retcode[b] = rc;
    iters[b] = it;
  }
}
)NKSRC";

// ---- SimpleTrustRegion, one system per wavefront (8 < n ≤ 64): the semantics of nk_batch_trust_region above, the layout of
// nk_batch_newton_wave. Lane j owns column j of J, so g_j = col·f needs no other lane, and g, δN, δsd, δ, xₒ and the trial point
// live one entry per lane; x, f(x) and p are replicated, as nk_f needs them. ‖·‖₂ and the dogleg's dot products are 64-lane
// xor butterflies (a + b and b + a are the same bits, so every lane ends with the same sum). There is no second copy of the
// column: g is formed before the LU factors the column in place, and the next step — after a rejected trial too — gets the
// column again by a dual sweep at xₒ. δᵀJᵀJδ = ‖Jδ‖², with Jδ from one more dual sweep seeded with δ itself (replicated in all
// lanes): no transposed product. Every scalar that steers a branch is the same in all lanes; each decision still goes through
// v_readfirstlane, so that the branches are scalar ones.
// Rounding-level differences from nk_batch_trust_region: column instead of row pivoting in the LU; ‖Jδ‖² instead of
// δ·(Jᵀ(Jδ)); butterfly sums instead of sequential ones for the per-lane vectors (‖f‖₂ and g are summed in its order).
static const char *k_kernel_wave_tr = R"NKSRC(
__device__ inline nk_real nk_wave_sum(nk_real v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// a decision that every lane takes alike, as a scalar
__device__ inline bool nk_uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }
// AbsNormTerminationMode(maximum∘abs): maximum propagates NaN, and NaN <= abstol is false
__device__ inline bool nk_absmax_ok(const nk_real *f, nk_real abstol) {
  nk_real nrm = NK_R(0);
  bool nan = false;
#pragma unroll
  for (int i = 0; i < NK_N; ++i) { const nk_real a = fabs(f[i]); nan = nan || (a != a); nrm = a > nrm ? a : nrm; }
  return !nan && nrm <= abstol;
}
__device__ inline nk_real nk_norm2(const nk_real *v) {
  nk_real s = NK_R(0);
#pragma unroll
  for (int i = 0; i < NK_N; ++i) s += v[i] * v[i];
  return sqrt(s);
}
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_trust_region_wave(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p,
                           nk_real abstol, int maxiters, nk_real eta1, nk_real eta2, nk_real eta3, nk_real t1, nk_real t2,
                           int max_shrink, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                           int *__restrict__ iters) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * (NK_BLOCK_T / 64) + (threadIdx.x >> 6);
  if (b >= nbatch) return;   // whole wavefronts leave together
  nk_real x[NK_N], fx[NK_N], col[NK_N], pp[NK_NP > 0 ? NK_NP : 1];  // fx doubles as the right-hand side of the solve
#pragma unroll
  for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
#pragma unroll
  for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  // per lane: entry `lane` of the accepted point xₒ, of the trial point and of g; lanes without a column hold zeros
  const bool own = lane < NK_N;
  nk_real xo = u0[(u0_per_system ? b * NK_N : 0) + (own ? lane : 0)];
  xo = own ? xo : NK_R(0);
  nk_real xt = xo, g = NK_R(0);
  nk_f<nk_real>(x, pp, fx);
  const nk_real norm_fx = nk_norm2(fx);
  nk_real xmax = x[0], xmin = x[0];
#pragma unroll
  for (int i = 1; i < NK_N; ++i) { xmax = x[i] > xmax ? x[i] : xmax; xmin = x[i] < xmin ? x[i] : xmin; }
  const nk_real dmax = norm_fx > xmax - xmin ? norm_fx : xmax - xmin;
  nk_real delta = dmax / NK_R(11);
  nk_real fk = NK_R(0.5) * norm_fx * norm_fx;
  int shrink = 0, rc = 2, it = 0;
  bool at_xo = true;   // fx is the residual at xₒ (the start, or an accepted trial): g is due
  if (nk_uniform(nk_absmax_ok(fx, abstol))) rc = 1;
  else {
    for (it = 1; it <= maxiters; ++it) {
#pragma unroll
      for (int i = 0; i < NK_N; ++i) x[i] = nk_rl(xo, i);   // xₒ, replicated (after a rejected trial x holds the trial point)
      {  // column `lane` of J(xₒ) by one dual-number sweep
        Dual xd[NK_N], fd[NK_N];
#pragma unroll
        for (int i = 0; i < NK_N; ++i) { xd[i].v = x[i]; xd[i].d[0] = (i == lane) ? NK_R(1) : NK_R(0); }
        nk_f<Dual>(xd, pp, fd);
#pragma unroll
        for (int i = 0; i < NK_N; ++i) col[i] = own ? fd[i].d[0] : NK_R(0);
      }
      if (at_xo) {   // g = Jᵀf at the accepted point; after a rejected trial g stays while fx is the trial's residual
        nk_real s = NK_R(0);
#pragma unroll
        for (int i = 0; i < NK_N; ++i) s += col[i] * fx[i];
        g = own ? s : NK_R(0);   // (0·NaN of an idle lane must not reach the sums)
      }
      // ---- δN = −J \ fx: LU with column pivoting, applied to the right-hand side on the fly (as nk_batch_newton_wave)
      nk_real *rhs = fx;
      bool used = !own;   // lanes without a column never pivot
      int perm[NK_N];
#pragma unroll
      for (int c = 0; c < NK_N; ++c) {
        const nk_real mine = used ? -NK_R(1) : fabs(col[c]);
        const nk_real best = nk_wave_max(mine);
        const unsigned long long m = __ballot(!used && mine == best);
        const int pl = m ? (int)__ffsll((long long)m) - 1 : 0;   // (a NaN row: every compare fails — take lane 0, NaNs propagate)
        const int pv = __builtin_amdgcn_readfirstlane(pl);
        perm[c] = pv;
        const nk_real inv = NK_R(1) / nk_rl(col[c], pv);
        if (lane == pv) used = true;
        const nk_real cc = col[c];
#pragma unroll
        for (int r = c + 1; r < NK_N; ++r) {
          const nk_real l = nk_rl(col[r], pv) * inv;
          if (!used) col[r] -= l * cc;
          rhs[r] -= l * rhs[c];
        }
      }
      nk_real dN = NK_R(0);
#pragma unroll
      for (int c = NK_N - 1; c >= 0; --c) {
        const int pv = perm[c];
        const nk_real xc = rhs[c] / nk_rl(col[c], pv);
        if (lane == pv) dN = -xc;
#pragma unroll
        for (int r = 0; r < c; ++r) rhs[r] -= nk_rl(col[r], pv) * xc;
      }
      // ---- dogleg: the Newton step inside the region, else −g clipped to Δ, else the boundary point of the segment
      nk_real dl;
      if (nk_uniform(sqrt(nk_wave_sum(dN * dN)) <= delta)) dl = dN;
      else {
        const nk_real dsd = -g;
        const nk_real nsd = sqrt(nk_wave_sum(dsd * dsd));
        if (nk_uniform(nsd >= delta)) dl = dsd * (delta / nsd);
        else {
          const nk_real q = dN - dsd;
          const nk_real dNN = nk_wave_sum(q * q), dSN = nk_wave_sum(dsd * q), dSS = nk_wave_sum(dsd * dsd);
          const nk_real fact = dSN * dSN - dNN * (dSS - delta * delta);
          const nk_real tau = (-dSN + sqrt(fact)) / dNN;
          dl = dsd + tau * q;
        }
        dl = own ? dl : NK_R(0);   // (a NaN or infinite factor must not reach the sums through the idle lanes)
      }
      // ---- δᵀJᵀJδ = ‖Jδ‖²: one dual sweep at xₒ seeded with δ
      nk_real dHd = NK_R(0);
      {
        Dual xd[NK_N], fd[NK_N];
#pragma unroll
        for (int i = 0; i < NK_N; ++i) { xd[i].v = x[i]; xd[i].d[0] = nk_rl(dl, i); }
        nk_f<Dual>(xd, pp, fd);
#pragma unroll
        for (int i = 0; i < NK_N; ++i) dHd += fd[i].d[0] * fd[i].d[0];
      }
      xt = xo + dl;
#pragma unroll
      for (int i = 0; i < NK_N; ++i) x[i] = nk_rl(xt, i);
      nk_f<nk_real>(x, pp, fx);
      const nk_real nf = nk_norm2(fx);
      const nk_real fk1 = nf * nf / NK_R(2);
      const nk_real r = (fk1 - fk) / (nk_wave_sum(dl * g) + dHd / NK_R(2));
      at_xo = false;
      if (nk_uniform(r >= eta2)) shrink = 0;
      else {
        delta = t1 * delta;
        if (++shrink > max_shrink) { rc = 6; break; }   // ShrinkThresholdExceeded
      }
      if (nk_uniform(r >= eta1)) {
        if (nk_uniform(nk_absmax_ok(fx, abstol))) { rc = 1; break; }
        xo = xt;
        if (nk_uniform(r > eta3)) delta = t2 * delta < dmax ? t2 * delta : dmax;
        fk = fk1;
        at_xo = true;
      }
    }
    if (it > maxiters) it = maxiters;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
    retcode[b] = rc;
    iters[b] = it;
  }
}
)NKSRC";

// ----------------------------------------------------------------------------- Jacobian-free methods, one system per thread
// SimpleBroyden (broyden.jl:31-108, linesearch = nothing), SimpleKlement (klement.jl:9-56) and SimpleDFSane (dfsane.jl:66-172,
// η_k = f₁/k²). A module of their own (nk_batch::mod_jf), compiled on first use, so that the Newton kernels' code objects and
// compile time stay as they were. All three test AbsNormTerminationMode(maximum∘abs) on the NEW residual right after it is
// evaluated (NaN never terminates) and return f at the returned u. No Jacobian, no LU: Klement and DFSane keep O(n) state,
// Broyden one n×n inverse. While n ≤ 8 every index is a compile-time constant and everything lives in registers (DFSane's
// history of up to 32 values too: select-writes, never a dynamic index); above that the arrays go to scratch.
static const char *k_kernel_jf = R"NKSRC(
#if NK_N <= 8
#define NK_UNROLL _Pragma("unroll")
#else
#define NK_UNROLL _Pragma("nounroll")
#endif
#define NK_HIST 32   // DFSane's M is at most this

__device__ inline nk_real nk_norm2(const nk_real *v) {
  nk_real s = NK_R(0);
  NK_UNROLL for (int i = 0; i < NK_N; ++i) s += v[i] * v[i];
  return sqrt(s);
}
// AbsNormTerminationMode(maximum∘abs): maximum propagates NaN, and NaN <= abstol is false
__device__ inline bool nk_absmax_ok(const nk_real *f, nk_real abstol) {
  nk_real nrm = NK_R(0);
  bool nan = false;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { const nk_real a = fabs(f[i]); nan = nan || (a != a); nrm = a > nrm ? a : nrm; }
  return !nan && nrm <= abstol;
}
// Julia's max / clamp / sign on floats: NaN propagates (fmax / fmin would drop it)
__device__ inline nk_real nk_jl_max(nk_real a, nk_real b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }
__device__ inline nk_real nk_jl_clamp(nk_real x, nk_real lo, nk_real hi) { return x > hi ? hi : (x < lo ? lo : x); }
__device__ inline nk_real nk_jl_sign(nk_real x) { return x > NK_R(0) ? NK_R(1) : (x < NK_R(0) ? NK_R(-1) : x); }

// ---- SimpleBroyden: J⁻¹ = init_α·I; δx = −J⁻¹ fprev, x += δx, f, check; J⁻¹ += ((δx − J⁻¹δf)/(δx·J⁻¹δf)) (J⁻¹ᵀδx)ᵀ.
// alpha_inv > 0 is 1/alpha (computed on the host in double, as Julia's inv(alpha) is); else init_α comes from the norms.
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_broyden(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                 int maxiters, nk_real alpha_inv, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out,
                 int *__restrict__ retcode, int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], fx[NK_N], fprev[NK_N], dx[NK_N], t[NK_N], xJ[NK_N], pp[NK_NP > 0 ? NK_NP : 1];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
  NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  bool allzero = true;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) allzero = allzero && (fx[i] == NK_R(0));
  int rc = 2, it = 0;
  if (allzero) {
    rc = 1;  // iszero(fx) (broyden.jl:44-45)
  } else {
    nk_real init_a = alpha_inv;
    if (!(alpha_inv > NK_R(0))) {
      // Julia compares fx_norm ≥ 1.0e-5 in Float64; for a Float32 norm that is fx_norm ≥ the smallest float ≥ 1e-5
#ifdef NK_F32
      const nk_real thresh = 0x1.4f8b5ap-17f;
#else
      const nk_real thresh = 1.0e-5;
#endif
      const nk_real fn = nk_norm2(fx), xn = nk_norm2(x);
      init_a = fn >= thresh ? nk_jl_max(xn, NK_R(1)) / (NK_R(2) * fn) : NK_R(1);
    }
    nk_real Ji[NK_N][NK_N];
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      fprev[i] = fx[i];
      NK_UNROLL for (int k = 0; k < NK_N; ++k) Ji[i][k] = (i == k) ? init_a : NK_R(0);
    }
    for (it = 1; it <= maxiters; ++it) {
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        nk_real s = NK_R(0);
        NK_UNROLL for (int k = 0; k < NK_N; ++k) s += Ji[i][k] * fprev[k];
        dx[i] = -s;
      }
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] += dx[i];   // x = xo + δx (xo is always the previous x)
      nk_f<nk_real>(x, pp, fx);
      if (nk_absmax_ok(fx, abstol)) { rc = 1; break; }
      NK_UNROLL for (int i = 0; i < NK_N; ++i) xJ[i] = fx[i] - fprev[i];   // δf (xJ is free until below)
      nk_real d = NK_R(0);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        nk_real s = NK_R(0);
        NK_UNROLL for (int k = 0; k < NK_N; ++k) s += Ji[i][k] * xJ[k];
        t[i] = s;                                                  // J⁻¹δf
        d += dx[i] * s;
      }
      NK_UNROLL for (int j = 0; j < NK_N; ++j) {
        nk_real s = NK_R(0);
        NK_UNROLL for (int i = 0; i < NK_N; ++i) s += Ji[i][j] * dx[i];
        xJ[j] = s;                                                 // J⁻¹ᵀδx
      }
      // no guard on d = 0: inf / NaN propagate as in Julia
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        const nk_real w = (dx[i] - t[i]) / d;
        NK_UNROLL for (int j = 0; j < NK_N; ++j) Ji[i][j] += w * xJ[j];
        fprev[i] = fx[i];
      }
    }
    if (it > maxiters) it = maxiters;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
  retcode[b] = rc;
  iters[b] = it;
}

// ---- SimpleKlement: diagonal J, starting at ones and reset to ones when any entry is 0; δx = fprev ./ J, x −= δx, f, check;
// J += (f − fprev − J·δ)/(δ²J², or 1e-5 where that is 0)·δ·J² with δ = −δx.
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_klement(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                 int maxiters, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                 int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], fx[NK_N], fprev[NK_N], J[NK_N], dx[NK_N], pp[NK_NP > 0 ? NK_NP : 1];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
  NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { fprev[i] = fx[i]; J[i] = NK_R(1); }
  int rc = 2, it;
  for (it = 1; it <= maxiters; ++it) {
    bool anyzero = false;
    NK_UNROLL for (int i = 0; i < NK_N; ++i) anyzero = anyzero || (J[i] == NK_R(0));
    if (anyzero) {
      NK_UNROLL for (int i = 0; i < NK_N; ++i) J[i] = NK_R(1);
    }
    NK_UNROLL for (int i = 0; i < NK_N; ++i) { dx[i] = fprev[i] / J[i]; x[i] -= dx[i]; }
    nk_f<nk_real>(x, pp, fx);
    if (nk_absmax_ok(fx, abstol)) { rc = 1; break; }
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      const nk_real d = -dx[i], j2 = J[i] * J[i];
      const nk_real d2 = (d * d) * j2;
      const nk_real den = d2 == NK_R(0) ? NK_R(1.0e-5) : d2;
      J[i] = J[i] + (((fx[i] - fprev[i]) - J[i] * d) / den) * d * j2;
      fprev[i] = fx[i];
    }
  }
  if (it > maxiters) it = maxiters;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
  retcode[b] = rc;
  iters[b] = it;
}

// ---- SimpleDFSane: spectral residual steps d = −σF with the Grippo–Lampariello–Lucidi non-monotone line search over the
// last M merit values f = ‖F‖₂^n_exp. The counter k is the reference's: it counts outer iterations AND inner line-search
// passes, both loops run while k < maxiters, and the history slot written is mod1(k, M) with k after the inner increments.
__device__ inline nk_real nk_merit(const nk_real *f, int nexp) {
  const nk_real s = nk_norm2(f);
  return nexp == 1 ? s : s * s;
}
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_dfsane(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                int maxiters, nk_real sigma_min, nk_real sigma_max, nk_real sigma_1, int M, nk_real gamma, nk_real tau_min,
                nk_real tau_max, int nexp, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  // fp: F at x (the reference's δf between iterations; d = −σ·fp); xc: the trial point (x_cache)
  nk_real x[NK_N], fx[NK_N], fp[NK_N], xc[NK_N], hist[NK_HIST], pp[NK_NP > 0 ? NK_NP : 1];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
  NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
  nk_f<nk_real>(x, pp, fx);
  nk_real fn = nk_merit(fx, nexp);
  const nk_real f1 = fn;
#pragma unroll
  for (int j = 0; j < NK_HIST; ++j) hist[j] = fn;
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { fp[i] = fx[i]; xc[i] = x[i]; }
  nk_real sk = sigma_1;
  int rc = 2, k = 0;
  while (k < maxiters) {
    sk = nk_jl_sign(sk) * nk_jl_clamp(fabs(sk), sigma_min, sigma_max);
    const nk_real ms = -sk;
    const long k1 = (long)k + 1;
    const nk_real eta = f1 / (nk_real)(k1 * k1);
    nk_real fbar = hist[0];
#pragma unroll
    for (int j = 1; j < NK_HIST; ++j) fbar = j < M ? nk_jl_max(fbar, hist[j]) : fbar;
    const nk_real fbe = fbar + eta;
    nk_real ap = NK_R(1), am = NK_R(1);
    NK_UNROLL for (int i = 0; i < NK_N; ++i) xc[i] = x[i] + ap * (ms * fp[i]);
    nk_f<nk_real>(xc, pp, fx);
    nk_real fnew = nk_merit(fx, nexp);
    while (k < maxiters) {
      if (fnew <= fbe - gamma * (ap * ap) * fn) break;
      const nk_real atp = (ap * ap) * fn / (fnew + (NK_R(2) * ap - NK_R(1)) * fn);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) xc[i] = x[i] - am * (ms * fp[i]);
      nk_f<nk_real>(xc, pp, fx);
      fnew = nk_merit(fx, nexp);
      if (fnew <= fbe - gamma * (am * am) * fn) break;
      const nk_real atm = (am * am) * fn / (fnew + (NK_R(2) * am - NK_R(1)) * fn);
      ap = nk_jl_clamp(atp, tau_min * ap, tau_max * ap);
      am = nk_jl_clamp(atm, tau_min * am, tau_max * am);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) xc[i] = x[i] + ap * (ms * fp[i]);
      nk_f<nk_real>(xc, pp, fx);
      fnew = nk_merit(fx, nexp);
      ++k;
    }
    if (nk_absmax_ok(fx, abstol)) {
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = xc[i];
      rc = 1;
      ++k;   // counts the iteration that passed the check
      break;
    }
    // σ = δx·δx / δx·δf with δx = x_new − x, δf = F(x_new) − F(x)
    nk_real sxx = NK_R(0), sxf = NK_R(0);
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      const nk_real dxi = xc[i] - x[i], dfi = fx[i] - fp[i];
      sxx += dxi * dxi;
      sxf += dxi * dfi;
      x[i] = xc[i];
      fp[i] = fx[i];
    }
    sk = sxx / sxf;
    fn = fnew;
    const int slot = (k + M - 1) % M;   // mod1(k, M), 0-based
#pragma unroll
    for (int j = 0; j < NK_HIST; ++j) hist[j] = j == slot ? fnew : hist[j];
    ++k;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { u_out[b * NK_N + i] = x[i]; r_out[b * NK_N + i] = fx[i]; }
  retcode[b] = rc;
  iters[b] = k < maxiters ? k : maxiters;
}
)NKSRC";

// ----------------------------------------------------------------------------- nonlinear least squares, one problem per thread
// m residuals, n unknowns, m ≥ n (-DNK_M, -DNK_N): SimpleGaussNewton = SimpleNewtonRaphson on a NonlinearLeastSquaresProblem
// (raphson.jl:31, 41-82) and SimpleTrustRegion on one (trust_region.jl:60-229, default update rule). A kernel set and an object
// kind of their own (nk_batch_create_nlls); the square kernels above are not touched. What differs from them:
//  * J is m×n. One dual-number sweep with NK_CH = n partials returns all of it while n ≤ 8 (chunks of 8 above).
//  * `J \ f` is the least-squares solution by Householder QR with column pivoting — what `\` does for a non-square dense
//    matrix in the reference's language — in place on J: the reflector vectors stay below the diagonal, Q is never formed.
//    No normal equations in the Newton step. Divergence from the reference, which leaves rank deficiency to LAPACK's rank
//    truncation: here a column whose pivot has |r_kk| ≤ m·eps·|r_11| gets a zero step component (the basic solution).
//    The column norms are recomputed at every step (no downdating) and taken without scaling: entries beyond
//    sqrt(floatmax) overflow them.
//  * termination is AbsNormTerminationMode(Base.Fix2(norm, 2)), the :simple default for a NonlinearLeastSquaresProblem
//    (termination_conditions.jl:381-383): ‖f‖₂ ≤ abstol; NaN ≤ abstol is false. A fit whose minimum residual is not zero
//    therefore never reports Success.
//  * the trust region keeps H = JᵀJ (n×n) and g = Jᵀf, formed before the factorisation overwrites J, and takes Hδ from H
//    as trust_region.jl:151 does. As there, a rejected trial point leaves its residual in fx, and the next dogleg solves
//    with the unchanged factorisation against that residual.
// While n ≤ 8 and m·(n + 2) ≤ NK_NLLS_REG_LIMIT every index is a compile-time constant (column exchange by selects) and J lives in
// registers; above that the arrays go to scratch. p is copied into a private array while nparams ≤ 32 and read in place
// beyond (a fit's data travels in p: 2m values for (x_i, y_i) pairs). One problem per thread only: a per-wavefront form would
// need a per-residual user function, a second source contract.
static const char *k_kernel_nlls = R"NKSRC(
// register-resident shapes: n ≤ 8 and m·(n + 2) ≤ 80 (Float64) or 128 (Float32) — J, the duals of the sweep and the
// residual copies make about m·(2n + 3) live values. Found with the compiler's resource notes (no private segment for either
// kernel at the largest m of every n); not timed.
#ifndef NK_NLLS_REG_LIMIT
#ifdef NK_F32
#define NK_NLLS_REG_LIMIT 128
#else
#define NK_NLLS_REG_LIMIT 80
#endif
#endif
#if NK_N <= 8 && NK_M * (NK_N + 2) <= NK_NLLS_REG_LIMIT
#define NK_REGS 1
#define NK_UNROLL _Pragma("unroll")
#else
#define NK_UNROLL _Pragma("nounroll")
#endif
#ifdef NK_F32
#define NK_EPS 1.1920929e-7f
#else
#define NK_EPS 2.220446049250313e-16
#endif
#if NK_NP <= 32
#define NK_P_DECL nk_real pp[NK_NP > 0 ? NK_NP : 1]; NK_UNROLL for (int i = 0; i < NK_NP; ++i) pp[i] = p[b * NK_NP + i];
#else
#define NK_P_DECL const nk_real *pp = p + b * NK_NP;   // read in place: a private copy of this size would spill
#endif

__device__ inline nk_real nk_norm2_n(const nk_real *v) {
  nk_real s = NK_R(0);
  NK_UNROLL for (int i = 0; i < NK_N; ++i) s += v[i] * v[i];
  return sqrt(s);
}
__device__ inline nk_real nk_norm2_m(const nk_real *v) {
  nk_real s = NK_R(0);
  NK_UNROLL for (int i = 0; i < NK_M; ++i) s += v[i] * v[i];
  return sqrt(s);
}
// the residual; entries the source does not write (one written for n outputs, built with m > n) are zero
__device__ inline void nk_resid(const nk_real *x, const nk_real *p, nk_real *f) {
  NK_UNROLL for (int i = 0; i < NK_M; ++i) f[i] = NK_R(0);
  nk_f<nk_real>(x, p, f);
}
__device__ inline void nk_jacobian(const nk_real *x, const nk_real *p, nk_real (*J)[NK_N]) {
#ifdef NK_HAS_JAC
  nk_jac(x, p, &J[0][0]);  // user-supplied analytic Jacobian, row-major M×N (SciMLBase.has_jac, utils.jl:98-99)
#else
  // AutoForwardDiff: NK_CH directions per sweep of the residual on dual numbers (all of J in one sweep while N ≤ 8)
  NK_UNROLL for (int c0 = 0; c0 < NK_N; c0 += NK_CH) {
    Dual xd[NK_N], fd[NK_M];
    NK_UNROLL for (int i = 0; i < NK_N; ++i) {
      xd[i].v = x[i];
      NK_DUAL_LOOP xd[i].d[k] = (i == c0 + k) ? NK_R(1) : NK_R(0);
    }
    NK_UNROLL for (int i = 0; i < NK_M; ++i) fd[i] = Dual(NK_R(0));
    nk_f<Dual>(xd, p, fd);
    NK_UNROLL for (int i = 0; i < NK_M; ++i) {
      NK_DUAL_LOOP if (c0 + k < NK_N) J[i][c0 + k] = fd[i].d[k];
    }
  }
#endif
}

// Householder QR with column pivoting, in place. On return the upper triangle of J holds R, the part below the diagonal
// the reflector vectors (v_kk = 1 implied), H_k = I − tau_k v vᵀ, and piv[k] the column exchanged with column k at step k.
__device__ inline void nk_qr_factor(nk_real (*J)[NK_N], nk_real *tau, int *piv) {
  NK_UNROLL for (int k = 0; k < NK_N; ++k) {
    // the remaining column of largest 2-norm over rows k..M-1; the first one on ties, and a NaN norm never displaces column k
    int pv = k;
    nk_real best = NK_R(0);
    NK_UNROLL for (int j = k; j < NK_N; ++j) {
      nk_real s = NK_R(0);
      NK_UNROLL for (int i = k; i < NK_M; ++i) s += J[i][j] * J[i][j];
      if (j == k) best = s;
      else if (s > best) { best = s; pv = j; }
    }
    piv[k] = pv;
#ifdef NK_REGS
    // column exchange by selects, so that every index stays a compile-time constant and the matrix lives in registers
    NK_UNROLL for (int j = k + 1; j < NK_N; ++j) {
      const bool s = (j == pv);
      NK_UNROLL for (int i = 0; i < NK_M; ++i) {
        const nk_real t1 = J[i][k], t2 = J[i][j];
        J[i][k] = s ? t2 : t1;
        J[i][j] = s ? t1 : t2;
      }
    }
#else
    if (pv != k) {
      for (int i = 0; i < NK_M; ++i) { const nk_real t = J[i][k]; J[i][k] = J[i][pv]; J[i][pv] = t; }
    }
#endif
    // reflector: beta = −sign(alpha)·‖x‖, tau = (beta − alpha)/beta, v = x/(alpha − beta) below the diagonal; a zero column
    // gives tau = 0 (H = I)
    const nk_real alpha = J[k][k];
    const nk_real nrm = sqrt(best);
    const bool z = (nrm == NK_R(0));
    const nk_real beta = alpha >= NK_R(0) ? -nrm : nrm;
    const nk_real t = z ? NK_R(0) : (beta - alpha) / beta;
    const nk_real sc = z ? NK_R(0) : NK_R(1) / (alpha - beta);
    tau[k] = t;
    J[k][k] = beta;
    NK_UNROLL for (int i = k + 1; i < NK_M; ++i) J[i][k] *= sc;
    NK_UNROLL for (int j = k + 1; j < NK_N; ++j) {
      nk_real w = J[k][j];
      NK_UNROLL for (int i = k + 1; i < NK_M; ++i) w += J[i][k] * J[i][j];
      w *= t;
      J[k][j] -= w;
      NK_UNROLL for (int i = k + 1; i < NK_M; ++i) J[i][j] -= J[i][k] * w;
    }
  }
}
// dx = argmin ‖J dx − c‖₂ from the factorisation: c ← Qᵀc (destroyed), back substitution with R, columns below the rank
// threshold get 0, then the column exchanges are undone in reverse order
__device__ inline void nk_qr_solve(const nk_real (*J)[NK_N], const nk_real *tau, const int *piv, nk_real *c, nk_real *dx) {
  NK_UNROLL for (int k = 0; k < NK_N; ++k) {
    nk_real w = c[k];
    NK_UNROLL for (int i = k + 1; i < NK_M; ++i) w += J[i][k] * c[i];
    w *= tau[k];
    c[k] -= w;
    NK_UNROLL for (int i = k + 1; i < NK_M; ++i) c[i] -= J[i][k] * w;
  }
  const nk_real thr = (NK_R(NK_M) * NK_R(NK_EPS)) * fabs(J[0][0]);   // max(m, n)·eps·|r_11|
  NK_UNROLL for (int k = NK_N - 1; k >= 0; --k) {
    nk_real s = c[k];
    NK_UNROLL for (int j = k + 1; j < NK_N; ++j) s -= J[k][j] * dx[j];
    dx[k] = fabs(J[k][k]) <= thr ? NK_R(0) : s / J[k][k];
  }
  NK_UNROLL for (int k = NK_N - 1; k >= 0; --k) {
#ifdef NK_REGS
    NK_UNROLL for (int j = k + 1; j < NK_N; ++j) {
      const bool s = (j == piv[k]);
      const nk_real t1 = dx[k], t2 = dx[j];
      dx[k] = s ? t2 : t1;
      dx[j] = s ? t1 : t2;
    }
#else
    const int pv = piv[k];
    if (pv != k) { const nk_real t = dx[k]; dx[k] = dx[pv]; dx[pv] = t; }
#endif
  }
}

// ---- SimpleGaussNewton (raphson.jl:52-81 on a NonlinearLeastSquaresProblem)
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_gauss_newton(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p, nk_real abstol,
                      int maxiters, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                      int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], fx[NK_M], dx[NK_N], c[NK_M], tau[NK_N];
  int piv[NK_N];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = u0[(u0_per_system ? b * NK_N : 0) + i];
  NK_P_DECL
  nk_resid(x, pp, fx);
  bool allzero = true;
  NK_UNROLL for (int i = 0; i < NK_M; ++i) allzero = allzero && (fx[i] == NK_R(0));
  int rc = 2 /* MaxIters */, it = 0;
  if (allzero) {
    rc = 1;  // Success (raphson.jl:55-56)
  } else {
    nk_real J[NK_M][NK_N];
    nk_jacobian(x, pp, J);
    for (it = 1; it <= maxiters; ++it) {
      NK_UNROLL for (int i = 0; i < NK_M; ++i) c[i] = fx[i];
      nk_qr_factor(J, tau, piv);       // δx = J \ fx (raphson.jl:71)
      nk_qr_solve(J, tau, piv, c, dx);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] -= dx[i];
      // ‖fx‖₂ ≤ abstol on the residual of the PREVIOUS iterate (check_termination precedes evaluate_f!!, raphson.jl:74-77)
      if (nk_norm2_m(fx) <= abstol) { rc = 1; break; }
      nk_resid(x, pp, fx);
      nk_jacobian(x, pp, J);
    }
    if (it > maxiters) it = maxiters;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) u_out[b * NK_N + i] = x[i];
  NK_UNROLL for (int i = 0; i < NK_M; ++i) r_out[b * NK_M + i] = fx[i];
  retcode[b] = rc;
  iters[b] = it;
}

// ---- SimpleTrustRegion (trust_region.jl:60-229, default update rule) on m residuals
// H = JᵀJ and g = Jᵀf from the unfactored J (trust_region.jl:126-127, 185-186), then J is factored for the dogleg's Newton step
__device__ inline void nk_normal_forms(const nk_real (*J)[NK_N], const nk_real *fx, nk_real (*H)[NK_N], nk_real *g) {
  NK_UNROLL for (int i = 0; i < NK_N; ++i) {
    NK_UNROLL for (int j = 0; j < NK_N; ++j) {
      nk_real s = NK_R(0);
      NK_UNROLL for (int k = 0; k < NK_M; ++k) s += J[k][i] * J[k][j];
      H[i][j] = s;
    }
    nk_real s = NK_R(0);
    NK_UNROLL for (int k = 0; k < NK_M; ++k) s += J[k][i] * fx[k];
    g[i] = s;
  }
}
extern "C" __global__ void __launch_bounds__(NK_BLOCK_T)
nk_batch_trust_region_nlls(long nbatch, const nk_real *__restrict__ u0, int u0_per_system, const nk_real *__restrict__ p,
                           nk_real abstol, int maxiters, nk_real eta1, nk_real eta2, nk_real eta3, nk_real t1, nk_real t2,
                           int max_shrink, nk_real *__restrict__ u_out, nk_real *__restrict__ r_out, int *__restrict__ retcode,
                           int *__restrict__ iters) {
  const long b = (long)blockIdx.x * NK_BLOCK_T + threadIdx.x;
  if (b >= nbatch) return;
  nk_real x[NK_N], xo[NK_N], fx[NK_M], c[NK_M], g[NK_N], dl[NK_N], dN[NK_N], dsd[NK_N], tau[NK_N];
  nk_real J[NK_M][NK_N], H[NK_N][NK_N];
  int piv[NK_N];
  NK_UNROLL for (int i = 0; i < NK_N; ++i) { x[i] = u0[(u0_per_system ? b * NK_N : 0) + i]; xo[i] = x[i]; }
  NK_P_DECL
  nk_resid(x, pp, fx);
  const nk_real norm_fx = nk_norm2_m(fx);
  nk_jacobian(x, pp, J);
  nk_real xmax = x[0], xmin = x[0];
  NK_UNROLL for (int i = 1; i < NK_N; ++i) { xmax = x[i] > xmax ? x[i] : xmax; xmin = x[i] < xmin ? x[i] : xmin; }
  const nk_real dmax = norm_fx > xmax - xmin ? norm_fx : xmax - xmin;   // trust_region.jl:115
  nk_real delta = dmax / NK_R(11);
  nk_real fk = NK_R(0.5) * norm_fx * norm_fx;
  nk_normal_forms(J, fx, H, g);
  nk_qr_factor(J, tau, piv);
  int shrink = 0, rc = 2, it = 0;
  if (norm_fx <= abstol) rc = 1;   // the check before the loop (trust_region.jl:136-139); no iszero shortcut
  else {
    for (it = 1; it <= maxiters; ++it) {
      // dogleg (trust_region.jl:201-229): δN = −(J \ fx)
      NK_UNROLL for (int i = 0; i < NK_M; ++i) c[i] = fx[i];
      nk_qr_solve(J, tau, piv, c, dN);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) dN[i] = -dN[i];
      if (nk_norm2_n(dN) <= delta) {
        NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dN[i];
      } else {
        NK_UNROLL for (int i = 0; i < NK_N; ++i) dsd[i] = -g[i];
        const nk_real nsd = nk_norm2_n(dsd);
        if (nsd >= delta) {
          NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dsd[i] * (delta / nsd);
        } else {
          nk_real dNN = NK_R(0), dSN = NK_R(0), dSS = NK_R(0);
          NK_UNROLL for (int i = 0; i < NK_N; ++i) { const nk_real q = dN[i] - dsd[i]; dNN += q * q; dSN += dsd[i] * q; dSS += dsd[i] * dsd[i]; }
          const nk_real fact = dSN * dSN - dNN * (dSS - delta * delta);
          const nk_real tu = (-dSN + sqrt(fact)) / dNN;
          NK_UNROLL for (int i = 0; i < NK_N; ++i) dl[i] = dsd[i] + tu * (dN[i] - dsd[i]);
        }
      }
      NK_UNROLL for (int i = 0; i < NK_N; ++i) x[i] = xo[i] + dl[i];
      nk_resid(x, pp, fx);
      const nk_real nf = nk_norm2_m(fx);
      const nk_real fk1 = nf * nf / NK_R(2);
      // r = (f_{k+1} − f_k)/(δ·g + δ·Hδ/2) (trust_region.jl:151-152)
      nk_real dg = NK_R(0), dHd = NK_R(0);
      NK_UNROLL for (int i = 0; i < NK_N; ++i) {
        nk_real s = NK_R(0);
        NK_UNROLL for (int k = 0; k < NK_N; ++k) s += H[i][k] * dl[k];
        dHd += dl[i] * s;
        dg += dl[i] * g[i];
      }
      const nk_real r = (fk1 - fk) / (dg + dHd / NK_R(2));
      if (r >= eta2) shrink = 0;
      else {
        delta = t1 * delta;
        if (++shrink > max_shrink) { rc = 6; break; }   // ShrinkThresholdExceeded
      }
      if (r >= eta1) {
        if (nf <= abstol) { rc = 1; break; }
        NK_UNROLL for (int i = 0; i < NK_N; ++i) xo[i] = x[i];
        nk_jacobian(x, pp, J);
        if (r > eta3) delta = t2 * delta < dmax ? t2 * delta : dmax;
        fk = fk1;
        nk_normal_forms(J, fx, H, g);
        nk_qr_factor(J, tau, piv);
      }
    }
    if (it > maxiters) it = maxiters;
  }
  NK_UNROLL for (int i = 0; i < NK_N; ++i) u_out[b * NK_N + i] = x[i];
  NK_UNROLL for (int i = 0; i < NK_M; ++i) r_out[b * NK_M + i] = fx[i];
  retcode[b] = rc;
  iters[b] = it;
}
)NKSRC";


struct nk_batch {
  nk_ctx *ctx = nullptr;
  int n = 0, np = 0, block = 64;
  int m = 0;  // residuals of a least-squares object (nk_batch_create_nlls: mod holds the NLLS kernel set); 0 = a square object
  hipFunction_t fn_gn = nullptr, fn_tr_nlls = nullptr;
  hipModule_t mod = nullptr, mod_wave = nullptr;
  hipFunction_t fn = nullptr, fn_tr = nullptr, fn_wave = nullptr;  // fn_wave: one system per wavefront (8 < n ≤ 64)
  // the per-wavefront trust-region kernel: a module of its own, compiled on the first trust-region solve that can use it
  hipModule_t mod_tr_wave = nullptr;
  hipFunction_t fn_tr_wave = nullptr;
  bool tr_wave_tried = false;      // one attempt per object: a failed build leaves the per-thread kernel in charge
  const char *last_kernel = "";    // the kernel the last solve launched (nk_batch_last_kernel)
  // the Jacobian-free kernels: a module of their own, compiled on the first call that needs it (from source / flags)
  hipModule_t mod_jf = nullptr;
  hipFunction_t fn_broyden = nullptr, fn_klement = nullptr, fn_dfsane = nullptr;
  std::string source;
  int flags = 0;
  bool f32 = false;  // kernels built with -DNK_F32 (flags & NK_BATCH_FLOAT32): float arrays and scalar arguments
  // staging for host-memspace calls (sized in doubles; a Float32 object uses the first half of each)
  double *d_u0 = nullptr, *d_p = nullptr, *d_u = nullptr, *d_r = nullptr;
  int *d_rc = nullptr, *d_it = nullptr;
  int64_t cap = 0;
};

// the kernel sets, one hiprtc program each
enum { KSET_NEWTON = 0 /* nk_batch_newton + nk_batch_trust_region */, KSET_WAVE = 1 /* nk_batch_newton_wave */,
       KSET_JF = 2 /* nk_batch_broyden + nk_batch_klement + nk_batch_dfsane */,
       KSET_NLLS = 3 /* nk_batch_gauss_newton + nk_batch_trust_region_nlls (m residuals, -DNK_M) */,
       KSET_WAVE_TR = 4 /* nk_batch_trust_region_wave */ };

// SimpleTrustRegion runs one system per wavefront from this n on (up to 64), one per thread below: the smallest measured n
// from which nk_batch_trust_region_wave solved at least as many systems per second as nk_batch_trust_region at every larger
// measured n, in Float64 and in Float32 ("Ensemble SimpleTrustRegion per wavefront")
#define NK_BATCH_TR_WAVE_MIN_N 9

// compile `source` (+ prelude + solver kernels) for n unknowns / np parameters (and, for KSET_NLLS, m residuals); code
// object into `code`, log into `log`
static int batch_compile(const char *source, int n, int np, int flags, std::vector<char> *code, std::string *log,
                         int kset = KSET_NEWTON, int m = 0) {
  const bool wave = kset == KSET_WAVE || kset == KSET_WAVE_TR, nlls = kset == KSET_NLLS;
  NK_REQUIRE(source, "NULL source");
  NK_REQUIRE(n >= 1 && n <= 64, "n = %d outside 1..64 (one system per thread)", n);
  NK_REQUIRE(!nlls || (m >= n && m <= 64),
             "m = %d residuals for n = %d unknowns: a least-squares ensemble needs n <= m <= 64 (the contract is `template "
             "<typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f)` with u: n values, f: m values; the "
             "minimum-norm solution of an underdetermined problem is not offered)", m, n);
  NK_REQUIRE(np >= 0 && np <= 256, "nparams = %d outside 0..256", np);
  std::string full = std::string(nk_dual_prelude) + "\n// ---- user source\n" + source + "\n" +
                     (wave ? k_wave_helpers : "") +
                     (kset == KSET_WAVE ? k_kernel_wave : kset == KSET_WAVE_TR ? k_kernel_wave_tr : kset == KSET_JF ? k_kernel_jf
                      : nlls ? k_kernel_nlls : k_kernel);
  // dual-number partials per residual sweep (wave kernels: one per lane; the Jacobian-free kernels sweep no duals)
  const int ch = wave || kset == KSET_JF ? 1 : (n < 8 ? n : 8);
  const std::string dn = "-DNK_N=" + std::to_string(n), dp = "-DNK_NP=" + std::to_string(np), dc = "-DNK_CH=" + std::to_string(ch),
                    db = wave ? "-DNK_BLOCK_T=256" : "-DNK_BLOCK_T=64";
  std::vector<const char *> opts = nk_rtc_base_options();
  opts.insert(opts.end(), {dn.c_str(), dp.c_str(), dc.c_str(), db.c_str()});
  const std::string dm = "-DNK_M=" + std::to_string(m);
  if (nlls) opts.push_back(dm.c_str());
  if ((flags & NK_BATCH_ANALYTIC_JAC) && (kset == KSET_NEWTON || nlls)) opts.push_back("-DNK_HAS_JAC=1");
  if (flags & NK_BATCH_FLOAT32) opts.push_back("-DNK_F32=1");
  bool failed = false;
  NK_TRY(nk_rtc_compile(full, "nk_batch_user.hip", opts, code, log, &failed));
  if (failed) {
    const char *lg = log && !log->empty() ? log->c_str() : "(no log)";
    if (flags & NK_BATCH_FLOAT32)   // the usual cause: a source written against the Float64 contract (const double *p)
      NK_FAIL(NK_E_INVALID, "residual source does not compile in Float32 mode, whose contract is `template <typename T> "
              "__device__ void nk_f(const T *u, const nk_real *p, T *f)` (and `__device__ void nk_jac(const nk_real *u, "
              "const nk_real *p, nk_real *J)`) with nk_real = float: %.900s", lg);
    NK_FAIL(NK_E_INVALID, "residual source does not compile: %.900s", lg);
  }
  return NK_OK;
}

// compile only (no device needed): the "does the user's residual build for gfx950" check. (The per-wavefront trust-region
// kernel instantiates nk_f exactly as the per-wavefront Newton kernel does, so it is not compiled here as well.)
extern "C" int nk_batch_compile_check(const char *source, int n, int nparams, int flags, int64_t *code_bytes) {
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log));
  if (code_bytes) *code_bytes = (int64_t)code.size();
  if (n > 8 && !(flags & NK_BATCH_PER_THREAD)) {  // medium systems also get the per-wavefront Newton kernel
    std::vector<char> wcode;
    std::string wlog;
    NK_TRY(batch_compile(source, n, nparams, flags, &wcode, &wlog, KSET_WAVE));
    if (code_bytes) *code_bytes += (int64_t)wcode.size();
  }
  return NK_OK;
}

// the code object hiprtc makes for one kernel set (wave = 0: nk_batch_newton + nk_batch_trust_region; 1: nk_batch_newton_wave;
// 2: nk_batch_trust_region_wave), for inspection (disassembly, resource notes). *bytes gets its size; buf may be NULL to ask
// for the size only.
extern "C" int nk_batch_code_object(const char *source, int n, int nparams, int flags, int wave, void *buf, int64_t capacity,
                                    int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_REQUIRE(wave <= 2, "wave = %d: 0 (per thread), 1 (nk_batch_newton_wave) or 2 (nk_batch_trust_region_wave)", wave);
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log, wave == 2 ? KSET_WAVE_TR : wave != 0 ? KSET_WAVE : KSET_NEWTON));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}

// the same for the Jacobian-free kernel set (nk_batch_broyden, nk_batch_klement, nk_batch_dfsane)
extern "C" int nk_batch_jf_code_object(const char *source, int n, int nparams, int flags, void *buf, int64_t capacity,
                                       int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log, KSET_JF));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}

// ---- least squares: compile check, code object and object creation for the NLLS kernel set
extern "C" int nk_batch_nlls_compile_check(const char *source, int n, int m, int nparams, int flags, int64_t *code_bytes) {
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log, KSET_NLLS, m));
  if (code_bytes) *code_bytes = (int64_t)code.size();
  return NK_OK;
}

extern "C" int nk_batch_nlls_code_object(const char *source, int n, int m, int nparams, int flags, void *buf, int64_t capacity,
                                         int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log, KSET_NLLS, m));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}

extern "C" int nk_batch_create_nlls(nk_ctx *ctx, const char *source, int n, int m, int nparams, int flags, nk_batch **out) {
  NK_REQUIRE(ctx && out, "NULL argument");
  NK_HIP(hipSetDevice(ctx->device));
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log, KSET_NLLS, m));
  nk_batch *B = new nk_batch();
  B->ctx = ctx;
  B->n = n;
  B->m = m;
  B->np = nparams;
  B->f32 = (flags & NK_BATCH_FLOAT32) != 0;
  B->source = source;
  B->flags = flags;
  if (hipModuleLoadData(&B->mod, code.data()) != hipSuccess) { delete B; NK_FAIL(NK_E_HIP, "hipModuleLoadData failed"); }
  if (hipModuleGetFunction(&B->fn_gn, B->mod, "nk_batch_gauss_newton") != hipSuccess ||
      hipModuleGetFunction(&B->fn_tr_nlls, B->mod, "nk_batch_trust_region_nlls") != hipSuccess) {
    hipModuleUnload(B->mod);
    delete B;
    NK_FAIL(NK_E_HIP, "a least-squares kernel is missing from the compiled module");
  }
  *out = B;
  return NK_OK;
}

extern "C" int nk_batch_create(nk_ctx *ctx, const char *source, int n, int nparams, int flags, nk_batch **out) {
  NK_REQUIRE(ctx && out, "NULL argument");
  NK_HIP(hipSetDevice(ctx->device));
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(source, n, nparams, flags, &code, &log));
  nk_batch *B = new nk_batch();
  B->ctx = ctx;
  B->n = n;
  B->np = nparams;
  B->f32 = (flags & NK_BATCH_FLOAT32) != 0;
  B->source = source;
  B->flags = flags;
  if (hipModuleLoadData(&B->mod, code.data()) != hipSuccess) { delete B; NK_FAIL(NK_E_HIP, "hipModuleLoadData failed"); }
  if (hipModuleGetFunction(&B->fn, B->mod, "nk_batch_newton") != hipSuccess) {
    hipModuleUnload(B->mod);
    delete B;
    NK_FAIL(NK_E_HIP, "kernel nk_batch_newton not found in the compiled module");
  }
  if (hipModuleGetFunction(&B->fn_tr, B->mod, "nk_batch_trust_region") != hipSuccess) B->fn_tr = nullptr;
  if (n > 8 && !(flags & NK_BATCH_PER_THREAD)) {  // Newton for medium systems: the per-wavefront kernel
    std::vector<char> wcode;
    std::string wlog;
    if (batch_compile(source, n, nparams, flags, &wcode, &wlog, KSET_WAVE) == NK_OK &&
        hipModuleLoadData(&B->mod_wave, wcode.data()) == hipSuccess) {
      if (hipModuleGetFunction(&B->fn_wave, B->mod_wave, "nk_batch_newton_wave") != hipSuccess) B->fn_wave = nullptr;
    }
  }
  *out = B;
  return NK_OK;
}

extern "C" int nk_batch_destroy(nk_batch *B) {
  if (!B) return NK_OK;
  hipFree(B->d_u0); hipFree(B->d_p); hipFree(B->d_u); hipFree(B->d_r); hipFree(B->d_rc); hipFree(B->d_it);
  if (B->mod) hipModuleUnload(B->mod);
  if (B->mod_wave) hipModuleUnload(B->mod_wave);
  if (B->mod_jf) hipModuleUnload(B->mod_jf);
  if (B->mod_tr_wave) hipModuleUnload(B->mod_tr_wave);
  delete B;
  return NK_OK;
}

// Solve all systems. u0: n values shared by every system (u0_per_system = 0, the tutorial's case) or nbatch×n;
// p: nbatch×nparams. Outputs (nbatch×n, nbatch×n, nbatch, nbatch); retcode/iters may be NULL. The arrays hold doubles, or
// floats for an object built with NK_BATCH_FLOAT32 (f32 says which entry point the caller used); the scalars arrive as double
// and reach the kernels in the object's precision, T(abstol) as the reference takes them.
// prm holds the method's parameters, defaults applied (reals and integers alike as double):
//   BATCH_TRUST_REGION {η₁, η₂, η₃, t₁, t₂, max_shrink_times}; BATCH_BROYDEN {1/alpha, or 0 for `nothing`};
//   BATCH_DFSANE {σ_min, σ_max, σ₁, M, γ, τ_min, τ_max, n_exp}; nothing for BATCH_NEWTON and BATCH_KLEMENT.
//   BATCH_TR_NLLS as BATCH_TRUST_REGION; nothing for BATCH_GAUSS_NEWTON. The last two run on a least-squares object
//   (nk_batch_create_nlls) only, the others on a square one only; resid_out is nbatch×m there.
enum { BATCH_NEWTON, BATCH_TRUST_REGION, BATCH_BROYDEN, BATCH_KLEMENT, BATCH_DFSANE, BATCH_GAUSS_NEWTON, BATCH_TR_NLLS };

// the Jacobian-free module, compiled and loaded on the first call that needs it, then kept on the object
static int batch_load_jf(nk_batch *B) {
  if (B->mod_jf) return NK_OK;
  std::vector<char> code;
  std::string log;
  NK_TRY(batch_compile(B->source.c_str(), B->n, B->np, B->flags, &code, &log, KSET_JF));
  hipModule_t m = nullptr;
  if (hipModuleLoadData(&m, code.data()) != hipSuccess) NK_FAIL(NK_E_HIP, "hipModuleLoadData failed (Jacobian-free kernels)");
  hipFunction_t fb = nullptr, fk = nullptr, fd = nullptr;
  if (hipModuleGetFunction(&fb, m, "nk_batch_broyden") != hipSuccess || hipModuleGetFunction(&fk, m, "nk_batch_klement") != hipSuccess ||
      hipModuleGetFunction(&fd, m, "nk_batch_dfsane") != hipSuccess) {
    hipModuleUnload(m);
    NK_FAIL(NK_E_HIP, "a Jacobian-free kernel is missing from the compiled module");
  }
  B->mod_jf = m;
  B->fn_broyden = fb;
  B->fn_klement = fk;
  B->fn_dfsane = fd;
  return NK_OK;
}

// the per-wavefront trust-region module, compiled and loaded on the first trust-region solve of an object that can use it
// (NK_BATCH_TR_WAVE_MIN_N ≤ n ≤ 64, no NK_BATCH_PER_THREAD). As with the Newton wave kernel, a failure is not an error: fn_tr_wave
// stays NULL and the per-thread kernel runs; nk_batch_last_kernel says which one did.
static void batch_load_tr_wave(nk_batch *B) {
  if (B->tr_wave_tried) return;
  B->tr_wave_tried = true;
  std::vector<char> code;
  std::string log;
  hipModule_t m = nullptr;
  if (batch_compile(B->source.c_str(), B->n, B->np, B->flags, &code, &log, KSET_WAVE_TR) != NK_OK ||
      hipModuleLoadData(&m, code.data()) != hipSuccess)
    return;
  if (hipModuleGetFunction(&B->fn_tr_wave, m, "nk_batch_trust_region_wave") != hipSuccess) {
    B->fn_tr_wave = nullptr;
    hipModuleUnload(m);
    return;
  }
  B->mod_tr_wave = m;
}

static int batch_run(nk_batch *B, bool f32, int method, int64_t nbatch, const void *u0, int u0_per_system, const void *p,
                     int memspace, double abstol, int maxiters, const double *prm, void *u_out, void *resid_out,
                     int32_t *retcode_out, int32_t *iters_out) {
  NK_REQUIRE(B && u0 && u_out && resid_out, "NULL argument");
  NK_REQUIRE(B->f32 == f32, B->f32 ? "this ensemble was compiled for Float32 (NK_BATCH_FLOAT32): call the _f32 entry points"
                                   : "this ensemble was compiled for Float64: the _f32 entry points need NK_BATCH_FLOAT32");
  NK_REQUIRE((method >= BATCH_GAUSS_NEWTON) == (B->m > 0),
             B->m > 0 ? "this is a least-squares ensemble (nk_batch_create_nlls): call nk_batch_solve_gauss_newton or "
                        "nk_batch_solve_trust_region_nlls"
                      : "this is a square ensemble (nk_batch_create): the least-squares entry points need nk_batch_create_nlls");
  NK_REQUIRE(nbatch >= 0, "negative batch size");
  NK_REQUIRE(B->np == 0 || p, "parameters are required (nparams = %d)", B->np);
  NK_REQUIRE(method != BATCH_TRUST_REGION || B->fn_tr, "the compiled module lacks the trust-region kernel");
  nk_ctx *ctx = B->ctx;
  NK_HIP(hipSetDevice(ctx->device));
  if (nbatch == 0) return NK_OK;
  if (method >= BATCH_BROYDEN && method <= BATCH_DFSANE) NK_TRY(batch_load_jf(B));
  if (method == BATCH_TRUST_REGION && !(B->flags & NK_BATCH_PER_THREAD) && B->n >= NK_BATCH_TR_WAVE_MIN_N && B->n <= 64)
    batch_load_tr_wave(B);
  if (maxiters <= 0) maxiters = 1000;                             // raphson.jl:42 / trust_region.jl:60 / broyden.jl:33 / ...
  const int n = B->n, np = B->np;
  const int nr = B->m > 0 ? B->m : n;   // residuals per system
  const size_t es = f32 ? sizeof(float) : sizeof(double);
  if (B->cap < nbatch) {
    hipFree(B->d_u0); hipFree(B->d_p); hipFree(B->d_u); hipFree(B->d_r); hipFree(B->d_rc); hipFree(B->d_it);
    B->d_u0 = B->d_p = B->d_u = B->d_r = nullptr;
    B->d_rc = B->d_it = nullptr;
    NK_TRY(nk_dev_alloc(&B->d_u0, (size_t)nbatch * n));
    NK_TRY(nk_dev_alloc(&B->d_p, (size_t)nbatch * (np > 0 ? np : 1)));
    NK_TRY(nk_dev_alloc(&B->d_u, (size_t)nbatch * n));
    NK_TRY(nk_dev_alloc(&B->d_r, (size_t)nbatch * nr));
    NK_TRY(nk_dev_alloc(&B->d_rc, (size_t)nbatch));
    NK_TRY(nk_dev_alloc(&B->d_it, (size_t)nbatch));
    B->cap = nbatch;
  }
  const void *du0 = u0, *dp = p;
  void *du = u_out, *dr = resid_out;
  const size_t nu0 = (size_t)(u0_per_system ? nbatch : 1) * n;
  if (memspace != NK_DEVICE) {
    NK_HIP(hipMemcpyAsync(B->d_u0, u0, nu0 * es, hipMemcpyHostToDevice, ctx->stream));
    if (np > 0) NK_HIP(hipMemcpyAsync(B->d_p, p, (size_t)nbatch * np * es, hipMemcpyHostToDevice, ctx->stream));
    du0 = B->d_u0;
    dp = B->d_p;
    du = B->d_u;
    dr = B->d_r;
  }
  long nb = (long)nbatch;
  int ups = u0_per_system ? 1 : 0;
  int *drc = B->d_rc, *dit = B->d_it;
  // the kernels' real scalars: abstol, then the method's parameters; the defaults are the element type's
  // (common_defaults.jl:39-53: eps(T)^(4/5), taken in T)
  const int nprm = method == BATCH_TRUST_REGION || method == BATCH_TR_NLLS ? 6 : method == BATCH_BROYDEN ? 1 : method == BATCH_DFSANE ? 8 : 0;
  double sd[9];
  float sf[9];
  sd[0] = abstol > 0.0 ? abstol : pow(2.220446049250313e-16, 0.8);
  sf[0] = abstol > 0.0 ? (float)abstol : powf(1.1920929e-7f, 0.8f);
  for (int k = 0; k < 8; ++k) { sd[k + 1] = k < nprm ? prm[k] : 0.0; sf[k + 1] = (float)sd[k + 1]; }
  void *sa[9];
  for (int k = 0; k < 9; ++k) sa[k] = f32 ? (void *)&sf[k] : (void *)&sd[k];
  const unsigned grid = (unsigned)((nbatch + B->block - 1) / B->block);
  hipError_t st = hipSuccess;
  const char *kname = "";
  if (method == BATCH_NEWTON && B->fn_wave) {
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, &du, &dr, &drc, &dit};
    const unsigned wgrid = (unsigned)((nbatch + 3) / 4);  // 4 wavefronts = 4 systems per 256-thread workgroup
    st = hipModuleLaunchKernel(B->fn_wave, wgrid, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_newton_wave";
  } else if (method == BATCH_NEWTON) {
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_newton";
  } else if (method == BATCH_TRUST_REGION && B->fn_tr_wave) {
    int ms = (int)prm[5];
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, sa[1], sa[2], sa[3], sa[4], sa[5], &ms, &du, &dr, &drc, &dit};
    const unsigned wgrid = (unsigned)((nbatch + 3) / 4);  // 4 wavefronts = 4 systems per 256-thread workgroup
    st = hipModuleLaunchKernel(B->fn_tr_wave, wgrid, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_trust_region_wave";
  } else if (method == BATCH_TRUST_REGION) {
    int ms = (int)prm[5];
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, sa[1], sa[2], sa[3], sa[4], sa[5], &ms, &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_tr, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_trust_region";
  } else if (method == BATCH_GAUSS_NEWTON) {
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_gn, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_gauss_newton";
  } else if (method == BATCH_TR_NLLS) {
    int ms = (int)prm[5];
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, sa[1], sa[2], sa[3], sa[4], sa[5], &ms, &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_tr_nlls, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_trust_region_nlls";
  } else if (method == BATCH_BROYDEN) {
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, sa[1], &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_broyden, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_broyden";
  } else if (method == BATCH_KLEMENT) {
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_klement, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_klement";
  } else {
    int M = (int)prm[3], ne = (int)prm[7];
    void *args[] = {&nb, &du0, &ups, &dp, sa[0], &maxiters, sa[1], sa[2], sa[3], &M, sa[5], sa[6], sa[7], &ne,
                    &du, &dr, &drc, &dit};
    st = hipModuleLaunchKernel(B->fn_dfsane, grid, 1, 1, B->block, 1, 1, 0, ctx->stream, args, nullptr);
    kname = "nk_batch_dfsane";
  }
  if (st != hipSuccess) NK_FAIL(NK_E_HIP, "launch of %s failed", kname);
  B->last_kernel = kname;
  if (memspace != NK_DEVICE) {
    NK_HIP(hipMemcpyAsync(u_out, du, (size_t)nbatch * n * es, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(resid_out, dr, (size_t)nbatch * nr * es, hipMemcpyDeviceToHost, ctx->stream));
  }
  // retcode / iteration outputs follow the memory space of the other arrays
  if (retcode_out)
    NK_HIP(hipMemcpyAsync(retcode_out, drc, (size_t)nbatch * sizeof(int32_t),
                          memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  if (iters_out)
    NK_HIP(hipMemcpyAsync(iters_out, dit, (size_t)nbatch * sizeof(int32_t),
                          memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  if (memspace != NK_DEVICE) NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}

// the name of the kernel the last solve on B launched: "" before any solve, NULL for a NULL object
extern "C" const char *nk_batch_last_kernel(nk_batch *B) { return B ? B->last_kernel : nullptr; }

extern "C" int nk_batch_solve(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                              double abstol, int maxiters, double *u_out, double *resid_out, int32_t *retcode_out,
                              int32_t *iters_out) {
  return batch_run(B, false, BATCH_NEWTON, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out, resid_out,
                   retcode_out, iters_out);
}

extern "C" int nk_batch_solve_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p, int memspace,
                                  double abstol, int maxiters, float *u_out, float *resid_out, int32_t *retcode_out,
                                  int32_t *iters_out) {
  return batch_run(B, true, BATCH_NEWTON, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out, resid_out,
                   retcode_out, iters_out);
}

// SimpleTrustRegion (lib/SimpleNonlinearSolve/src/trust_region.jl); thresholds/factors ≤ 0 and max_shrink_times < 0 select
// the reference defaults η₁ = 1e-4, η₂ = 0.25, η₃ = 0.75, t₁ = 0.25, t₂ = 2, 32. Retcodes: Success, MaxIters,
// ShrinkThresholdExceeded.
static void trust_region_params(double *tr, double step_threshold, double shrink_threshold, double expand_threshold,
                                double shrink_factor, double expand_factor, int max_shrink_times) {
  tr[0] = step_threshold > 0 ? step_threshold : 1e-4;
  tr[1] = shrink_threshold > 0 ? shrink_threshold : 0.25;
  tr[2] = expand_threshold > 0 ? expand_threshold : 0.75;
  tr[3] = shrink_factor > 0 ? shrink_factor : 0.25;
  tr[4] = expand_factor > 0 ? expand_factor : 2.0;
  tr[5] = (double)(max_shrink_times >= 0 ? max_shrink_times : 32);
}

extern "C" int nk_batch_solve_trust_region(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                           int memspace, double abstol, int maxiters, double step_threshold,
                                           double shrink_threshold, double expand_threshold, double shrink_factor,
                                           double expand_factor, int max_shrink_times, double *u_out, double *resid_out,
                                           int32_t *retcode_out, int32_t *iters_out) {
  double tr[6];
  trust_region_params(tr, step_threshold, shrink_threshold, expand_threshold, shrink_factor, expand_factor, max_shrink_times);
  return batch_run(B, false, BATCH_TRUST_REGION, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, tr, u_out,
                   resid_out, retcode_out, iters_out);
}

extern "C" int nk_batch_solve_trust_region_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                               int memspace, double abstol, int maxiters, double step_threshold,
                                               double shrink_threshold, double expand_threshold, double shrink_factor,
                                               double expand_factor, int max_shrink_times, float *u_out, float *resid_out,
                                               int32_t *retcode_out, int32_t *iters_out) {
  double tr[6];
  trust_region_params(tr, step_threshold, shrink_threshold, expand_threshold, shrink_factor, expand_factor, max_shrink_times);
  return batch_run(B, true, BATCH_TRUST_REGION, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, tr, u_out,
                   resid_out, retcode_out, iters_out);
}

// Least squares (m residuals, n unknowns; objects of nk_batch_create_nlls): SimpleGaussNewton and SimpleTrustRegion with
// ‖f‖₂ ≤ abstol termination; resid_out is nbatch×m
extern "C" int nk_batch_solve_gauss_newton(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                           int memspace, double abstol, int maxiters, double *u_out, double *resid_out,
                                           int32_t *retcode_out, int32_t *iters_out) {
  return batch_run(B, false, BATCH_GAUSS_NEWTON, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out,
                   resid_out, retcode_out, iters_out);
}

extern "C" int nk_batch_solve_gauss_newton_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                               int memspace, double abstol, int maxiters, float *u_out, float *resid_out,
                                               int32_t *retcode_out, int32_t *iters_out) {
  return batch_run(B, true, BATCH_GAUSS_NEWTON, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out,
                   resid_out, retcode_out, iters_out);
}

extern "C" int nk_batch_solve_trust_region_nlls(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                                int memspace, double abstol, int maxiters, double step_threshold,
                                                double shrink_threshold, double expand_threshold, double shrink_factor,
                                                double expand_factor, int max_shrink_times, double *u_out, double *resid_out,
                                                int32_t *retcode_out, int32_t *iters_out) {
  double tr[6];
  trust_region_params(tr, step_threshold, shrink_threshold, expand_threshold, shrink_factor, expand_factor, max_shrink_times);
  return batch_run(B, false, BATCH_TR_NLLS, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, tr, u_out, resid_out,
                   retcode_out, iters_out);
}

extern "C" int nk_batch_solve_trust_region_nlls_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system,
                                                    const float *p, int memspace, double abstol, int maxiters,
                                                    double step_threshold, double shrink_threshold, double expand_threshold,
                                                    double shrink_factor, double expand_factor, int max_shrink_times,
                                                    float *u_out, float *resid_out, int32_t *retcode_out, int32_t *iters_out) {
  double tr[6];
  trust_region_params(tr, step_threshold, shrink_threshold, expand_threshold, shrink_factor, expand_factor, max_shrink_times);
  return batch_run(B, true, BATCH_TR_NLLS, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, tr, u_out, resid_out,
                   retcode_out, iters_out);
}

// SimpleBroyden (broyden.jl:31-108, linesearch = nothing): alpha ≤ 0 is `nothing` (init_α from the norms of f(u0) and u0),
// else init_α = inv(alpha), taken in double as Julia takes it for a Float64 alpha.
extern "C" int nk_batch_solve_broyden(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                      int memspace, double abstol, int maxiters, double alpha, double *u_out, double *resid_out,
                                      int32_t *retcode_out, int32_t *iters_out) {
  const double prm[1] = {alpha > 0 ? 1.0 / alpha : 0.0};
  return batch_run(B, false, BATCH_BROYDEN, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, prm, u_out, resid_out,
                   retcode_out, iters_out);
}

extern "C" int nk_batch_solve_broyden_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                          int memspace, double abstol, int maxiters, double alpha, float *u_out,
                                          float *resid_out, int32_t *retcode_out, int32_t *iters_out) {
  const double prm[1] = {alpha > 0 ? 1.0 / alpha : 0.0};
  return batch_run(B, true, BATCH_BROYDEN, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, prm, u_out, resid_out,
                   retcode_out, iters_out);
}

// SimpleKlement (klement.jl:9-56): no parameters
extern "C" int nk_batch_solve_klement(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                      int memspace, double abstol, int maxiters, double *u_out, double *resid_out,
                                      int32_t *retcode_out, int32_t *iters_out) {
  return batch_run(B, false, BATCH_KLEMENT, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out, resid_out,
                   retcode_out, iters_out);
}

extern "C" int nk_batch_solve_klement_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                          int memspace, double abstol, int maxiters, float *u_out, float *resid_out,
                                          int32_t *retcode_out, int32_t *iters_out) {
  return batch_run(B, true, BATCH_KLEMENT, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, nullptr, u_out, resid_out,
                   retcode_out, iters_out);
}

// SimpleDFSane (dfsane.jl:66-172): reals ≤ 0 select the defaults σ_min = 1e-10, σ_max = 1e10, σ₁ = 1, γ = 1e-4, τ_min = 0.1,
// τ_max = 0.5; M (1..32) and n_exp (1 or 2) take 0 for their defaults 10 and 2; any other value is NK_E_INVALID.
static int dfsane_params(double *prm, double sigma_min, double sigma_max, double sigma_1, int M, double gamma, double tau_min,
                         double tau_max, int n_exp) {
  NK_REQUIRE(M >= 0 && M <= 32, "M = %d outside 1..32 (0 selects the default, 10)", M);
  NK_REQUIRE(n_exp >= 0 && n_exp <= 2, "n_exp = %d: 1 or 2 (0 selects the default, 2)", n_exp);
  prm[0] = sigma_min > 0 ? sigma_min : 1e-10;
  prm[1] = sigma_max > 0 ? sigma_max : 1e10;
  prm[2] = sigma_1 > 0 ? sigma_1 : 1.0;
  prm[3] = M > 0 ? M : 10;
  prm[4] = gamma > 0 ? gamma : 1e-4;
  prm[5] = tau_min > 0 ? tau_min : 0.1;
  prm[6] = tau_max > 0 ? tau_max : 0.5;
  prm[7] = n_exp > 0 ? n_exp : 2;
  return NK_OK;
}

extern "C" int nk_batch_solve_dfsane(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                     int memspace, double abstol, int maxiters, double sigma_min, double sigma_max,
                                     double sigma_1, int M, double gamma, double tau_min, double tau_max, int n_exp,
                                     double *u_out, double *resid_out, int32_t *retcode_out, int32_t *iters_out) {
  double prm[8];
  NK_TRY(dfsane_params(prm, sigma_min, sigma_max, sigma_1, M, gamma, tau_min, tau_max, n_exp));
  return batch_run(B, false, BATCH_DFSANE, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, prm, u_out, resid_out,
                   retcode_out, iters_out);
}

extern "C" int nk_batch_solve_dfsane_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                         int memspace, double abstol, int maxiters, double sigma_min, double sigma_max,
                                         double sigma_1, int M, double gamma, double tau_min, double tau_max, int n_exp,
                                         float *u_out, float *resid_out, int32_t *retcode_out, int32_t *iters_out) {
  double prm[8];
  NK_TRY(dfsane_params(prm, sigma_min, sigma_max, sigma_1, M, gamma, tau_min, tau_max, n_exp));
  return batch_run(B, true, BATCH_DFSANE, nbatch, u0, u0_per_system, p, memspace, abstol, maxiters, prm, u_out, resid_out,
                   retcode_out, iters_out);
}
