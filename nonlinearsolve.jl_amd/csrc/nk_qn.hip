// LimitedMemoryBroyden's low-rank inverse Jacobian on the device (lib/NonlinearSolveQuasiNewton/src/lbroyden.jl,
// initialization.jl:139-298 BroydenLowRankJacobian, broyden.jl:129-147 GoodBroydenUpdateRule):
//   J⁻¹ = a·I + U Vᵀ over the first min(idx, threshold) columns.
// Storage: U and V column by column, [threshold][ld] doubles each, ld = n rounded up to even + NK_LDV_PAD_DEFAULT, so that
// every column starts 16-byte aligned and a sweep over all columns is `threshold` unit-stride streams. A column of U is
// stored UNSCALED, Ũ_j = −J⁻¹fu_new of the step that wrote it, with its denominator in dn[j]: the reference's column is
// Ũ_j / dn[j], and the division is applied to the k coefficients instead of the n entries.
//
// One step of the solver (nk_solver.hip: lb_step) is the residual kernel plus
//   k_lb_update   vectors only: δu, u_new = u + δu, partial sums of ‖δu‖² and ‖u_new‖²
//   k_lb_reduce   ONE read of U and V: c₁ = Vᵀfu_new, c₂ = Ũᵀδu (each divided by dn), and in the same pass max|fu|, ‖fu‖²
//                 and the reset test's two any(|·| ≤ tol) flags — everything the host reads back for this step
//   k_lb_combine  ONE read of U and V: g = a·fu_new + U c₁ (= J⁻¹fu_new), z = a·δu + V c₂ (= J⁻ᵀδu); because
//                 δu = −J⁻¹fu_prev under the same J⁻¹, w = J⁻¹(fu_new − fu_prev) = g + δu and δu − w = −g: the new column pair
//                 is (−g, z) with denom = δu·w, and the next direction is −(d₀ + Ũ_new·(z·fu_new)/denom) with
//                 d₀ = g minus the evicted column's term — written by this pass, finished by the next k_lb_update.
// Reductions: per-workgroup partial sums in a fixed order, combined in a fixed order by the workgroup that draws the last
// ticket (an integer counter; no floating-point atomics): two runs give the same bits.
#include "nk_internal.h"

constexpr int LB_MAX_T = 32;        // supported threshold
constexpr int LB_MAX_GRID = 512;    // two workgroups per CU at most: the last workgroup reads (2k + 4)·grid partials
// device scalars (doubles) of a workspace
enum { LB_FNORM_INF = 0, LB_FNORM_SS = 1, LB_DU_SS = 2, LB_FLAG_DU = 3, LB_FLAG_DFU = 4, LB_U_SS = 5, LB_DENOM = 6, LB_ZETA = 7,
       LB_C1 = 8, LB_C2 = LB_C1 + LB_MAX_T, LB_NSCAL = LB_C2 + LB_MAX_T };

struct nk_lbroyden {
  nk_ctx *ctx = nullptr;
  int64_t n = 0, ld = 0;
  int T = 0, idx = 0;
  double *U = nullptr, *V = nullptr, *d0 = nullptr, *du = nullptr;
  double *sc = nullptr, *dn = nullptr, *part = nullptr, *part0 = nullptr;
  unsigned int *ticket = nullptr;
  int grid0 = 0;      // workgroups of the last k_lb_update (its partial sums are folded by the next k_lb_reduce)
  int last_col = -1;  // column the last k_lb_combine wrote
};

__device__ __forceinline__ double lb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double lb_wave_nanmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nk_nanmax(v, __shfl_xor(v, o, 64));
  return v;
}
// Hand-off of a workgroup's partial results to the workgroup that arrives last: stores drained by their wavefronts → barrier →
// agent-scope release → ticket; the last arriver acquires before anybody in it reads. True in every thread of that workgroup.
__device__ __forceinline__ bool lb_arrive_last(unsigned int *ticket, unsigned int nwg, double *s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (t == nwg - 1u);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_flag = last ? 1.0 : 0.0;
  }
  __syncthreads();
  return *s_flag != 0.0;
}

// ----------------------------------------------------------------------------- update (vectors only)
// mode 0: δu = −(a·fu)                      (idx = 0: the first step and the step after a reset)
// mode 1: δu = −(d₀ + Ũ_new·(ζ/denom))      (J⁻¹fu under the J⁻¹ the last combine pass completed)
__global__ __launch_bounds__(NK_BLOCK) void k_lb_update(int64_t n, int mode, double a, const double *__restrict__ fu,
                                                        const double *__restrict__ d0, const double *__restrict__ ucol,
                                                        const double *__restrict__ sc, const double *__restrict__ u,
                                                        double *__restrict__ unew, double *__restrict__ du,
                                                        double *__restrict__ part0) {
  __shared__ double sm[8];
  const double beta = mode ? sc[LB_ZETA] / sc[LB_DENOM] : 0.0;
  double sd = 0.0, su = 0.0;
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < n; i += stride) {
    const double d = mode ? -(d0[i] + ucol[i] * beta) : -(a * fu[i]);
    const double un = u[i] + d;
    du[i] = d;
    unew[i] = un;
    sd += d * d;
    su += un * un;
  }
  sd = lb_wave_sum(sd);
  su = lb_wave_sum(su);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[w] = sd; sm[4 + w] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part0[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    part0[gridDim.x + blockIdx.x] = (sm[4] + sm[5]) + (sm[6] + sm[7]);
  }
}

// ----------------------------------------------------------------------------- reduce pass
struct lb_reduce_args {
  int64_t n, ld;
  const double *U, *V, *x, *y, *r;   // x = fu_new, y = δu, r = the residual the reset test compares with (never NULL)
  double tol;
  const double *dn, *part0;
  int grid0;
  double *part, *sc;
  unsigned int *ticket;
};
// M = number of active columns (exact: no per-column predicate around the loads)
template <int M>
__global__ __launch_bounds__(NK_BLOCK) void k_lb_reduce(lb_reduce_args a) {
  constexpr int MA = M > 0 ? M : 1, NS = 2 * M + 4;   // slots: Vᵀx (M), Ũᵀy (M), Σx², max|x|, flag du, flag dfu
  constexpr int CH = 8;                                // columns requested together
  __shared__ double sm[4 * NS + 1];
  double av[MA], au[MA];
#pragma unroll
  for (int j = 0; j < MA; ++j) av[j] = au[j] = 0.0;
  double ss = 0.0, mx = 0.0, fdu = 0.0, fdf = 0.0;
  const int64_t npair = a.n >> 1, stride = (int64_t)gridDim.x * NK_BLOCK;
  const double2 *x2 = reinterpret_cast<const double2 *>(a.x), *y2 = reinterpret_cast<const double2 *>(a.y),
                *r2 = reinterpret_cast<const double2 *>(a.r);
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < npair; i += stride) {
    const double2 xv = x2[i], yv = y2[i], rv = r2[i];
#pragma unroll
    for (int c = 0; c < M; c += CH) {
      double2 uu[CH], vv[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (c + j < M) {
          uu[j] = reinterpret_cast<const double2 *>(a.U + (size_t)(c + j) * a.ld)[i];
          vv[j] = reinterpret_cast<const double2 *>(a.V + (size_t)(c + j) * a.ld)[i];
        }
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (c + j < M) {
          av[c + j] += vv[j].x * xv.x + vv[j].y * xv.y;
          au[c + j] += uu[j].x * yv.x + uu[j].y * yv.y;
        }
    }
    ss += xv.x * xv.x + xv.y * xv.y;
    mx = nk_nanmax(mx, nk_nanmax(fabs(xv.x), fabs(xv.y)));
    if (fabs(yv.x) <= a.tol || fabs(yv.y) <= a.tol) fdu = 1.0;
    if (fabs(xv.x - rv.x) <= a.tol || fabs(xv.y - rv.y) <= a.tol) fdf = 1.0;
  }
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd tail
    const int64_t i = a.n - 1;
    const double xv = a.x[i], yv = a.y[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      av[j] += a.V[(size_t)j * a.ld + i] * xv;
      au[j] += a.U[(size_t)j * a.ld + i] * yv;
    }
    ss += xv * xv;
    mx = nk_nanmax(mx, fabs(xv));
    if (fabs(yv) <= a.tol) fdu = 1.0;
    if (fabs(xv - a.r[i]) <= a.tol) fdf = 1.0;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double s1 = lb_wave_sum(av[j]), s2 = lb_wave_sum(au[j]);
    if (lane == 0) { sm[wid * NS + j] = s1; sm[wid * NS + M + j] = s2; }
  }
  {
    const double s = lb_wave_sum(ss), m = lb_wave_nanmax(mx), f1 = lb_wave_nanmax(fdu), f2 = lb_wave_nanmax(fdf);
    if (lane == 0) { sm[wid * NS + 2 * M] = s; sm[wid * NS + 2 * M + 1] = m; sm[wid * NS + 2 * M + 2] = f1; sm[wid * NS + 2 * M + 3] = f2; }
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    const int s = threadIdx.x;
    const double p0 = sm[s], p1 = sm[NS + s], p2 = sm[2 * NS + s], p3 = sm[3 * NS + s];
    a.part[(size_t)s * gridDim.x + blockIdx.x] = (s <= 2 * M) ? (p0 + p1) + (p2 + p3) : nk_nanmax(nk_nanmax(p0, p1), nk_nanmax(p2, p3));
  }
  if (!lb_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  // ---- the last workgroup: slot s is combined by wavefront s mod 4, workgroup partials in ascending order per lane
  const int nwg = gridDim.x;
  for (int s = wid; s < NS + 2; s += 4) {
    const bool is_max = s > 2 * M && s < NS;
    const double *p = s < NS ? a.part + (size_t)s * nwg : a.part0 + (size_t)(s - NS) * a.grid0;
    const int cnt = s < NS ? nwg : a.grid0;
    double v = 0.0;
    for (int b = lane; b < cnt; b += 64) v = is_max ? nk_nanmax(v, p[b]) : v + p[b];
    v = is_max ? lb_wave_nanmax(v) : lb_wave_sum(v);
    if (lane == 0) {
      if (s < M) a.sc[LB_C1 + s] = v / a.dn[s];
      else if (s < 2 * M) a.sc[LB_C2 + (s - M)] = v / a.dn[s - M];
      else if (s == 2 * M) a.sc[LB_FNORM_SS] = v;
      else if (s == 2 * M + 1) a.sc[LB_FNORM_INF] = v;
      else if (s == 2 * M + 2) a.sc[LB_FLAG_DU] = v;
      else if (s == 2 * M + 3) a.sc[LB_FLAG_DFU] = v;
      else if (s == NS) a.sc[LB_DU_SS] = v;
      else a.sc[LB_U_SS] = v;
    }
  }
  if (threadIdx.x == 0) *a.ticket = 0u;   // (for the next launch: the kernel boundary publishes it)
}

// ----------------------------------------------------------------------------- combine pass
struct lb_combine_args {
  int64_t n, ld;
  double *U, *V;                     // read over the M active columns, column jw written (may be one of them: the eviction)
  const double *x, *y;               // fu_new, δu
  double a;
  int jw;
  double *d0, *part, *sc, *dn;
  unsigned int *ticket;
};
// (c: the coefficient pairs {c₁[j], c₂[j]} in LDS — 2·32 of them in scalar registers spill)
template <int M>
__device__ __forceinline__ void lb_combine_one(const lb_combine_args &a, const double2 *c, const double *uu,
                                               const double *vv, double x, double y, double *gneg, double *z, double *d0,
                                               double *den, double *zeta) {
  double gex = 0.0, ge = 0.0, zz = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double2 cj = c[j];
    const double t = uu[j] * cj.x;
    if (j == a.jw) ge = t; else gex += t;
    zz += vv[j] * cj.y;
  }
  const double ax = a.a * x;
  const double g = (gex + ge) + ax;     // J⁻¹ fu_new
  zz = zz + a.a * y;                    // J⁻ᵀ δu
  const double w = g + y;               // J⁻¹ (fu_new − fu_prev)
  *den += y * w;
  *zeta += zz * x;
  *gneg = -g;
  *z = zz;
  *d0 = gex + ax;                       // J⁻¹ fu_new without the column this pass overwrites
}
template <int M>
__global__ __launch_bounds__(NK_BLOCK) void k_lb_combine(lb_combine_args a) {
  constexpr int MA = M > 0 ? M : 1;
  __shared__ double sm[9];
  __shared__ double2 c[MA];
  if ((int)threadIdx.x < M) c[threadIdx.x] = make_double2(a.sc[LB_C1 + threadIdx.x], a.sc[LB_C2 + threadIdx.x]);
  __syncthreads();
  double den = 0.0, zeta = 0.0;
  const int64_t npair = a.n >> 1, stride = (int64_t)gridDim.x * NK_BLOCK;
  const double2 *x2 = reinterpret_cast<const double2 *>(a.x), *y2 = reinterpret_cast<const double2 *>(a.y);
  double2 *uw = reinterpret_cast<double2 *>(a.U + (size_t)a.jw * a.ld), *vw = reinterpret_cast<double2 *>(a.V + (size_t)a.jw * a.ld),
          *d2 = reinterpret_cast<double2 *>(a.d0);
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < npair; i += stride) {
    const double2 xv = x2[i], yv = y2[i];
    double ux[MA], uy[MA], vx[MA], vy[MA];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double2 u = reinterpret_cast<const double2 *>(a.U + (size_t)j * a.ld)[i];
      const double2 v = reinterpret_cast<const double2 *>(a.V + (size_t)j * a.ld)[i];
      ux[j] = u.x; uy[j] = u.y; vx[j] = v.x; vy[j] = v.y;
    }
    double2 gn, z, d;
    lb_combine_one<M>(a, c, ux, vx, xv.x, yv.x, &gn.x, &z.x, &d.x, &den, &zeta);
    lb_combine_one<M>(a, c, uy, vy, xv.y, yv.y, &gn.y, &z.y, &d.y, &den, &zeta);
    uw[i] = gn;
    vw[i] = z;
    d2[i] = d;
  }
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd tail
    const int64_t i = a.n - 1;
    double uu[MA], vv[MA];
#pragma unroll
    for (int j = 0; j < M; ++j) { uu[j] = a.U[(size_t)j * a.ld + i]; vv[j] = a.V[(size_t)j * a.ld + i]; }
    double gn, z, d;
    lb_combine_one<M>(a, c, uu, vv, a.x[i], a.y[i], &gn, &z, &d, &den, &zeta);
    a.U[(size_t)a.jw * a.ld + i] = gn;
    a.V[(size_t)a.jw * a.ld + i] = z;
    a.d0[i] = d;
  }
  den = lb_wave_sum(den);
  zeta = lb_wave_sum(zeta);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sm[wid] = den; sm[4 + wid] = zeta; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    a.part[gridDim.x + blockIdx.x] = (sm[4] + sm[5]) + (sm[6] + sm[7]);
  }
  if (!lb_arrive_last(a.ticket, gridDim.x, &sm[8])) return;
  const int nwg = gridDim.x;
  if (wid < 2) {
    const double *p = a.part + (size_t)wid * nwg;
    double v = 0.0;
    for (int b = lane; b < nwg; b += 64) v += p[b];
    v = lb_wave_sum(v);
    if (lane == 0) {
      if (wid == 0) {
        if (v == 0.0) v = 1.0e-5;   // ifelse(iszero(denom), T(1.0e-5), denom)  (broyden.jl:143)
        a.sc[LB_DENOM] = v;
        a.dn[a.jw] = v;
      } else {
        a.sc[LB_ZETA] = v;
      }
    }
  }
  if (threadIdx.x == 0) *a.ticket = 0u;
}

// ----------------------------------------------------------------------------- host side
#define LB_SWITCH_0_32(m, F)                                                                                         \
  switch (m) {                                                                                                       \
    case 0: F(0); break;   case 1: F(1); break;   case 2: F(2); break;   case 3: F(3); break;   case 4: F(4); break;  \
    case 5: F(5); break;   case 6: F(6); break;   case 7: F(7); break;   case 8: F(8); break;   case 9: F(9); break;  \
    case 10: F(10); break; case 11: F(11); break; case 12: F(12); break; case 13: F(13); break; case 14: F(14); break; \
    case 15: F(15); break; case 16: F(16); break; case 17: F(17); break; case 18: F(18); break; case 19: F(19); break; \
    case 20: F(20); break; case 21: F(21); break; case 22: F(22); break; case 23: F(23); break; case 24: F(24); break; \
    case 25: F(25); break; case 26: F(26); break; case 27: F(27); break; case 28: F(28); break; case 29: F(29); break; \
    case 30: F(30); break; case 31: F(31); break; case 32: F(32); break;                                              \
    default: NK_FAIL(NK_E_INVALID, "LimitedMemoryBroyden: %d active columns", (int)(m));                              \
  }

static int lb_grid(const nk_lbroyden *W) {   // sized to the CUs: at most two workgroups each
  int cap = 2 * W->ctx->num_cus;
  if (cap > LB_MAX_GRID) cap = LB_MAX_GRID;
  return nk_grid_for(W->n >> 1, NK_BLOCK * 2, cap);
}

int nk_lb_create(nk_ctx *ctx, int64_t n, int threshold, nk_lbroyden **out) {
  NK_REQUIRE(ctx && out && n > 0, "bad argument");
  NK_REQUIRE(threshold >= 1 && threshold <= LB_MAX_T, "LimitedMemoryBroyden: threshold %d is outside 1..%d", threshold, LB_MAX_T);
  nk_lbroyden *W = new nk_lbroyden();
  auto guard = nk_make_guard(W, [](nk_lbroyden *w) { nk_lb_destroy(w); });
  W->ctx = ctx;
  W->n = n;
  W->T = threshold;
  W->ld = ((n + 1) & ~(int64_t)1) + NK_LDV_PAD_DEFAULT;
  NK_TRY(nk_dev_alloc(&W->U, (size_t)W->ld * threshold));
  NK_TRY(nk_dev_alloc(&W->V, (size_t)W->ld * threshold));
  NK_TRY(nk_dev_alloc(&W->d0, (size_t)n + 2));
  NK_TRY(nk_dev_alloc(&W->du, (size_t)n + 2));
  NK_TRY(nk_dev_alloc(&W->sc, (size_t)LB_NSCAL));
  NK_TRY(nk_dev_alloc(&W->dn, (size_t)LB_MAX_T));
  NK_TRY(nk_dev_alloc(&W->part, (size_t)(2 * LB_MAX_T + 4) * LB_MAX_GRID));
  NK_TRY(nk_dev_alloc(&W->part0, (size_t)2 * NK_MAX_RED_BLOCKS));
  NK_TRY(nk_dev_alloc(&W->ticket, (size_t)2));
  NK_HIP(nk_memset(ctx, W->sc, 0, LB_NSCAL * sizeof(double)));
  NK_HIP(nk_memset(ctx, W->du, 0, ((size_t)n + 2) * sizeof(double)));
  NK_TRY(nk_lb_restart(W));
  *out = guard.release();
  return NK_OK;
}
void nk_lb_destroy(nk_lbroyden *W) {
  if (!W) return;
  hipFree(W->U); hipFree(W->V); hipFree(W->d0); hipFree(W->du); hipFree(W->sc); hipFree(W->dn); hipFree(W->part);
  hipFree(W->part0); hipFree(W->ticket);
  delete W;
}
// idx = 0 (a reset, or a new solve); the tickets are zeroed as well, in stream order
int nk_lb_restart(nk_lbroyden *W) {
  W->idx = 0;
  W->last_col = -1;
  NK_HIP(nk_memset(W->ctx, W->ticket, 0, 2 * sizeof(unsigned int)));
  return NK_OK;
}
int nk_lb_columns(const nk_lbroyden *W) { return W->idx < W->T ? W->idx : W->T; }
int nk_lb_index(const nk_lbroyden *W) { return W->idx; }
const double *nk_lb_du(const nk_lbroyden *W) { return W->du; }

// δu = −J⁻¹ fu and u_new = u + δu. idx = 0: J⁻¹ = a·I. Otherwise the pass finishes what the last combine pass prepared,
// which is J⁻¹ applied to the residual THAT pass was given — the caller's fu must be that vector.
int nk_lb_direction(nk_lbroyden *W, double a, const double *fu, const double *u, double *u_new) {
  nk_ctx *ctx = W->ctx;
  const int mode = W->idx > 0 ? 1 : 0;
  NK_REQUIRE(!mode || W->last_col >= 0, "LimitedMemoryBroyden: no update to take the direction from");
  const int grid = nk_grid_for(W->n, NK_BLOCK * 4, NK_MAX_RED_BLOCKS);
  nk_prof_scope prof_(ctx, NK_K_NEWTON_UPDATE, (mode ? 40.0 : 32.0) * (double)W->n);
  NK_LAUNCH(ctx, k_lb_update, dim3(grid), dim3(NK_BLOCK), W->n, mode, a, fu, (const double *)W->d0,
            (const double *)(W->U + (size_t)(mode ? W->last_col : 0) * W->ld), (const double *)W->sc, u, u_new, W->du, W->part0);
  NK_HIP(hipGetLastError());
  W->grid0 = grid;
  return NK_OK;
}
// one read of U and V: the coefficients of the update, the residual's norms, the step's norms and the reset test's flags.
// `ref` is the residual the reset test last looked at. The six leading scalars are what the host fetches (nk_lb_scalars).
int nk_lb_reduce(nk_lbroyden *W, const double *fu_new, const double *ref, double tol) {
  nk_ctx *ctx = W->ctx;
  const int m = nk_lb_columns(W), grid = lb_grid(W);
  lb_reduce_args a{W->n, W->ld, W->U, W->V, fu_new, W->du, ref, tol, W->dn, W->part0, W->grid0, W->part, W->sc, W->ticket};
  nk_prof_scope prof_(ctx, NK_K_MULTIDOT, (16.0 * m + 24.0) * (double)W->n);
#define LB_F(M) NK_LAUNCH(ctx, k_lb_reduce<M>, dim3(grid), dim3(NK_BLOCK), a)
  LB_SWITCH_0_32(m, LB_F)
#undef LB_F
  NK_HIP(hipGetLastError());
  return NK_OK;
}
double *nk_lb_scalars(nk_lbroyden *W) { return W->sc; }
// one read of U and V: the new column pair (column mod1(idx + 1, threshold)), d₀, denom and z·fu_new; idx += 1
int nk_lb_combine(nk_lbroyden *W, double a, const double *fu_new) {
  nk_ctx *ctx = W->ctx;
  const int m = nk_lb_columns(W), grid = lb_grid(W), jw = W->idx % W->T;
  lb_combine_args c{W->n, W->ld, W->U, W->V, fu_new, W->du, a, jw, W->d0, W->part, W->sc, W->dn, W->ticket + 1};
  nk_prof_scope prof_(ctx, NK_K_MULTIAXPY, (16.0 * m + 40.0) * (double)W->n);
#define LB_F(M) NK_LAUNCH(ctx, k_lb_combine<M>, dim3(grid), dim3(NK_BLOCK), c)
  LB_SWITCH_0_32(m, LB_F)
#undef LB_F
  NK_HIP(hipGetLastError());
  W->last_col = jw;
  W->idx += 1;
  return NK_OK;
}
// algorithmic bytes of the two passes over U and V for m active columns (what tools/lbroyden_bench.py divides by)
double nk_lb_pass_bytes(int64_t n, int m) { return ((16.0 * m + 24.0) + (16.0 * m + 40.0)) * (double)n; }

// ============================================================================= DFSane (nk_solver.hip: sane_step)
// GeneralizedDFSane with RobustNonMonotoneLineSearch (lib/NonlinearSolveSpectralMethods/src/solve.jl:201-259, the line search as
// lib/SimpleNonlinearSolve/src/dfsane.jl:114-144 states it). The whole state is u, fu and a handful of host scalars. A trial of
// the line search is the residual kernel plus
//   k_sane_trial    x_t = x + a·(−(σ·f)), a = α₊ or −α₋: the two products are rounded one after the other, as `d = −σ f` and
//                   `x + α d` are in the literal form, so the iterate carries the literal form's bits. 16 B read, 8 B written.
//   k_sane_reduce   ONE read of f_t and f: Σf_t², max|f_t| (NaN-propagating) and Σ f·(f_t − f), the last accumulated elementwise.
// With δu = c·f, c = −aσ: ⟨δu,δu⟩ = c²·Σf², ⟨δu,δf⟩ = c·Σ f(f_t − f), ‖δu‖₂ = |c|·‖f‖₂ — acceptance, termination and the spectral
// update need nothing else, so no pass reads u to form δu or δf and the caches of the literal form are pointer swaps.
enum { SANE_SS = 0, SANE_MAX = 1, SANE_DOT = 2, SANE_NSCAL = 3 };

struct nk_sane {
  nk_ctx *ctx = nullptr;
  int64_t n = 0;
  double *sc = nullptr, *part = nullptr;
  unsigned int *ticket = nullptr;
};

__global__ __launch_bounds__(NK_BLOCK) void k_sane_trial(int64_t n, double sigma, double a, const double *__restrict__ x,
                                                         const double *__restrict__ f, double *__restrict__ xt) {
  const int64_t npair = n >> 1, stride = (int64_t)gridDim.x * NK_BLOCK;
  const double2 *x2 = reinterpret_cast<const double2 *>(x), *f2 = reinterpret_cast<const double2 *>(f);
  double2 *t2 = reinterpret_cast<double2 *>(xt);
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < npair; i += stride) {
    const double2 xv = x2[i], fv = f2[i];
    t2[i] = make_double2(xv.x + a * (-(sigma * fv.x)), xv.y + a * (-(sigma * fv.y)));
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd tail
    const int64_t i = n - 1;
    xt[i] = x[i] + a * (-(sigma * f[i]));
  }
}

struct sane_reduce_args {
  int64_t n;
  const double *ft, *f;   // the trial residual, the residual of the iterate the search started from
  double *part, *sc;
  unsigned int *ticket;
};
__global__ __launch_bounds__(NK_BLOCK) void k_sane_reduce(sane_reduce_args a) {
  constexpr int NS = SANE_NSCAL;
  __shared__ double sm[4 * NS + 1];
  double ss = 0.0, mx = 0.0, dt = 0.0;
  const int64_t npair = a.n >> 1, stride = (int64_t)gridDim.x * NK_BLOCK;
  const double2 *t2 = reinterpret_cast<const double2 *>(a.ft), *f2 = reinterpret_cast<const double2 *>(a.f);
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < npair; i += stride) {
    const double2 tv = t2[i], fv = f2[i];
    ss += tv.x * tv.x + tv.y * tv.y;
    mx = nk_nanmax(mx, nk_nanmax(fabs(tv.x), fabs(tv.y)));
    dt += fv.x * (tv.x - fv.x) + fv.y * (tv.y - fv.y);
  }
  if ((a.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd tail
    const int64_t i = a.n - 1;
    const double tv = a.ft[i], fv = a.f[i];
    ss += tv * tv;
    mx = nk_nanmax(mx, fabs(tv));
    dt += fv * (tv - fv);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  {
    const double s = lb_wave_sum(ss), m = lb_wave_nanmax(mx), d = lb_wave_sum(dt);
    if (lane == 0) { sm[wid * NS + SANE_SS] = s; sm[wid * NS + SANE_MAX] = m; sm[wid * NS + SANE_DOT] = d; }
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    const int s = threadIdx.x;
    const double p0 = sm[s], p1 = sm[NS + s], p2 = sm[2 * NS + s], p3 = sm[3 * NS + s];
    a.part[(size_t)s * gridDim.x + blockIdx.x] = (s == SANE_MAX) ? nk_nanmax(nk_nanmax(p0, p1), nk_nanmax(p2, p3)) : (p0 + p1) + (p2 + p3);
  }
  if (!lb_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  // ---- the last workgroup: slot s is combined by wavefront s, workgroup partials in ascending order per lane
  const int nwg = gridDim.x;
  if (wid < NS) {
    const bool is_max = wid == SANE_MAX;
    const double *p = a.part + (size_t)wid * nwg;
    double v = 0.0;
    for (int b = lane; b < nwg; b += 64) v = is_max ? nk_nanmax(v, p[b]) : v + p[b];
    v = is_max ? lb_wave_nanmax(v) : lb_wave_sum(v);
    if (lane == 0) a.sc[wid] = v;
  }
  if (threadIdx.x == 0) *a.ticket = 0u;   // (for the next launch: the kernel boundary publishes it)
}

static int sane_grid(const nk_sane *W) {   // sized to the CUs: at most two workgroups each
  int cap = 2 * W->ctx->num_cus;
  if (cap > LB_MAX_GRID) cap = LB_MAX_GRID;
  if (cap < 1) cap = 1;
  return nk_grid_for(W->n >> 1, NK_BLOCK * 2, cap);
}

int nk_sane_create(nk_ctx *ctx, int64_t n, nk_sane **out) {
  NK_REQUIRE(ctx && out && n > 0, "bad argument");
  nk_sane *W = new nk_sane();
  auto guard = nk_make_guard(W, [](nk_sane *w) { nk_sane_destroy(w); });
  W->ctx = ctx;
  W->n = n;
  NK_TRY(nk_dev_alloc(&W->sc, (size_t)SANE_NSCAL + 1));
  NK_TRY(nk_dev_alloc(&W->part, (size_t)SANE_NSCAL * LB_MAX_GRID));
  NK_TRY(nk_dev_alloc(&W->ticket, (size_t)1));
  NK_HIP(nk_memset(ctx, W->sc, 0, (SANE_NSCAL + 1) * sizeof(double)));
  NK_TRY(nk_sane_restart(W));
  *out = guard.release();
  return NK_OK;
}
void nk_sane_destroy(nk_sane *W) {
  if (!W) return;
  hipFree(W->sc); hipFree(W->part); hipFree(W->ticket);
  delete W;
}
// a new solve: the ticket is zeroed, in stream order
int nk_sane_restart(nk_sane *W) {
  NK_HIP(nk_memset(W->ctx, W->ticket, 0, sizeof(unsigned int)));
  return NK_OK;
}
// x_t = x + a·(−(σ·f)); out of place (x stays intact)
int nk_sane_trial(nk_sane *W, double sigma, double a, const double *x, const double *f, double *xt) {
  nk_ctx *ctx = W->ctx;
  NK_REQUIRE(xt != x && xt != f, "DFSane: the trial point is written out of place");
  const int grid = nk_grid_for(W->n >> 1, NK_BLOCK * 2, 8 * (ctx->num_cus > 0 ? ctx->num_cus : 1));
  nk_prof_scope prof_(ctx, NK_K_NEWTON_UPDATE, 24.0 * (double)W->n);
  NK_LAUNCH(ctx, k_sane_trial, dim3(grid), dim3(NK_BLOCK), W->n, sigma, a, x, f, xt);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
// one read of f_t and f; the three scalars the host fetches are nk_sane_scalars()[0..2]: Σf_t², max|f_t|, Σ f·(f_t − f)
int nk_sane_reduce(nk_sane *W, const double *ft, const double *f) {
  nk_ctx *ctx = W->ctx;
  const int grid = sane_grid(W);
  sane_reduce_args a{W->n, ft, f, W->part, W->sc, W->ticket};
  nk_prof_scope prof_(ctx, NK_K_MULTIDOT, 16.0 * (double)W->n);
  NK_LAUNCH(ctx, k_sane_reduce, dim3(grid), dim3(NK_BLOCK), a);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
double *nk_sane_scalars(nk_sane *W) { return W->sc; }
// algorithmic bytes of the two passes of one trial (what tools/dfsane_bench.py divides by)
double nk_sane_pass_bytes(int64_t n) { return 40.0 * (double)n; }
