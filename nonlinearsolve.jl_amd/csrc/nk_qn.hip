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
//
// Reductions, for the three families of this file alike: qn_block_partials leaves a workgroup's partial of every
// slot in part[slot][workgroup]; the workgroup that draws the last ticket (an integer counter; no floating-point atomics) folds
// each slot with qn_fold_slot, one wavefront per slot, and lane 0 puts the scalar where the host reads it. Every order is fixed:
// two runs give the same bits.
#include "nk_internal.h"

constexpr int LB_MAX_T = 32;        // supported threshold
constexpr int LB_MAX_GRID = 512;    // two workgroups per CU at most: the last workgroup reads (2k + 4)·grid partials
// device scalars (doubles) of a workspace
enum { LB_FNORM_INF = 0, LB_FNORM_SS = 1, LB_DU_SS = 2, LB_FLAG_DU = 3, LB_FLAG_DFU = 4, LB_U_SS = 5, LB_DENOM = 6, LB_ZETA = 7,
       LB_C1 = 8, LB_C2 = LB_C1 + LB_MAX_T, LB_NSCAL = LB_C2 + LB_MAX_T };

// the reduction workspace of a family: the scalars the host reads, the partials of its reduce passes, the partials of its
// vector (update) launch with the number of workgroups that wrote them and that nobody has folded yet (0: none), the tickets
struct qn_red {
  double *sc = nullptr, *part = nullptr, *part0 = nullptr;
  unsigned int *ticket = nullptr;
  int ntickets = 0, grid0 = 0;
};
// the tickets are zeroed in stream order (a new solve, or a reset)
static int qn_red_restart(const nk_ctx *ctx, qn_red *r) {
  r->grid0 = 0;
  NK_HIP(nk_memset(ctx, r->ticket, 0, r->ntickets * sizeof(unsigned int)));
  return NK_OK;
}
static int qn_red_alloc(const nk_ctx *ctx, qn_red *r, int nscal, int nslots, int nslots0, int ntickets) {
  r->ntickets = ntickets;
  NK_TRY(nk_dev_alloc(&r->sc, (size_t)nscal));
  NK_TRY(nk_dev_alloc(&r->part, (size_t)nslots * LB_MAX_GRID));
  NK_TRY(nk_dev_alloc(&r->part0, (size_t)nslots0 * NK_MAX_RED_BLOCKS));
  NK_TRY(nk_dev_alloc(&r->ticket, (size_t)ntickets));
  NK_HIP(nk_memset(ctx, r->sc, 0, nscal * sizeof(double)));
  return qn_red_restart(ctx, r);
}
static void qn_red_free(qn_red *r) { hipFree(r->sc); hipFree(r->part); hipFree(r->part0); hipFree(r->ticket); }
// workgroups of a reduce pass, each taking `per_wg` of `items`: sized to the CUs, at most two workgroups each
static int qn_red_grid(const nk_ctx *ctx, int64_t items, int per_wg) {
  int cap = 2 * ctx->num_cus;
  if (cap > LB_MAX_GRID) cap = LB_MAX_GRID;
  if (cap < 1) cap = 1;
  return nk_grid_for(items, per_wg, cap);
}

struct nk_lbroyden {
  nk_ctx *ctx = nullptr;
  int64_t n = 0, ld = 0;
  int T = 0, idx = 0;
  double *U = nullptr, *V = nullptr, *d0 = nullptr, *du = nullptr, *dn = nullptr;
  qn_red red;         // grid0: the last k_lb_update's, folded by the next k_lb_reduce
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
__device__ __forceinline__ double qn_denom(double v) { return v == 0.0 ? 1.0e-5 : v; }   // ifelse(iszero(denom), T(1.0e-5), denom)
// Hand-off of a workgroup's partial results to the workgroup that arrives last: stores drained by their wavefronts → barrier →
// agent-scope release → ticket; the last arriver acquires before anybody in it reads. True in every thread of that workgroup.
__device__ __forceinline__ bool qn_arrive_last(unsigned int *ticket, unsigned int nwg, double *s_flag) {
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
// (the last workgroup, once its folds are issued; for the next launch: the kernel boundary publishes it)
__device__ __forceinline__ void qn_ticket_reset(unsigned int *ticket) {
  if (threadIdx.x == 0) *ticket = 0u;
}
// A workgroup's partials of NS slots; slots s < NSUM are sums, the others NaN-propagating maxima. sm: 4·NS doubles.
// qn_store_partials: the wavefronts' values are in sm[wid·NS + s]; the four are combined pairwise, first with second and third
// with fourth, into part[s·gridDim.x + blockIdx.x]. The caller's barrier (qn_arrive_last's, or the end of the kernel) follows the store.
template <int NS, int NSUM>
__device__ __forceinline__ void qn_store_partials(const double *sm, double *part) {
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    const int s = threadIdx.x;
    const double p0 = sm[s], p1 = sm[NS + s], p2 = sm[2 * NS + s], p3 = sm[3 * NS + s];
    part[(size_t)s * gridDim.x + blockIdx.x] = s < NSUM ? (p0 + p1) + (p2 + p3) : nk_nanmax(nk_nanmax(p0, p1), nk_nanmax(p2, p3));
  }
}
// qn_block_partials: from v[s] per thread — the wave butterfly first
template <int NS, int NSUM>
__device__ __forceinline__ void qn_block_partials(const double (&v)[NS], double *sm, double *part) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double r[NS];   // (all butterflies, then one block of stores: a store between two butterflies is a branch of its own)
#pragma unroll
  for (int s = 0; s < NS; ++s) r[s] = s < NSUM ? lb_wave_sum(v[s]) : lb_wave_nanmax(v[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) sm[wid * NS + s] = r[s];
  }
  qn_store_partials<NS, NSUM>(sm, part);
}
// One wavefront folds one slot over the cnt workgroups that wrote it: lane b takes p[b], p[b + 64], … in ascending order, then
// the butterfly. The value is in every lane.
__device__ __forceinline__ double qn_fold_slot(const double *p, int cnt, bool is_max) {
  double v = 0.0;
  for (int b = threadIdx.x & 63; b < cnt; b += 64) v = is_max ? nk_nanmax(v, p[b]) : v + p[b];
  return is_max ? lb_wave_nanmax(v) : lb_wave_sum(v);
}

// ----------------------------------------------------------------------------- update (vectors only)
// mode 0: δu = −(a·fu)                      (idx = 0: the first step and the step after a reset)
// mode 1: δu = −(d₀ + Ũ_new·(ζ/denom))      (J⁻¹fu under the J⁻¹ the last combine pass completed)
__global__ __launch_bounds__(NK_BLOCK) void k_lb_update(int64_t n, int mode, double a, const double *__restrict__ fu,
                                                        const double *__restrict__ d0, const double *__restrict__ ucol,
                                                        const double *__restrict__ sc, const double *__restrict__ u,
                                                        double *__restrict__ unew, double *__restrict__ du,
                                                        double *__restrict__ part0) {
  __shared__ double sm[4 * 2];
  const double beta = mode ? sc[LB_ZETA] / sc[LB_DENOM] : 0.0;
  double acc[2] = {0.0, 0.0};   // Σδu², Σu_new²
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < n; i += stride) {
    const double d = mode ? -(d0[i] + ucol[i] * beta) : -(a * fu[i]);
    const double un = u[i] + d;
    du[i] = d;
    unew[i] = un;
    acc[0] += d * d;
    acc[1] += un * un;
  }
  qn_block_partials<2, 2>(acc, sm, part0);
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
  constexpr int MA = M > 0 ? M : 1, NS = 2 * M + 4;   // slots: Vᵀx (M), Ũᵀy (M), Σx² — sums; max|x|, flag du, flag dfu — maxima
  constexpr int NSUM = 2 * M + 1, CH = 8;              // CH: columns requested together
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
  // (the wave stage by hand: 2M + 4 accumulators handed to qn_block_partials as one array cost occupancy from M = 5 on)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwg = gridDim.x;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double s1 = lb_wave_sum(av[j]), s2 = lb_wave_sum(au[j]);
    if (lane == 0) { sm[wid * NS + j] = s1; sm[wid * NS + M + j] = s2; }
  }
  {
    const double s = lb_wave_sum(ss), m = lb_wave_nanmax(mx), f1 = lb_wave_nanmax(fdu), f2 = lb_wave_nanmax(fdf);
    if (lane == 0) { sm[wid * NS + 2 * M] = s; sm[wid * NS + 2 * M + 1] = m; sm[wid * NS + 2 * M + 2] = f1; sm[wid * NS + 2 * M + 3] = f2; }
  }
  qn_store_partials<NS, NSUM>(sm, a.part);
  if (!qn_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  // ---- the last workgroup: its NS slots, then the two sums k_lb_update left in part0
  for (int s = wid; s < NS + 2; s += 4) {
    const bool own = s < NS;
    const double v = qn_fold_slot(own ? a.part + (size_t)s * nwg : a.part0 + (size_t)(s - NS) * a.grid0, own ? nwg : a.grid0,
                                  own && s >= NSUM);
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
  qn_ticket_reset(a.ticket);
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
  __shared__ double sm[4 * 2 + 1];
  __shared__ double2 c[MA];
  if ((int)threadIdx.x < M) c[threadIdx.x] = make_double2(a.sc[LB_C1 + threadIdx.x], a.sc[LB_C2 + threadIdx.x]);
  __syncthreads();
  double acc[2] = {0.0, 0.0};
  double &den = acc[0], &zeta = acc[1];
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
  qn_block_partials<2, 2>(acc, sm, a.part);
  if (!qn_arrive_last(a.ticket, gridDim.x, &sm[4 * 2])) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwg = gridDim.x;
  for (int s = wid; s < 2; s += 4) {
    const double v = qn_fold_slot(a.part + (size_t)s * nwg, nwg, false);
    if (lane == 0) {
      if (s == 0) a.sc[LB_DENOM] = a.dn[a.jw] = qn_denom(v);   // (broyden.jl:143)
      else a.sc[LB_ZETA] = v;
    }
  }
  qn_ticket_reset(a.ticket);
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
  NK_TRY(nk_dev_alloc(&W->dn, (size_t)LB_MAX_T));
  NK_TRY(qn_red_alloc(ctx, &W->red, LB_NSCAL, 2 * LB_MAX_T + 4, 2, 2));   // tickets: the reduce pass's, the combine pass's
  NK_HIP(nk_memset(ctx, W->du, 0, ((size_t)n + 2) * sizeof(double)));
  *out = guard.release();
  return NK_OK;
}
void nk_lb_destroy(nk_lbroyden *W) {
  if (!W) return;
  hipFree(W->U); hipFree(W->V); hipFree(W->d0); hipFree(W->du); hipFree(W->dn);
  qn_red_free(&W->red);
  delete W;
}
// idx = 0 (a reset, or a new solve)
int nk_lb_restart(nk_lbroyden *W) {
  W->idx = 0;
  W->last_col = -1;
  return qn_red_restart(W->ctx, &W->red);
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
            (const double *)(W->U + (size_t)(mode ? W->last_col : 0) * W->ld), (const double *)W->red.sc, u, u_new, W->du, W->red.part0);
  NK_HIP(hipGetLastError());
  W->red.grid0 = grid;
  return NK_OK;
}
// one read of U and V: the coefficients of the update, the residual's norms, the step's norms and the reset test's flags.
// `ref` is the residual the reset test last looked at. The six leading scalars are what the host fetches (nk_lb_scalars).
int nk_lb_reduce(nk_lbroyden *W, const double *fu_new, const double *ref, double tol) {
  nk_ctx *ctx = W->ctx;
  const int m = nk_lb_columns(W), grid = qn_red_grid(ctx, W->n >> 1, NK_BLOCK * 2);
  const qn_red &r = W->red;
  lb_reduce_args a{W->n, W->ld, W->U, W->V, fu_new, W->du, ref, tol, W->dn, r.part0, r.grid0, r.part, r.sc, r.ticket};
  nk_prof_scope prof_(ctx, NK_K_MULTIDOT, (16.0 * m + 24.0) * (double)W->n);
#define LB_F(M) NK_LAUNCH(ctx, k_lb_reduce<M>, dim3(grid), dim3(NK_BLOCK), a)
  LB_SWITCH_0_32(m, LB_F)
#undef LB_F
  NK_HIP(hipGetLastError());
  return NK_OK;
}
double *nk_lb_scalars(nk_lbroyden *W) { return W->red.sc; }
// one read of U and V: the new column pair (column mod1(idx + 1, threshold)), d₀, denom and z·fu_new; idx += 1
int nk_lb_combine(nk_lbroyden *W, double a, const double *fu_new) {
  nk_ctx *ctx = W->ctx;
  const int m = nk_lb_columns(W), grid = qn_red_grid(ctx, W->n >> 1, NK_BLOCK * 2), jw = W->idx % W->T;
  lb_combine_args c{W->n, W->ld, W->U, W->V, fu_new, W->du, a, jw, W->d0, W->red.part, W->red.sc, W->dn, W->red.ticket + 1};
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
  qn_red red;   // (no vector launch leaves partials: part0 is empty)
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
  constexpr int NS = SANE_NSCAL, NSUM = 2;   // slots: Σf_t², Σ f·(f_t − f) — sums; max|f_t| — a maximum
  __shared__ double sm[4 * NS + 1];
  double acc[NS] = {0.0, 0.0, 0.0};
  double &ss = acc[0], &dt = acc[1], &mx = acc[2];
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
  qn_block_partials<NS, NSUM>(acc, sm, a.part);
  if (!qn_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwg = gridDim.x;
  for (int s = wid; s < NS; s += 4) {
    const double v = qn_fold_slot(a.part + (size_t)s * nwg, nwg, s >= NSUM);
    if (lane == 0) a.sc[s == 0 ? SANE_SS : (s == 1 ? SANE_DOT : SANE_MAX)] = v;
  }
  qn_ticket_reset(a.ticket);
}

int nk_sane_create(nk_ctx *ctx, int64_t n, nk_sane **out) {
  NK_REQUIRE(ctx && out && n > 0, "bad argument");
  nk_sane *W = new nk_sane();
  auto guard = nk_make_guard(W, [](nk_sane *w) { nk_sane_destroy(w); });
  W->ctx = ctx;
  W->n = n;
  NK_TRY(qn_red_alloc(ctx, &W->red, SANE_NSCAL + 1, SANE_NSCAL, 0, 1));
  *out = guard.release();
  return NK_OK;
}
void nk_sane_destroy(nk_sane *W) {
  if (!W) return;
  qn_red_free(&W->red);
  delete W;
}
int nk_sane_restart(nk_sane *W) { return qn_red_restart(W->ctx, &W->red); }   // a new solve
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
  const int grid = qn_red_grid(ctx, W->n >> 1, NK_BLOCK * 2);
  sane_reduce_args a{W->n, ft, f, W->red.part, W->red.sc, W->red.ticket};
  nk_prof_scope prof_(ctx, NK_K_MULTIDOT, 16.0 * (double)W->n);
  NK_LAUNCH(ctx, k_sane_reduce, dim3(grid), dim3(NK_BLOCK), a);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
double *nk_sane_scalars(nk_sane *W) { return W->red.sc; }
// algorithmic bytes of the two passes of one trial (what tools/dfsane_bench.py divides by)
double nk_sane_pass_bytes(int64_t n) { return 40.0 * (double)n; }

// ============================================================================= Broyden and Klement (nk_solver.hip: qn_step)
// Broyden (lib/NonlinearSolveQuasiNewton/src/broyden.jl:129-167) keeps the inverse Jacobian itself: a dense n×n matrix, row-major
// with ld = n rounded up to even + NK_LDV_PAD_DEFAULT so that every row starts 16-byte aligned, or its diagonal (DiagonalStructure).
// Klement (klement.jl:116-128) keeps the diagonal of J, not inverted. A step of the dense form is the residual kernel plus
//   k_qn_update   vectors: δu = −(row sums pass B left) — or −(a·fu) after a reset —, u_new = u + δu, partials of ‖δu‖², ‖u_new‖², any(|δu| ≤ tol)
//   k_qn_reduce   vectors: dfu = fu_new − fu_prev, max|fu|, ‖fu‖², ‖dfu‖², the reset test's dfu flag: what the host reads for this step
//   k_bd_pass_a   ONE READ of J⁻¹: a workgroup owns BD_R rows across all columns; it completes w = J⁻¹dfu for its rows and
//                 δu·w over them, and writes its partial column sums of z = J⁻ᵀδu to zpart[tile][·]
//   k_bd_fold     z = Σ_tiles zpart, tiles in ascending order; denom = Σ_tiles (δu·w), 1e-5 if exactly 0     (good Broyden only)
//   k_bd_pass_b   ONE READ + ONE WRITE: J⁻¹ᵢⱼ += cᵢ zⱼ, c = (δu − w)/denom, and in the same pass the row sums (J⁻¹_new fu)ᵢ
// 24·n² bytes plus 16·n²/BD_R for zpart. Bad Broyden has z = dfu and denom = ‖dfu‖²: no z pass. A reset is k_bd_fill. No workgroup
// waits for another.
constexpr int BD_R = 32;   // rows of a tile: 32 row accumulators per lane
enum { QN_FNORM_INF = 0, QN_FNORM_SS = 1, QN_DU_SS = 2, QN_FLAG_DU = 3, QN_FLAG_DFU = 4, QN_U_SS = 5, QN_DFU_SS = 6, QN_DIAG_DEN = 7,
       QN_DENOM = 8, QN_FLAG_ZERO = 9, QN_NEXT_SS = 10, QN_NSCAL = 11 };
constexpr int QN_NRED = 5, QN_NSUM = 3;   // slots a reduce pass writes per workgroup: three sums, then two maxima

struct nk_qn {
  nk_ctx *ctx = nullptr;
  int64_t n = 0, ld = 0, ldz = 0;
  int kind = 0, tiles = 0;
  double *Jm = nullptr, *zpart = nullptr;                     // the dense form: allocated by the first fill
  double *Jd = nullptr, *du = nullptr, *dnext = nullptr, *w = nullptr, *z = nullptr, *dfu = nullptr, *dpart = nullptr;
  qn_red red;          // grid0: the last k_qn_update's, until k_qn_reduce or k_kl_step has folded it
};

// ----------------------------------------------------------------------------- vectors: the step
// mode 0: δu = −(a·fu)   mode 1: δu = −src   mode 2: δu = −(Jd·fu)   mode 3: δu = −(fu/Jd);   fill: Jd = a first (a reset)
__global__ __launch_bounds__(NK_BLOCK) void k_qn_update(int64_t n, int mode, int fill, double a, double tol,
                                                        const double *__restrict__ fu, const double *__restrict__ src,
                                                        double *__restrict__ Jd, const double *__restrict__ u,
                                                        double *__restrict__ unew, double *__restrict__ du,
                                                        double *__restrict__ part0) {
  __shared__ double sm[4 * 3];
  double acc[3] = {0.0, 0.0, 0.0};   // Σδu², Σu_new², any(|δu| ≤ tol)
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < n; i += stride) {
    double d;
    if (mode == 0) d = -(a * fu[i]);
    else if (mode == 1) d = -src[i];
    else {
      double j = a;
      if (fill) Jd[i] = a; else j = Jd[i];
      d = mode == 2 ? -(j * fu[i]) : -(fu[i] / j);
    }
    const double un = u[i] + d;
    du[i] = d;
    unew[i] = un;
    acc[0] += d * d;
    acc[1] += un * un;
    if (fabs(d) <= tol) acc[2] = 1.0;
  }
  qn_block_partials<3, 2>(acc, sm, part0);
}

// the last workgroup of k_qn_reduce and k_kl_step: slot s < QN_NRED of `part`, or slot s − QN_NRED of an unfolded k_qn_update
// (the caller skips those when grid0 = 0)
__device__ __forceinline__ double qn_fold_red(const double *part, int nwg, const double *part0, int grid0, int s) {
  const bool own = s < QN_NRED;
  return qn_fold_slot(own ? part + (size_t)s * nwg : part0 + (size_t)(s - QN_NRED) * grid0, own ? nwg : grid0,
                      own ? s >= QN_NSUM : s == QN_NRED + 2);
}

// ----------------------------------------------------------------------------- vectors: what the host reads (Broyden)
struct qn_reduce_args {
  int64_t n;
  const double *x, *xp, *y, *r, *Jd;   // fu_new, fu_prev, δu, the residual the reset test compares with; Jd: NULL or the diagonal
  double tol;
  int den;                              // what sc[QN_DENOM] becomes: 0 nothing (k_bd_fold writes it), 1 ‖dfu‖² (slot 1), 2 Σ Jd·dfu·δu (slot 2)
  double *dfu;
  const double *part0;
  int grid0;
  double *part, *sc;
  unsigned int *ticket;
};
__global__ __launch_bounds__(NK_BLOCK) void k_qn_reduce(qn_reduce_args a) {
  constexpr int NS = QN_NRED;   // Σx², Σdfu², Σ (Jd·dfu)·δu, max|x|, flag dfu
  __shared__ double sm[4 * NS + 1];
  double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double &ss = acc[0], &sd = acc[1], &dd = acc[2], &mx = acc[3], &fdf = acc[4];
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < a.n; i += stride) {
    const double xv = a.x[i], df = xv - a.xp[i];
    a.dfu[i] = df;
    mx = nk_nanmax(mx, fabs(xv));
    ss += xv * xv;
    if (fabs(xv - a.r[i]) <= a.tol) fdf = 1.0;
    sd += df * df;
    if (a.Jd) dd += (a.Jd[i] * df) * a.y[i];
  }
  qn_block_partials<NS, QN_NSUM>(acc, sm, a.part);
  if (!qn_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int s = wid; s < NS + (a.grid0 ? 3 : 0); s += 4) {
    const double v = qn_fold_red(a.part, gridDim.x, a.part0, a.grid0, s);
    if (lane == 0) switch (s) {
      case 0: a.sc[QN_FNORM_SS] = v; break;
      case 1: a.sc[QN_DFU_SS] = v; if (a.den == 1) a.sc[QN_DENOM] = qn_denom(v); break;
      case 2: a.sc[QN_DIAG_DEN] = v; if (a.den == 2) a.sc[QN_DENOM] = qn_denom(v); break;
      case 3: a.sc[QN_FNORM_INF] = v; break;
      case 4: a.sc[QN_FLAG_DFU] = v; break;
      case 5: a.sc[QN_DU_SS] = v; break;
      case 6: a.sc[QN_U_SS] = v; break;
      default: a.sc[QN_FLAG_DU] = v;
    }
  }
  qn_ticket_reset(a.ticket);
}

// ----------------------------------------------------------------------------- the dense inverse: fill, pass A, fold, pass B
__global__ __launch_bounds__(NK_BLOCK) void k_bd_fill(int64_t n, int64_t ld, int64_t ldz, double a, double *__restrict__ J) {
  const int64_t hp = ldz >> 1, total = n * hp, stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t t = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; t < total; t += stride) {
    const int64_t i = t / hp, p = t - i * hp;
    reinterpret_cast<double2 *>(J + (size_t)i * ld)[p] = make_double2(2 * p == i ? a : 0.0, 2 * p + 1 == i ? a : 0.0);
  }
}

struct bd_args {
  int64_t n, ld, ldz;
  double *J;
  const double *x;       // pass A: dfu.   pass B: fu_new
  const double *du;
  double *w;             // pass A writes it, pass B reads it
  const double *z;       // pass B: z (good Broyden) or dfu (bad Broyden)
  double *zpart, *dpart; // pass A, good Broyden only (zpart NULL: no z pass)
  double *dnext;         // pass B: (J⁻¹_new fu)ᵢ
  const double *sc;
};

// a tile's sweep over all column pairs. FULL: all BD_R rows exist (no row predicate around the loads).
template <bool FULL>
__device__ __forceinline__ void bd_sweep_a(const bd_args &a, int64_t row0, int nr, const double *sdu, double (&acc)[BD_R]) {
  const int64_t npair = a.n >> 1;
  const double2 *x2 = reinterpret_cast<const double2 *>(a.x);
  double2 *zp2 = a.zpart ? reinterpret_cast<double2 *>(a.zpart + (size_t)blockIdx.x * a.ldz) : nullptr;
  for (int64_t p = threadIdx.x; p < npair; p += NK_BLOCK) {
    const double2 xv = x2[p];
    double2 zz = make_double2(0.0, 0.0);
#pragma unroll
    for (int c = 0; c < BD_R; c += 8) {
      double2 jv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (FULL || c + k < nr) jv[k] = reinterpret_cast<const double2 *>(a.J + (size_t)(row0 + c + k) * a.ld)[p];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (FULL || c + k < nr) {
          acc[c + k] += jv[k].x * xv.x + jv[k].y * xv.y;
          zz.x += jv[k].x * sdu[c + k];
          zz.y += jv[k].y * sdu[c + k];
        }
    }
    if (zp2) zp2[p] = zz;
  }
}
template <bool FULL>
__device__ __forceinline__ void bd_sweep_b(const bd_args &a, int64_t row0, int nr, const double *sc_, double (&acc)[BD_R]) {
  const int64_t npair = a.n >> 1;
  const double2 *x2 = reinterpret_cast<const double2 *>(a.x), *z2 = reinterpret_cast<const double2 *>(a.z);
  for (int64_t p = threadIdx.x; p < npair; p += NK_BLOCK) {
    const double2 xv = x2[p], zv = z2[p];
#pragma unroll
    for (int c = 0; c < BD_R; c += 8) {
      double2 jv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (FULL || c + k < nr) jv[k] = reinterpret_cast<const double2 *>(a.J + (size_t)(row0 + c + k) * a.ld)[p];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (FULL || c + k < nr) {
          jv[k].x += sc_[c + k] * zv.x;
          jv[k].y += sc_[c + k] * zv.y;
          reinterpret_cast<double2 *>(a.J + (size_t)(row0 + c + k) * a.ld)[p] = jv[k];
          acc[c + k] += jv[k].x * xv.x + jv[k].y * xv.y;
        }
    }
  }
}
// the workgroup's row sums: acc[r] over all lanes → out[r] in lanes r < BD_R of wavefront 0 (returned), fixed order
__device__ __forceinline__ double bd_row_sums(double (&acc)[BD_R], double *sm) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < BD_R; ++r) {
    const double s = lb_wave_sum(acc[r]);
    if (lane == 0) sm[wid * BD_R + r] = s;
  }
  __syncthreads();
  const int r = threadIdx.x & (BD_R - 1);
  return (sm[r] + sm[BD_R + r]) + (sm[2 * BD_R + r] + sm[3 * BD_R + r]);
}

__global__ __launch_bounds__(NK_BLOCK) void k_bd_pass_a(bd_args a) {
  __shared__ double sdu[BD_R], sm[4 * BD_R];
  const int64_t row0 = (int64_t)blockIdx.x * BD_R;
  const int nr = (int)((a.n - row0) < BD_R ? (a.n - row0) : BD_R);
  if ((int)threadIdx.x < BD_R) sdu[threadIdx.x] = (int)threadIdx.x < nr ? a.du[row0 + threadIdx.x] : 0.0;
  __syncthreads();
  double acc[BD_R];
#pragma unroll
  for (int r = 0; r < BD_R; ++r) acc[r] = 0.0;
  if (nr == BD_R) bd_sweep_a<true>(a, row0, nr, sdu, acc);
  else bd_sweep_a<false>(a, row0, nr, sdu, acc);
  if ((a.n & 1) && threadIdx.x == 0) {  // odd tail: the last column
    const int64_t j = a.n - 1;
    const double xv = a.x[j];
    double zt = 0.0;
#pragma unroll
    for (int r = 0; r < BD_R; ++r)
      if (r < nr) {
        const double v = a.J[(size_t)(row0 + r) * a.ld + j];
        acc[r] += v * xv;
        zt += v * sdu[r];
      }
    if (a.zpart) a.zpart[(size_t)blockIdx.x * a.ldz + j] = zt;
  }
  const double wr = bd_row_sums(acc, sm);
  if (threadIdx.x < 64) {
    const int r = threadIdx.x;
    double dp = 0.0;
    if (r < nr) { a.w[row0 + r] = wr; dp = sdu[r] * wr; }
    dp = lb_wave_sum(dp);
    if (r == 0 && a.dpart) a.dpart[blockIdx.x] = dp;
  }
}

// z = Σ_tiles zpart (ascending); workgroup 0 also folds δu·w and writes the denominator
__global__ __launch_bounds__(NK_BLOCK) void k_bd_fold(int64_t n, int64_t ldz, int tiles, const double *__restrict__ zpart,
                                                      const double *__restrict__ dpart, double *__restrict__ z,
                                                      double *__restrict__ sc) {
  const int64_t npair = n >> 1, p = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x;
  if (p < npair) {
    double2 zz = make_double2(0.0, 0.0);
    for (int t = 0; t < tiles; ++t) {
      const double2 v = reinterpret_cast<const double2 *>(zpart + (size_t)t * ldz)[p];
      zz.x += v.x;
      zz.y += v.y;
    }
    reinterpret_cast<double2 *>(z)[p] = zz;
  }
  if ((n & 1) && p == npair) {   // odd tail (npair < gridDim.x·NK_BLOCK: the grid covers npair + 1 lanes)
    double zt = 0.0;
    for (int t = 0; t < tiles; ++t) zt += zpart[(size_t)t * ldz + (n - 1)];
    z[n - 1] = zt;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const double v = qn_fold_slot(dpart, tiles, false);
    if (threadIdx.x == 0) sc[QN_DENOM] = qn_denom(v);
  }
}

__global__ __launch_bounds__(NK_BLOCK) void k_bd_pass_b(bd_args a) {
  __shared__ double scf[BD_R], sm[4 * BD_R];
  const int64_t row0 = (int64_t)blockIdx.x * BD_R;
  const int nr = (int)((a.n - row0) < BD_R ? (a.n - row0) : BD_R);
  if ((int)threadIdx.x < BD_R)
    scf[threadIdx.x] = (int)threadIdx.x < nr ? (a.du[row0 + threadIdx.x] - a.w[row0 + threadIdx.x]) / a.sc[QN_DENOM] : 0.0;
  __syncthreads();
  double acc[BD_R];
#pragma unroll
  for (int r = 0; r < BD_R; ++r) acc[r] = 0.0;
  if (nr == BD_R) bd_sweep_b<true>(a, row0, nr, scf, acc);
  else bd_sweep_b<false>(a, row0, nr, scf, acc);
  if ((a.n & 1) && threadIdx.x == 0) {  // odd tail: the last column
    const int64_t j = a.n - 1;
    const double xv = a.x[j], zv = a.z[j];
#pragma unroll
    for (int r = 0; r < BD_R; ++r)
      if (r < nr) {
        const double v = a.J[(size_t)(row0 + r) * a.ld + j] + scf[r] * zv;
        a.J[(size_t)(row0 + r) * a.ld + j] = v;
        acc[r] += v * xv;
      }
  }
  const double s = bd_row_sums(acc, sm);
  if ((int)threadIdx.x < nr) a.dnext[row0 + threadIdx.x] = s;
}

// the diagonal form of good Broyden (broyden.jl:149-167): J⁻¹ += (δu − t)·δu·J⁻¹/denom, t = J⁻¹·dfu·δu, denom = Σt (k_qn_reduce)
__global__ __launch_bounds__(NK_BLOCK) void k_bd_diag_update(int64_t n, double *__restrict__ Jd, const double *__restrict__ du,
                                                             const double *__restrict__ dfu, const double *__restrict__ sc) {
  const double den = sc[QN_DENOM];
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < n; i += stride) {
    const double j = Jd[i], d = du[i], t = (j * dfu[i]) * d;
    Jd[i] = j + (((d - t) * d) * j) / den;
  }
}

// ----------------------------------------------------------------------------- Klement: the whole step in one launch
// the update of J from the step just taken (klement.jl:116-128), any(iszero, J), the NEXT δu = −(fu ./ J) and u + δu, and every
// sum the host reads: max|fu|, ‖fu‖², ‖δu_next‖², ‖u‖² (for the scaling of a reset), folded by the workgroup that arrives last
struct kl_args {
  int64_t n;
  double *J, *du;                // δu: the step just taken in, the next one out
  const double *f, *fp, *u;      // fu_new, fu_prev, the iterate fu_new belongs to
  double *unew;
  const double *part0;
  int grid0;
  double *part, *sc;
  unsigned int *ticket;
};
__global__ __launch_bounds__(NK_BLOCK) void k_kl_step(kl_args a) {
  constexpr int NS = QN_NRED;   // Σf², Σδu_next², Σu², max|f|, flag zero
  __shared__ double sm[4 * NS + 1];
  double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double &ss = acc[0], &sd = acc[1], &su = acc[2], &mx = acc[3], &fz = acc[4];
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < a.n; i += stride) {
    const double f = a.f[i], d = a.du[i], uu = a.u[i];
    double j = a.J[i];
    const double j2 = j * j;
    const double jdu = j2 * (d * d);
    j = j + (((f - a.fp[i] - j * d) / (jdu == 0.0 ? 1.0e-5 : jdu)) * d) * j2;
    a.J[i] = j;
    if (j == 0.0) fz = 1.0;
    const double dn = -(f / j);
    a.du[i] = dn;
    a.unew[i] = uu + dn;
    mx = nk_nanmax(mx, fabs(f));
    ss += f * f;
    sd += dn * dn;
    su += uu * uu;
  }
  qn_block_partials<NS, QN_NSUM>(acc, sm, a.part);
  if (!qn_arrive_last(a.ticket, gridDim.x, &sm[4 * NS])) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int s = wid; s < NS + (a.grid0 ? 3 : 0); s += 4) {
    const double v = qn_fold_red(a.part, gridDim.x, a.part0, a.grid0, s);
    if (lane == 0) switch (s) {
      case 0: a.sc[QN_FNORM_SS] = v; break;
      case 1: a.sc[QN_NEXT_SS] = v; break;
      case 2: a.sc[QN_U_SS] = v; break;
      case 3: a.sc[QN_FNORM_INF] = v; break;
      case 4: a.sc[QN_FLAG_ZERO] = v; break;
      case 5: a.sc[QN_DU_SS] = v; break;
      case 6: a.sc[QN_DIAG_DEN] = v; break;   // (an unfolded k_qn_update's ‖u_new‖² is this launch's Σu² summed in another order: a slot Klement does not read)
      default: a.sc[QN_FLAG_DU] = v;
    }
  }
  qn_ticket_reset(a.ticket);
}

// ----------------------------------------------------------------------------- host side
static bool qn_dense(const nk_qn *W) { return W->kind == NK_QN_GOOD || W->kind == NK_QN_BAD; }

int nk_qn_create(nk_ctx *ctx, int64_t n, int kind, nk_qn **out) {
  NK_REQUIRE(ctx && out && n > 0, "bad argument");
  NK_REQUIRE(kind >= NK_QN_GOOD && kind <= NK_QN_KLEMENT, "bad quasi-Newton kind %d", kind);
  if ((kind == NK_QN_GOOD || kind == NK_QN_BAD) && n > NK_BROYDEN_MAX_N)
    NK_FAIL(NK_E_UNSUPPORTED, "Broyden: n = %lld is above NK_BROYDEN_MAX_N = %d (the dense inverse Jacobian would exceed 8 GiB); "
            "update_rule = diagonal, LimitedMemoryBroyden or a Jacobian-based method take such sizes", (long long)n, NK_BROYDEN_MAX_N);
  nk_qn *W = new nk_qn();
  auto guard = nk_make_guard(W, [](nk_qn *w) { nk_qn_destroy(w); });
  W->ctx = ctx;
  W->n = n;
  W->kind = kind;
  W->ldz = (n + 1) & ~(int64_t)1;
  W->ld = W->ldz + NK_LDV_PAD_DEFAULT;
  W->tiles = (int)((n + BD_R - 1) / BD_R);
  const size_t na = (size_t)n + 2;
  NK_TRY(nk_dev_alloc(&W->du, na));
  NK_TRY(nk_dev_alloc(&W->dfu, na));
  if (qn_dense(W)) {
    NK_TRY(nk_dev_alloc(&W->dnext, na));
    NK_TRY(nk_dev_alloc(&W->w, na));
    NK_TRY(nk_dev_alloc(&W->z, na));
    NK_TRY(nk_dev_alloc(&W->dpart, (size_t)W->tiles));
  } else {
    NK_TRY(nk_dev_alloc(&W->Jd, na));
    NK_HIP(nk_memset(ctx, W->Jd, 0, na * sizeof(double)));
  }
  NK_TRY(qn_red_alloc(ctx, &W->red, QN_NSCAL, QN_NRED, 3, 1));
  NK_HIP(nk_memset(ctx, W->du, 0, na * sizeof(double)));
  *out = guard.release();
  return NK_OK;
}
void nk_qn_destroy(nk_qn *W) {
  if (!W) return;
  hipFree(W->Jm); hipFree(W->zpart); hipFree(W->Jd); hipFree(W->du); hipFree(W->dnext); hipFree(W->w); hipFree(W->z);
  hipFree(W->dfu); hipFree(W->dpart);
  qn_red_free(&W->red);
  delete W;
}
int nk_qn_restart(nk_qn *W) { return qn_red_restart(W->ctx, &W->red); }   // a new solve
// J⁻¹ = a·I, write-only; the dense matrix (and zpart for good Broyden) is allocated here, by the first step of the first solve
int nk_qn_fill(nk_qn *W, double a) {
  nk_ctx *ctx = W->ctx;
  NK_REQUIRE(qn_dense(W), "not a dense Broyden workspace");
  if (!W->Jm) {
    NK_TRY(nk_dev_alloc(&W->Jm, (size_t)W->n * (size_t)W->ld));
    if (W->kind == NK_QN_GOOD) NK_TRY(nk_dev_alloc(&W->zpart, (size_t)W->tiles * (size_t)W->ldz));
  }
  const int grid = nk_grid_for(W->n * (W->ldz >> 1), NK_BLOCK * 4, 16 * (ctx->num_cus > 0 ? ctx->num_cus : 1));
  nk_prof_scope prof_(ctx, NK_K_SCALE, 8.0 * (double)W->n * (double)W->ldz);
  NK_LAUNCH(ctx, k_bd_fill, dim3(grid), dim3(NK_BLOCK), W->n, W->ld, W->ldz, a, W->Jm);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
// δu and u_new = u + δu. mode 0: −(a·fu) (the dense form after nk_qn_fill); 1: −(the row sums the last dense update left);
// 2: −(Jd·fu); 3: −(fu ./ Jd); fill: Jd = a first (modes 2, 3)
int nk_qn_direction(nk_qn *W, int mode, int fill, double a, double tol, const double *fu, const double *u, double *u_new) {
  nk_ctx *ctx = W->ctx;
  NK_REQUIRE(mode >= 0 && mode <= 3 && (mode < 2) == qn_dense(W), "quasi-Newton: direction mode %d does not fit the structure", mode);
  const int grid = nk_grid_for(W->n, NK_BLOCK * 4, NK_MAX_RED_BLOCKS);
  nk_prof_scope prof_(ctx, NK_K_NEWTON_UPDATE, 40.0 * (double)W->n);
  NK_LAUNCH(ctx, k_qn_update, dim3(grid), dim3(NK_BLOCK), W->n, mode, fill, a, tol, fu, (const double *)W->dnext, W->Jd, u, u_new,
            W->du, W->red.part0);
  NK_HIP(hipGetLastError());
  W->red.grid0 = grid;
  return NK_OK;
}
// Broyden: dfu and everything the host reads for this step (nk_qn_scalars: QN_FNORM_INF … QN_U_SS)
int nk_qn_reduce(nk_qn *W, const double *fu_new, const double *fu_prev, const double *ref, double tol) {
  nk_ctx *ctx = W->ctx;
  NK_REQUIRE(W->kind != NK_QN_KLEMENT, "Klement has no reduce pass of its own");
  const int grid = qn_red_grid(ctx, W->n, NK_BLOCK * 4);
  qn_red &r = W->red;
  qn_reduce_args a{W->n, fu_new, fu_prev, W->du, ref, W->kind == NK_QN_DIAGONAL ? W->Jd : nullptr, tol,
                   W->kind == NK_QN_BAD ? 1 : (W->kind == NK_QN_DIAGONAL ? 2 : 0), W->dfu, r.part0, r.grid0, r.part, r.sc, r.ticket};
  nk_prof_scope prof_(ctx, NK_K_OTHER, 40.0 * (double)W->n);
  NK_LAUNCH(ctx, k_qn_reduce, dim3(grid), dim3(NK_BLOCK), a);
  NK_HIP(hipGetLastError());
  r.grid0 = 0;
  return NK_OK;
}
double *nk_qn_scalars(nk_qn *W) { return W->red.sc; }
const double *nk_qn_du(const nk_qn *W) { return W->du; }
// the update of J⁻¹ from the step nk_qn_reduce looked at, and (dense) the row sums J⁻¹_new·fu_new for the next direction
int nk_qn_update(nk_qn *W, const double *fu_new) {
  nk_ctx *ctx = W->ctx;
  if (W->kind == NK_QN_DIAGONAL) {
    const int grid = nk_grid_for(W->n, NK_BLOCK * 4, NK_MAX_RED_BLOCKS);
    nk_prof_scope prof_(ctx, NK_K_MULTIAXPY, 32.0 * (double)W->n);
    NK_LAUNCH(ctx, k_bd_diag_update, dim3(grid), dim3(NK_BLOCK), W->n, W->Jd, (const double *)W->du, (const double *)W->dfu,
              (const double *)W->red.sc);
    NK_HIP(hipGetLastError());
    return NK_OK;
  }
  NK_REQUIRE(qn_dense(W) && W->Jm, "Broyden: no inverse Jacobian to update");
  const bool good = W->kind == NK_QN_GOOD;
  const double nn = (double)W->n * (double)W->n;
  bd_args a{W->n, W->ld, W->ldz, W->Jm, W->dfu, W->du, W->w, good ? W->z : W->dfu, good ? W->zpart : nullptr,
            good ? W->dpart : nullptr, W->dnext, W->red.sc};
  {
    nk_prof_scope prof_(ctx, NK_K_MULTIDOT, 8.0 * nn + (good ? 8.0 * nn / BD_R : 0.0));
    NK_LAUNCH(ctx, k_bd_pass_a, dim3(W->tiles), dim3(NK_BLOCK), a);
    NK_HIP(hipGetLastError());
  }
  if (good) {
    const int grid = (int)(((W->n >> 1) + 1 + NK_BLOCK - 1) / NK_BLOCK);
    nk_prof_scope prof_(ctx, NK_K_REDUCE_SMALL, 8.0 * nn / BD_R);
    NK_LAUNCH(ctx, k_bd_fold, dim3(grid), dim3(NK_BLOCK), W->n, W->ldz, W->tiles, (const double *)W->zpart, (const double *)W->dpart,
              W->z, W->red.sc);
    NK_HIP(hipGetLastError());
  }
  a.x = fu_new;
  {
    nk_prof_scope prof_(ctx, NK_K_MULTIAXPY, 16.0 * nn);
    NK_LAUNCH(ctx, k_bd_pass_b, dim3(W->tiles), dim3(NK_BLOCK), a);
    NK_HIP(hipGetLastError());
  }
  return NK_OK;
}
// Klement's one launch per step: the update of J from (fu_new, fu_prev, δu), the zero flag, the next δu and u_next = u + δu
int nk_qn_klement_step(nk_qn *W, const double *fu_new, const double *fu_prev, const double *u, double *u_next) {
  nk_ctx *ctx = W->ctx;
  NK_REQUIRE(W->kind == NK_QN_KLEMENT, "not a Klement workspace");
  const int grid = qn_red_grid(ctx, W->n, NK_BLOCK * 4);
  qn_red &r = W->red;
  kl_args a{W->n, W->Jd, W->du, fu_new, fu_prev, u, u_next, r.part0, r.grid0, r.part, r.sc, r.ticket};
  nk_prof_scope prof_(ctx, NK_K_MULTIAXPY, 64.0 * (double)W->n);
  NK_LAUNCH(ctx, k_kl_step, dim3(grid), dim3(NK_BLOCK), a);
  NK_HIP(hipGetLastError());
  r.grid0 = 0;
  return NK_OK;
}
// J⁻¹ as the caller's row-major n×n matrix with leading dimension ldo, or the n diagonal entries (Klement: of J)
int nk_qn_copy_matrix(nk_qn *W, double *out, int64_t ldo, int memspace) {
  nk_ctx *ctx = W->ctx;
  const hipMemcpyKind kind = memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (qn_dense(W)) {
    NK_REQUIRE(W->Jm, "Broyden: the inverse Jacobian exists from the first step on");
    NK_REQUIRE(ldo >= W->n, "leading dimension %lld is below n = %lld", (long long)ldo, (long long)W->n);
    NK_HIP(hipMemcpy2DAsync(out, (size_t)ldo * sizeof(double), W->Jm, (size_t)W->ld * sizeof(double), (size_t)W->n * sizeof(double),
                            (size_t)W->n, kind, ctx->stream));
  } else {
    NK_HIP(hipMemcpyAsync(out, W->Jd, (size_t)W->n * sizeof(double), kind, ctx->stream));
  }
  NK_HIP(hipStreamSynchronize(ctx->stream));
  return NK_OK;
}
// algorithmic bytes of the dense update's passes (what tools/broyden_bench.py divides by): pass A, the fold, pass B
void nk_qn_pass_bytes(int64_t n, int kind, double bytes[3]) {
  const double nn = (double)n * (double)n;
  const bool good = kind == NK_QN_GOOD;
  bytes[0] = 8.0 * nn + (good ? 8.0 * nn / BD_R : 0.0);
  bytes[1] = good ? 8.0 * nn / BD_R : 0.0;
  bytes[2] = 16.0 * nn;
}
