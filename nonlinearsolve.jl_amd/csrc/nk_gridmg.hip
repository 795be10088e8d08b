// Geometric multigrid V-cycle as a right preconditioner for ANY compiled grid problem on one rank (nk_grid.hip): 2-D and 3-D,
// every stencil, dof <= 4, fields, every combination of side kinds. What nk_mg.hip does for the two built-in grid problems with
// their own stencil kernels, here through the problem's CSR Jacobian fill.
//
//   levels     by REDISCRETISATION: level l is the same compiled grid problem — the same source, options and p, the fine
//              problem's code objects loaded again (nk_grid_level_create; the sizes are kernel arguments, nothing is compiled
//              twice) — on smaller sides. A_l is that problem's Jacobian fill at u_l = R u_{l−1}; its fields are the restriction
//              of the finer level's fields. CONTRACT: a source used with the multigrid takes its spacing from s.nx, s.ny, s.nz,
//              not from p; one that does not gets a poor preconditioner, never a wrong answer.
//   geometry   of one axis of n nodes, in units of the fine spacing: a side has the offset a = 1 (Dirichlet: the wall is one
//              spacing outside the outermost node), 0 (mirror_node) or ½ (mirror_face); L = n − 1 + a_lo + a_hi, node i sits at
//              a_lo + i, nc = ⌊L/2 + 1.5 − a_lo − a_hi⌋. Periodic: L = n, nc = ⌊n/2 + 0.5⌋. An axis is coarsened while
//              n > coarse_max and nc >= the stencil's smallest side (3; radius 2: 5); the hierarchy ends when no axis is.
//   transfers  tensor products of 1-D tables (nk_grid_mg_axis): linear interpolation at the nodes' positions, a coarse index
//              outside 0 … nc−1 folded by the grid's own side map (Dirichlet drops it, periodic wraps, the mirrors reflect),
//              weights on one coarse node added. Restriction = the row-normalised transpose, for residuals, u and fields alike.
//              Components one by one (vectors are component-major). One pair of kernels for 2-D and 3-D (2-D: nz = 1).
//   smoother   ν Chebyshev steps on D⁻¹A_l over [ρ/4, ρ], ρ = max_i Σ_j |a_ij| / |a_ii| computed on the device at every update
//              (a maximum needs no summation order). The recurrence of nk_cheb_run (coefficients: nk_cheb.h) with r replaced by
//              D⁻¹r: the sign of a negative-definite operator and the scales of several components need no special case. One
//              step is ONE launch: CSR row product, b − A x, the division by a_ii, the updates of d and x; x ping-pongs between
//              two buffers so that no row reads a value another row has replaced.
//   coarsest   nk_bandlu of the assembled matrix, refactored at every update.
//
// Algorithmic bytes (n rows, nnz non-zeros of the level; 8-byte values, 4-byte columns):
//   k_gmg_smooth    12·nnz + 4·n (row pointer) + 8·n·(b, 1/a_ii, x_in gathered ≈ once, d in, d out, x out) = 12·nnz + 52·n;
//                   the first step from a zero guess has no row product: 8·n·(b, 1/a_ii, d, x) = 32·n
//   k_gmg_residual  12·nnz + 4·n + 24·n
//   k_gmg_restrict  8·n_f read (every fine value belongs to <= 2^dim coarse rows, re-reads come from cache) + 8·n_c written
//   k_gmg_prolong   8·n_c read + 16·n_f (x read and written) + the 1-D tables (12 bytes per node of an axis: cached)
//   k_gmg_diag      12·nnz + 4·n + 8·n (1/a_ii)
// Restated on the CPU by tests/gridmg_reference.py.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "nk_internal.h"
#include "nk_cheb.h"

// coarse_max when the caller names none (< 3): the sweep is in DESIGN.md §6f addendum 7
constexpr int NK_GRIDMG_COARSE_MAX_DEFAULT = 8;

// ----------------------------------------------------------------------------- the 1-D table (host only)
static double gmg_side_offset(int kind) { return kind == NK_GRID_DIRICHLET0 ? 1.0 : (kind == NK_GRID_MIRROR_FACE ? 0.5 : 0.0); }

static int64_t gmg_coarse_side(int64_t n, int lo, int hi) {
  if (lo == NK_GRID_PERIODIC) return (int64_t)floor(0.5 * (double)n + 0.5);
  const double a = gmg_side_offset(lo) + gmg_side_offset(hi), L = (double)(n - 1) + a;
  return (int64_t)floor(0.5 * L + 1.5 - a);
}

extern "C" int nk_grid_mg_axis(int64_t n, int lo_kind, int hi_kind, int64_t *nc_out, int32_t *idx, double *w) {
  NK_REQUIRE(nc_out, "NULL argument");
  NK_REQUIRE(n >= 3 && n <= INT32_MAX, "n = %lld outside 3..2^31-1", (long long)n);
  NK_REQUIRE(lo_kind >= NK_GRID_DIRICHLET0 && lo_kind <= NK_GRID_MIRROR_FACE && hi_kind >= NK_GRID_DIRICHLET0 &&
             hi_kind <= NK_GRID_MIRROR_FACE, "side kinds (%d, %d): none of NK_GRID_DIRICHLET0 … NK_GRID_MIRROR_FACE", lo_kind, hi_kind);
  NK_REQUIRE((lo_kind == NK_GRID_PERIODIC) == (hi_kind == NK_GRID_PERIODIC), "an axis wraps as a whole: both of its sides must be "
             "NK_GRID_PERIODIC");
  const int64_t nc = gmg_coarse_side(n, lo_kind, hi_kind);
  NK_REQUIRE(nc >= 2, "n = %lld with sides (%d, %d) has no coarser axis", (long long)n, lo_kind, hi_kind);
  *nc_out = nc;
  if (!idx && !w) return NK_OK;
  NK_REQUIRE(idx && w, "NULL argument");
  const bool per = lo_kind == NK_GRID_PERIODIC;
  const double alo = gmg_side_offset(lo_kind), ahi = gmg_side_offset(hi_kind);
  const double L = per ? (double)n : (double)(n - 1) + alo + ahi, Lc = per ? (double)nc : (double)(nc - 1) + alo + ahi;
  for (int64_t i = 0; i < n; ++i) {
    const double t = per ? (double)i * Lc / L : (alo + (double)i) * Lc / L - alo;
    int64_t J0 = (int64_t)floor(t);
    double w1 = t - (double)J0;
    // a weight within 1e-12 of 0 or 1 is the node itself: the table does not depend on last-bit rounding
    if (w1 < 1e-12) w1 = 0.0;
    else if (w1 > 1.0 - 1e-12) { J0 += 1; w1 = 0.0; }
    const double wt[2] = {1.0 - w1, w1};
    int64_t at[2];
    double ww[2];
    for (int s = 0; s < 2; ++s) {
      at[s] = wt[s] == 0.0 ? -1 : nk_grid_side_map(J0 + s, nc, lo_kind, hi_kind);
      NK_REQUIRE(at[s] >= -1 && at[s] < nc, "internal: coarse index %lld outside the axis of %lld", (long long)at[s], (long long)nc);
      ww[s] = at[s] < 0 ? 0.0 : wt[s];
    }
    if (at[1] >= 0 && at[1] == at[0]) { ww[0] += ww[1]; at[1] = -1; ww[1] = 0.0; }   // folded onto one node: added
    for (int s = 0; s < 2; ++s) { idx[2 * i + s] = (int32_t)at[s]; w[2 * i + s] = ww[s]; }
  }
  return NK_OK;
}

// ----------------------------------------------------------------------------- the hierarchy
struct gmg_axis {   // transfers of one axis between a level (n nodes) and the next coarser one (nc nodes), on the device
  int n = 0, nc = 0;
  int32_t *pidx = nullptr;   // [2n]  prolongation: the (at most) two coarse nodes of fine node i, −1 = none
  double *pw = nullptr;      // [2n]  their weights
  int32_t *rptr = nullptr;   // [nc + 1]  restriction row I: entries rptr[I] … rptr[I + 1]
  int32_t *ridx = nullptr;   // fine node of an entry
  double *rw = nullptr;      // its normalised weight
};
struct gmg_level {
  int side[3] = {1, 1, 1};
  int64_t nn = 0, n = 0;     // nodes, unknowns
  nk_problem *P = nullptr;   // the level's problem (level 0: the caller's, not owned)
  nk_csr *A = nullptr;       // its Jacobian (level 0: own values on the problem's pattern; coarser: the level problem's own pattern)
  const double *u = nullptr; // linearisation point (level 0: the caller's vector)
  double *u_own = nullptr;
  double *b = nullptr, *xa = nullptr, *xb = nullptr, *d = nullptr, *r = nullptr, *dinv = nullptr;
  double rho = 0;
  gmg_axis ax[3];            // to the next coarser level (unused on the coarsest)
};
struct gmg_stat { unsigned long long rho_bits; int bad_row; int pad; };
struct nk_gridmg {
  nk_ctx *ctx = nullptr;
  nk_problem *P0 = nullptr;
  int nu = 2, dof = 1, nfields = 0;
  int nu_asked = 0, coarse_asked = 0;   // as the caller passed them (nk_gridmg_matches)
  std::vector<gmg_level> lv;
  nk_bandlu *LU = nullptr;
  gmg_stat *d_stat = nullptr;
};

// ----------------------------------------------------------------------------- kernels
struct gmg_dims { int nx, ny, nz, cx, cy, cz; };   // fine and coarse sides (2-D: nz = cz = 1)

// x_f += P e_c, one fine unknown per thread: the tensor product of the (at most) two entries per axis. A missing entry has the
// index −1 and the weight 0: its load is clamped to node 0 and stays unconditional
__global__ __launch_bounds__(NK_BLOCK) void k_gmg_prolong_add(gmg_dims g, int ncomp, const int32_t *__restrict__ ix,
                                                              const double *__restrict__ wx, const int32_t *__restrict__ iy,
                                                              const double *__restrict__ wy, const int32_t *__restrict__ iz,
                                                              const double *__restrict__ wz, const double *__restrict__ ec,
                                                              double *__restrict__ xf, const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int nnf = g.nx * g.ny * g.nz, nnc = g.cx * g.cy * g.cz;
  const int e = (int)blockIdx.x * NK_BLOCK + (int)threadIdx.x;
  if (e >= ncomp * nnf) return;
  const int c = e / nnf, node = e - c * nnf;
  const int k = node / (g.nx * g.ny), rem = node - k * (g.nx * g.ny), j = rem / g.nx, i = rem - j * g.nx;
  const double *src = ec + (size_t)c * nnc;
  double v = 0.0;
#pragma unroll
  for (int sz = 0; sz < 2; ++sz) {
    const int K = max(iz[2 * k + sz], 0);
    double pl = 0.0;
#pragma unroll
    for (int sy = 0; sy < 2; ++sy) {
      const int J = max(iy[2 * j + sy], 0);
      const double *line = src + ((size_t)K * g.cy + J) * g.cx;
      pl += wy[2 * j + sy] * (wx[2 * i] * line[max(ix[2 * i], 0)] + wx[2 * i + 1] * line[max(ix[2 * i + 1], 0)]);
    }
    v += wz[2 * k + sz] * pl;
  }
  xf[e] += v;
}

// r_c = R r_f, one coarse unknown per thread: the tensor product of the axes' normalised rows
__global__ __launch_bounds__(NK_BLOCK) void k_gmg_restrict(gmg_dims g, int ncomp, const int32_t *__restrict__ px,
                                                           const int32_t *__restrict__ jx, const double *__restrict__ wx,
                                                           const int32_t *__restrict__ py, const int32_t *__restrict__ jy,
                                                           const double *__restrict__ wy, const int32_t *__restrict__ pz,
                                                           const int32_t *__restrict__ jz, const double *__restrict__ wz,
                                                           const double *__restrict__ rf, double *__restrict__ rc,
                                                           const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int nnf = g.nx * g.ny * g.nz, nnc = g.cx * g.cy * g.cz;
  const int e = (int)blockIdx.x * NK_BLOCK + (int)threadIdx.x;
  if (e >= ncomp * nnc) return;
  const int c = e / nnc, node = e - c * nnc;
  const int K = node / (g.cx * g.cy), rem = node - K * (g.cx * g.cy), J = rem / g.cx, I = rem - J * g.cx;
  const double *src = rf + (size_t)c * nnf;
  double s = 0.0;
  for (int a = pz[K]; a < pz[K + 1]; ++a) {
    double pl = 0.0;
    for (int b = py[J]; b < py[J + 1]; ++b) {
      const double *line = src + ((size_t)jz[a] * g.ny + jy[b]) * g.nx;
      double row = 0.0;
      for (int t = px[I]; t < px[I + 1]; ++t) row += wx[t] * line[jx[t]];
      pl += wy[b] * row;
    }
    s += wz[a] * pl;
  }
  rc[e] = s;
}

// One Chebyshev step on D⁻¹A, one row per thread:  z = (b − A x_in)/a_ii ;  d = first ? c2·z : c1·d + c2·z ;  x_out = x_in + d.
// zero: x_in is the zero vector (never read; no row product)
__global__ __launch_bounds__(NK_BLOCK) void k_gmg_smooth(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         const double *__restrict__ val, const double *__restrict__ dinv,
                                                         const double *__restrict__ b, const double *__restrict__ xin,
                                                         double *__restrict__ d, double *__restrict__ xout, double c1, double c2,
                                                         int first, int zero, const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int i = (int)blockIdx.x * NK_BLOCK + (int)threadIdx.x;
  if (i >= n) return;
  double s = 0.0, xi = 0.0;
  if (!zero) {
    const int p1 = rowptr[i + 1];
    for (int p = rowptr[i]; p < p1; ++p) s += val[p] * xin[col[p]];
    xi = xin[i];
  }
  const double z = (b[i] - s) * dinv[i];
  const double dn = first ? c2 * z : c1 * d[i] + c2 * z;
  d[i] = dn;
  xout[i] = xi + dn;
}

// r = b − A x
__global__ __launch_bounds__(NK_BLOCK) void k_gmg_residual(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, const double *__restrict__ b,
                                                           const double *__restrict__ x, double *__restrict__ r, const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int i = (int)blockIdx.x * NK_BLOCK + (int)threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  const int p1 = rowptr[i + 1];
  for (int p = rowptr[i]; p < p1; ++p) s += val[p] * x[col[p]];
  r[i] = b[i] - s;
}

// 1/a_ii of every row, ρ = max_i Σ_j |a_ij| / |a_ii| (a non-negative double orders like its bit pattern; a NaN sorts above
// every number and so survives the maximum) and the first row whose diagonal entry is zero, missing or not finite
__global__ __launch_bounds__(NK_BLOCK) void k_gmg_diag(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ val, double *__restrict__ dinv, gmg_stat *st) {
  __shared__ unsigned long long sm[NK_BLOCK / 64];
  const int i = (int)blockIdx.x * NK_BLOCK + (int)threadIdx.x;
  double ratio = 0.0;
  if (i < n) {
    double aii = 0.0, sum = 0.0;
    const int p1 = rowptr[i + 1];
    for (int p = rowptr[i]; p < p1; ++p) {
      const double v = val[p];
      sum += fabs(v);
      aii = col[p] == i ? v : aii;
    }
    const bool bad = aii == 0.0 || !isfinite(aii);
    if (bad) atomicMin(&st->bad_row, i);
    dinv[i] = bad ? 0.0 : 1.0 / aii;
    ratio = bad ? 0.0 : sum / fabs(aii);
  }
  unsigned long long bits = (unsigned long long)__double_as_longlong(ratio);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)bits, o, 64);
    bits = other > bits ? other : bits;
  }
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int wv = 1; wv < NK_BLOCK / 64; ++wv) bits = sm[wv] > bits ? sm[wv] : bits;
    atomicMax(&st->rho_bits, bits);
  }
}

// ----------------------------------------------------------------------------- set-up
static void gmg_axis_free(gmg_axis &a) {
  hipFree(a.pidx); hipFree(a.pw); hipFree(a.rptr); hipFree(a.ridx); hipFree(a.rw);
  a = gmg_axis();
}

void nk_gridmg_destroy(nk_gridmg *M) {
  if (!M) return;
  for (size_t l = 0; l < M->lv.size(); ++l) {
    gmg_level &L = M->lv[l];
    if (l == 0) nk_csr_destroy_shared(L.A);
    else nk_problem_destroy(L.P);   // (its matrix is the level problem's own pattern)
    hipFree(L.u_own); hipFree(L.b); hipFree(L.xa); hipFree(L.xb); hipFree(L.d); hipFree(L.r); hipFree(L.dinv);
    for (gmg_axis &a : L.ax) gmg_axis_free(a);
  }
  if (M->LU) nk_bandlu_destroy(M->LU);
  hipFree(M->d_stat);
  delete M;
}

// the tables of one axis on the device; coarsen = false: the identity (the axis keeps its side)
static int gmg_axis_make(nk_ctx *ctx, int n, int lo, int hi, bool coarsen, gmg_axis *out) {
  std::vector<int32_t> idx((size_t)2 * n, -1);
  std::vector<double> w((size_t)2 * n, 0.0);
  int64_t nc = n;
  if (coarsen) NK_TRY(nk_grid_mg_axis(n, lo, hi, &nc, idx.data(), w.data()));
  else
    for (int i = 0; i < n; ++i) { idx[2 * i] = i; w[2 * i] = 1.0; }
  // the row-normalised transpose, rows by coarse node, entries in ascending fine node
  std::vector<int32_t> rptr((size_t)nc + 1, 0), ridx;
  std::vector<double> rw, sum((size_t)nc, 0.0);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < 2; ++s)
      if (idx[2 * i + s] >= 0) { rptr[idx[2 * i + s] + 1]++; sum[idx[2 * i + s]] += w[2 * i + s]; }
  for (int64_t I = 0; I < nc; ++I) {
    NK_REQUIRE(sum[I] > 0.0, "internal: coarse node %lld of an axis of %d -> %lld nodes has no fine node", (long long)I, n, (long long)nc);
    rptr[I + 1] += rptr[I];
  }
  ridx.resize((size_t)rptr[nc]);
  rw.resize((size_t)rptr[nc]);
  std::vector<int32_t> fill(rptr.begin(), rptr.end() - 1);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < 2; ++s) {
      const int I = idx[2 * i + s];
      if (I < 0) continue;
      ridx[fill[I]] = i;
      rw[fill[I]++] = w[2 * i + s] / sum[I];
    }
  out->n = n;
  out->nc = (int)nc;
  NK_TRY(nk_upload(ctx, &out->pidx, idx));
  NK_TRY(nk_upload(ctx, &out->pw, w));
  NK_TRY(nk_upload(ctx, &out->rptr, rptr));
  NK_TRY(nk_upload(ctx, &out->ridx, ridx));
  NK_TRY(nk_upload(ctx, &out->rw, rw));
  return NK_OK;
}

int nk_gridmg_create(nk_problem *P, int nu, int coarse_max, nk_gridmg **out) {
  NK_REQUIRE(P && P->grid && out, "the problem is not a compiled grid problem");
  nk_ctx *ctx = P->ctx;
  NK_REQUIRE(ctx->nranks == 1, "the multigrid preconditioner of a compiled grid problem runs on one rank, the context has %d "
             "(several ranks: the AMG preconditioner object)", ctx->nranks);
  nk_grid_shape_info sh;
  NK_TRY(nk_grid_shape(P, &sh));
  const int nu_asked = nu, coarse_asked = coarse_max;
  if (nu <= 0) nu = 2;
  if (coarse_max < 3) coarse_max = NK_GRIDMG_COARSE_MAX_DEFAULT;
  const int min_side = 2 * sh.radius + 1;
  nk_gridmg *M = new nk_gridmg();
  auto guard = nk_make_guard(M, [](nk_gridmg *g) { nk_gridmg_destroy(g); });
  M->ctx = ctx;
  M->P0 = P;
  M->nu = nu;
  M->nu_asked = nu_asked;
  M->coarse_asked = coarse_asked;
  M->dof = sh.dof;
  M->nfields = sh.nfields;
  int side[3] = {sh.n[0], sh.n[1], sh.n[2]};
  for (int l = 0; l < 40; ++l) {
    M->lv.emplace_back();
    gmg_level &L = M->lv.back();
    for (int a = 0; a < 3; ++a) L.side[a] = side[a];
    L.nn = (int64_t)side[0] * side[1] * side[2];
    L.n = L.nn * sh.dof;
    if (l == 0) {
      L.P = P;
      NK_TRY(nk_csr_share_pattern(P->user_pattern, &L.A));   // (the problem outlives its preconditioner)
    } else {
      NK_TRY(nk_grid_level_create(P, side[0], side[1], side[2], &L.P));
      L.A = L.P->user_pattern;
      NK_TRY(nk_dev_alloc(&L.u_own, (size_t)L.n));
      L.u = L.u_own;
    }
    for (double **v : {&L.b, &L.xa, &L.xb, &L.d, &L.r, &L.dinv}) {
      NK_TRY(nk_dev_alloc(v, (size_t)L.n));
      NK_HIP(nk_memset(ctx, *v, 0, (size_t)L.n * sizeof(double)));
    }
    bool coarsen[3] = {false, false, false};
    int next[3] = {side[0], side[1], side[2]};
    for (int a = 0; a < sh.dim; ++a) {
      if (side[a] <= coarse_max) continue;
      const int64_t nc = gmg_coarse_side(side[a], sh.kind[2 * a], sh.kind[2 * a + 1]);
      if (nc < min_side || nc >= side[a]) continue;
      coarsen[a] = true;
      next[a] = (int)nc;
    }
    if (!coarsen[0] && !coarsen[1] && !coarsen[2]) break;
    for (int a = 0; a < 3; ++a) NK_TRY(gmg_axis_make(ctx, side[a], sh.kind[2 * a], sh.kind[2 * a + 1], coarsen[a], &L.ax[a]));
    for (int a = 0; a < 3; ++a) side[a] = next[a];
  }
  NK_TRY(nk_dev_alloc(&M->d_stat, M->lv.size()));
  if (M->lv.size() > 1) {
    if (nk_bandlu_create(M->lv.back().A, &M->LU, 1) != NK_OK) {   // the band LU, as nk_mg.hip: a handful of block columns
      const std::string why = nk_last_error();
      const gmg_level &C = M->lv.back();
      NK_FAIL(NK_E_INVALID, "multigrid: the coarsest level (%d x %d x %d, %lld unknowns) does not fit the band solver — choose a "
              "smaller coarse_max (%s)", C.side[0], C.side[1], C.side[2], (long long)C.n, why.c_str());
    }
  }
  *out = guard.release();
  return NK_OK;
}

// ----------------------------------------------------------------------------- transfers
static gmg_dims gmg_dims_of(const gmg_level &F, const gmg_level &C) {
  return {F.side[0], F.side[1], F.side[2], C.side[0], C.side[1], C.side[2]};
}
static int gmg_restrict(nk_gridmg *M, gmg_level &F, gmg_level &C, int ncomp, const double *src, double *dst, const int *d_skip) {
  const gmg_axis *a = F.ax;
  NK_LAUNCH(M->ctx, k_gmg_restrict, nk_grid1(C.nn * ncomp), dim3(NK_BLOCK), gmg_dims_of(F, C), ncomp, (const int32_t *)a[0].rptr,
            (const int32_t *)a[0].ridx, (const double *)a[0].rw, (const int32_t *)a[1].rptr, (const int32_t *)a[1].ridx,
            (const double *)a[1].rw, (const int32_t *)a[2].rptr, (const int32_t *)a[2].ridx, (const double *)a[2].rw, src, dst, d_skip);
  NK_HIP(hipGetLastError());
  return NK_OK;
}
static int gmg_prolong_add(nk_gridmg *M, gmg_level &F, gmg_level &C, const double *ec, double *xf, const int *d_skip) {
  const gmg_axis *a = F.ax;
  NK_LAUNCH(M->ctx, k_gmg_prolong_add, nk_grid1(F.n), dim3(NK_BLOCK), gmg_dims_of(F, C), M->dof, (const int32_t *)a[0].pidx,
            (const double *)a[0].pw, (const int32_t *)a[1].pidx, (const double *)a[1].pw, (const int32_t *)a[2].pidx,
            (const double *)a[2].pw, ec, xf, d_skip);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// new linearisation point (or new fields, or a new p): restrict u and every field down the hierarchy, copy the fine problem's p
// to the levels, refill every A_l, recompute 1/a_ii and ρ, refactor the coarsest level
int nk_gridmg_update(nk_gridmg *M, const double *d_u) {
  nk_ctx *ctx = M->ctx;
  const int nl = (int)M->lv.size();
  M->lv[0].u = d_u;
  nk_grid_shape_info fs, cs;
  for (int l = 0; l + 1 < nl; ++l) {
    gmg_level &F = M->lv[l], &C = M->lv[l + 1];
    NK_TRY(gmg_restrict(M, F, C, M->dof, F.u, C.u_own, nullptr));
    if (M->nfields > 0) {
      NK_TRY(nk_grid_shape(F.P, &fs));
      NK_TRY(nk_grid_shape(C.P, &cs));
      NK_TRY(gmg_restrict(M, F, C, M->nfields, fs.d_fields, cs.d_fields, nullptr));
    }
    NK_TRY(nk_grid_level_sync_params(M->P0, C.P));
  }
  std::vector<gmg_stat> st((size_t)nl);
  for (gmg_stat &s : st) { s.rho_bits = 0ull; s.bad_row = INT32_MAX; s.pad = 0; }
  NK_HIP(hipMemcpyAsync(M->d_stat, st.data(), st.size() * sizeof(gmg_stat), hipMemcpyHostToDevice, ctx->stream));
  for (int l = 0; l < nl; ++l) {
    gmg_level &L = M->lv[l];
    NK_TRY(nk_problem_jac_values_dev(L.P, L.u, L.A));
    NK_LAUNCH(ctx, k_gmg_diag, nk_grid1(L.n), dim3(NK_BLOCK), (int)L.n, (const int32_t *)L.A->d_rowptr, (const int32_t *)L.A->d_col,
              (const double *)L.A->d_val, L.dinv, M->d_stat + l);
  }
  NK_HIP(hipGetLastError());
  NK_HIP(nk_memcpy(ctx, st.data(), M->d_stat, st.size() * sizeof(gmg_stat), hipMemcpyDeviceToHost));
  for (int l = 0; l < nl; ++l) {
    gmg_level &L = M->lv[l];
    NK_REQUIRE(st[l].bad_row == INT32_MAX, "multigrid: level %d (%d x %d x %d): the diagonal entry of row %d is zero or not finite "
               "(the Jacobi-Chebyshev smoother divides by it)", l, L.side[0], L.side[1], L.side[2], st[l].bad_row);
    memcpy(&L.rho, &st[l].rho_bits, sizeof(double));
    NK_REQUIRE(isfinite(L.rho) && L.rho > 0.0, "multigrid: level %d (%d x %d x %d): the Jacobian has entries that are not finite", l,
               L.side[0], L.side[1], L.side[2]);
  }
  if (M->LU) {
    int ok = 0;
    NK_TRY(nk_bandlu_factor(M->LU, M->lv.back().A, &ok));
    NK_REQUIRE(ok, "multigrid: the coarsest Jacobian has a zero pivot");
  }
  return NK_OK;
}

// ----------------------------------------------------------------------------- the cycle
// ν Chebyshev steps for A x = b on level L from *x (zero_guess: from 0). x ping-pongs: the result is in *x afterwards; the
// last step may be told to write into `last_out` instead
static int gmg_smooth(nk_gridmg *M, gmg_level &L, const double *b, bool zero_guess, double **x, double *last_out, const int *d_skip) {
  nk_ctx *ctx = M->ctx;
  nk_cheb_coef co(L.rho / 4.0, L.rho);
  double *cur = *x;
  for (int k = 0; k < M->nu; ++k) {
    double c1 = 0.0, c2 = co.inv_theta();
    if (k > 0) co.next(&c1, &c2);
    double *nxt = (k == M->nu - 1 && last_out) ? last_out : (cur == L.xa ? L.xb : L.xa);
    NK_LAUNCH(ctx, k_gmg_smooth, nk_grid1(L.n), dim3(NK_BLOCK), (int)L.n, (const int32_t *)L.A->d_rowptr, (const int32_t *)L.A->d_col,
              (const double *)L.A->d_val, (const double *)L.dinv, b, (const double *)cur, L.d, nxt, c1, c2, k == 0 ? 1 : 0,
              (zero_guess && k == 0) ? 1 : 0, d_skip);
    cur = nxt;
  }
  *x = cur;
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// dst = V-cycle(src), src ≠ dst. Shaped as nk_mg.hip's mg_vcycle_body; plain launches
int nk_gridmg_apply(nk_gridmg *M, const double *src, double *dst, const int *d_skip) {
  nk_ctx *ctx = M->ctx;
  NK_REQUIRE(src != dst, "multigrid: the V-cycle does not run in place");
  const int nl = (int)M->lv.size();
  std::vector<double *> x((size_t)nl, nullptr);
  if (nl == 1) {   // a single (small) level: smoothing only
    x[0] = M->lv[0].xa;
    return gmg_smooth(M, M->lv[0], src, true, &x[0], dst, d_skip);
  }
  for (int l = 0; l + 1 < nl; ++l) {
    gmg_level &F = M->lv[l], &C = M->lv[l + 1];
    const double *b = l == 0 ? src : F.b;
    x[l] = F.xa;
    NK_TRY(gmg_smooth(M, F, b, true, &x[l], nullptr, d_skip));
    NK_LAUNCH(ctx, k_gmg_residual, nk_grid1(F.n), dim3(NK_BLOCK), (int)F.n, (const int32_t *)F.A->d_rowptr, (const int32_t *)F.A->d_col,
              (const double *)F.A->d_val, b, (const double *)x[l], F.r, d_skip);
    NK_TRY(gmg_restrict(M, F, C, M->dof, F.r, C.b, d_skip));
  }
  {
    gmg_level &C = M->lv[nl - 1];
    x[nl - 1] = C.xa;
    NK_TRY(nk_bandlu_solve(M->LU, C.b, C.xa));
  }
  for (int l = nl - 2; l >= 0; --l) {
    gmg_level &F = M->lv[l], &C = M->lv[l + 1];
    NK_TRY(gmg_prolong_add(M, F, C, x[l + 1], x[l], d_skip));
    NK_TRY(gmg_smooth(M, F, l == 0 ? src : F.b, false, &x[l], l == 0 ? dst : nullptr, d_skip));
  }
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// ----------------------------------------------------------------------------- inspection
int nk_gridmg_levels(const nk_gridmg *M) { return (int)M->lv.size(); }
// was the hierarchy built for this problem with these arguments?
bool nk_gridmg_matches(const nk_gridmg *M, const nk_problem *P, int nu, int coarse_max) {
  return M->P0 == P && M->nu_asked == nu && M->coarse_asked == coarse_max;
}
int nk_gridmg_level_info(const nk_gridmg *M, int l, int64_t *sides3, int64_t *n, int64_t *nnz, double *rho) {
  NK_REQUIRE(l >= 0 && l < (int)M->lv.size(), "level %d outside 0..%d", l, (int)M->lv.size() - 1);
  const gmg_level &L = M->lv[l];
  if (sides3) for (int a = 0; a < 3; ++a) sides3[a] = L.side[a];
  if (n) *n = L.n;
  if (nnz) *nnz = L.A->nnz;
  if (rho) *rho = L.rho;
  return NK_OK;
}
nk_csr *nk_gridmg_level_matrix(const nk_gridmg *M, int l) { return l >= 0 && l < (int)M->lv.size() ? M->lv[l].A : nullptr; }
nk_problem *nk_gridmg_level_problem(const nk_gridmg *M, int l) { return l >= 0 && l < (int)M->lv.size() ? M->lv[l].P : nullptr; }
