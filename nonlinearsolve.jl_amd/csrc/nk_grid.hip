// Compiled grid problems: a residual given pointwise on a 2-D grid through a radius-1 stencil, handed over as HIP C++ source
//     template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f);
// and compiled at run time (hiprtc, gfx950) into three kernels — the full-size analogue of what nk_batch_create does for
// ensembles, and of what the reference gets from `f` alone: SciMLJacobianOperators derives J·v with forward-mode duals, sparse
// AD fills jac_prototype.
//
//   nk_grid_residual   T = nk_real                              16 bytes per unknown (u, f)
//   nk_grid_jvp        T = Dual, NK_CH = 1: value u, partial v  24 bytes per unknown (u, v, Jv) — exact, one launch
//   nk_grid_jac        T = Dual, NK_CH = npts·dof, unit seeds   8·nnz/n + 8 bytes per unknown (+ 4 for the row pointer)
//
// One grid node per thread, all `dof` components of the node; 256 threads per workgroup, nodes in lexicographic order, so a
// wavefront's loads of a stencil point are 64 consecutive doubles. The neighbourhood is loaded up front into
// nk_nbhd<T>::val[npts·dof] from clamped (Dirichlet) or wrapped (periodic) addresses — every load unconditional, the Dirichlet
// zero applied by a select, as bratu_lap does with its weights — so all loads of a node are in flight together. The unit seeds
// of the Jacobian kernel are compile-time constants: the compiler folds them, and what is left of the 20-partial duals is the
// handful of derivative expressions the source really has.
//
// The result is an nk_problem of the callback kind NK_PROBLEM_USER whose callbacks are the three launchers below, with
// user_pattern set to the stencil's CSR pattern: every consumer (nk_problem_jvp_dev, user_lin_J, the solver, GMRES) treats it as
// it treats any callback problem. Jᵀv is user_lin_J + nk_csr_spmv_t_dev. One rank.
//
// Where a row's partials go: the pattern has ascending columns, i.e. component-major, then ascending node index. Inside the grid
// the stencil points are numbered in that order already; at a periodic edge wrap-around reorders them, at a Dirichlet edge some
// are missing. Each thread counts, for every stencil point, the in-domain points with a smaller node index (npts² integer
// compares on registers) instead of reading a per-node slot table: the fill is bound by its 8·nnz bytes of stores, and a table
// would add npts bytes per node to the stream for something 25 (81) compares give.
//
// Three dimensions (nk_problem_create_grid3): the same three kernels over nk_nbhd3<T> / nk_site3 = {i, j, k, nx, ny, nz} —
// nk_grid3_residual, nk_grid3_jvp, nk_grid3_jac — from source strings of their own, so the 2-D programs are compiled from the
// text and the options they always had. 7-point star (dof 1..4) or 27-point box (dof 1): at most 28 partials per row, and the
// staged fill's LDS is at most 256·28 doubles (57344 bytes). Unknown c of node (i, j, k) is element c·nn + (k·ny + j)·nx + i;
// the flat 256-thread workgroups walk that order, so a wavefront still loads 64 consecutive doubles per stencil point.
//
// Radius 2 (NK_GRID_STAR2 = 16, NK_GRID_DIAMOND2 = 17; bit 16 of the stencil code): the same kernels once more. Only four things
// know the radius — the offset tables nk_pt_di/dj/dk, nk_nbhd::operator() with its NaN rule, the periodic wrap (± n instead of
// "the other end") and the argument checks — so the radius-2 programs get types strings of their own (k_grid_types_r2,
// k_grid3_types_r2), the wrap piece k_grid_wrap_r2 between the two pieces of the kernels' text, and one more option,
// -DNK_STENCIL=<code>. The radius-1 programs are put together from the same bytes and options as before (hiprtc derives a unit id
// from the text, comments included: even a changed comment would change their code objects). 2-D: the 9-point star with dof 1..2
// (18 partials) and the 13-point diamond |di| + |dj| <= 2 with dof 1; 3-D: the 13-point star with dof 1..2 (26 partials, staged
// LDS 53248 bytes). Every side >= 5, so that the five offsets of a direction are five distinct columns on the torus.
//
// Fields (nk_problem_create_grid_fields, nfields = 1..4): read-only arrays of one double per node — a previous time level, a
// coefficient, a source term — which the source reads as a(di, dj, k) through the stencil's own offsets:
//     template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, nk_site s, T *f);
// Field k of node m is element k·nn + m of one buffer the problem owns (zero until nk_problem_set_field). The field neighbourhood
// is loaded like u's — unconditionally, from the same idx[q], before the source runs — but without the select: outside a
// Dirichlet boundary the clamped address is the node itself, and that value is what a field reads there (a face average
// 0.5·(a(0,0) + a(1,0)) becomes a(0,0) at the wall); a periodic index wraps. A field value is an nk_real in all three kernels:
// fields are constants of the differentiation. A load whose value the source never reads is dropped by the compiler (the
// neighbourhood is a fully unrolled register array), so a declared field costs nothing until it is read. Per unknown, with r the
// number of distinct fields the source reads: residual 16 + 8·r/dof bytes, JVP 24 + 8·r/dof, fill its figure + 8·r/dof (a field
// line read by three lines of threads comes from cache, as for u). These programs carry -DNK_NFIELDS=<k>, one string of field
// text after the types and two small pieces between the pieces of the kernels' text; the programs without fields are put
// together from the same bytes and options as before.
#include <math.h>
#include <string.h>

#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)
static const char *k_grid_types = R"NKSRC(
// ---- compiled grid problems: the node's position and its neighbourhood
#if NK_BOX
#define NK_NPTS 9
#else
#define NK_NPTS 5
#endif
struct nk_site { int i, j, nx, ny; };
// stencil point q → offset; q ascends with the node index (j·nx + i) of the point inside the grid:
// star S W C E N, box row by row
__device__ constexpr int nk_pt_di(int q) { return NK_BOX ? q % 3 - 1 : (q == 1 ? -1 : (q == 3 ? 1 : 0)); }
__device__ constexpr int nk_pt_dj(int q) { return NK_BOX ? q / 3 - 1 : (q == 0 ? -1 : (q == 4 ? 1 : 0)); }
template <typename T>
struct nk_nbhd {
  T val[NK_NPTS * NK_DOF];
  // component c at node (i + di, j + dj); di, dj ∈ {−1, 0, 1} (compile-time constants keep val in registers)
  __device__ __forceinline__ T operator()(int di, int dj, int c = 0) const {
#if NK_BOX
    return val[((dj + 1) * 3 + (di + 1)) * NK_DOF + c];
#else
    if (di != 0 && dj != 0) return T(NK_R(__builtin_nan("")));   // the star has no corners: a wrong source shows at once
    return val[(dj != 0 ? 2 + 2 * dj : 2 + di) * NK_DOF + c];
#endif
  }
};
)NKSRC";

// radius 2 (NK_GRID_STAR2, NK_GRID_DIAMOND2): the programs of these stencils carry -DNK_STENCIL=<code> and get this text in
// place of k_grid_types; the radius-1 programs are compiled from the text and the options they always had.
static const char *k_grid_types_r2 = R"NKSRC(
// ---- compiled grid problems, radius 2: the node's position and its neighbourhood
#if NK_STENCIL == 17
#define NK_NPTS 13
#else
#define NK_NPTS 9
#endif
struct nk_site { int i, j, nx, ny; };
// stencil point q → offset; q ascends with the node index (j·nx + i) of the point inside the grid:
// star2    (0,−2) (0,−1) (−2,0) (−1,0) C (1,0) (2,0) (0,1) (0,2)
// diamond2 (0,−2) (−1,−1) (0,−1) (1,−1) (−2,0) (−1,0) C (1,0) (2,0) (−1,1) (0,1) (1,1) (0,2)
#if NK_STENCIL == 17
__device__ constexpr int nk_pt_di(int q) { return q == 0 || q == 12 ? 0 : (q <= 3 ? q - 2 : (q <= 8 ? q - 6 : q - 10)); }
__device__ constexpr int nk_pt_dj(int q) { return q == 0 ? -2 : (q <= 3 ? -1 : (q <= 8 ? 0 : (q <= 11 ? 1 : 2))); }
#else
__device__ constexpr int nk_pt_di(int q) { return q >= 2 && q <= 6 ? q - 4 : 0; }
__device__ constexpr int nk_pt_dj(int q) { return q < 2 ? q - 2 : (q > 6 ? q - 6 : 0); }
#endif
template <typename T>
struct nk_nbhd {
  T val[NK_NPTS * NK_DOF];
  // component c at node (i + di, j + dj); di, dj ∈ {−2, …, 2} (compile-time constants keep val in registers). A read outside
  // the stencil's shape returns NaN: a wrong source shows at once
  __device__ __forceinline__ T operator()(int di, int dj, int c = 0) const {
    const int ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj;
#if NK_STENCIL == 17
    if (ai + aj > 2) return T(NK_R(__builtin_nan("")));
    return val[(aj == 2 ? 6 + 3 * dj : 6 + 4 * dj + di) * NK_DOF + c];
#else
    if ((di != 0 && dj != 0) || ai > 2 || aj > 2) return T(NK_R(__builtin_nan("")));
    return val[(dj != 0 ? (dj < 0 ? 2 + dj : 6 + dj) : 4 + di) * NK_DOF + c];
#endif
  }
};
)NKSRC";

static const char *k_grid_kernels_a = R"NKSRC(
// ---- generated kernels: one node per thread
#define NK_GRID_BLOCK 256
// node index of every stencil point (clamped to the node itself outside a Dirichlet boundary, wrapped at a periodic one) and
// whether the point is in the domain
__device__ __forceinline__ void nk_grid_geom(int i, int j, int nx, int ny, int (&idx)[NK_NPTS], bool (&in)[NK_NPTS]) {
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int ii = i + nk_pt_di(q), jj = j + nk_pt_dj(q);
#if NK_PERIODIC
)NKSRC";
// the periodic wrap, the one piece of the kernels' text that depends on the radius: with k_grid_wrap_r1 between the two pieces
// the radius-1 programs are compiled from the very text they always had; an offset of ±2 wraps by ± n
static const char *k_grid_wrap_r1 = R"NKSRC(    ii = ii < 0 ? nx - 1 : (ii >= nx ? 0 : ii);
    jj = jj < 0 ? ny - 1 : (jj >= ny ? 0 : jj);
)NKSRC";
static const char *k_grid_wrap_r2 = R"NKSRC(    ii = ii < 0 ? ii + nx : (ii >= nx ? ii - nx : ii);
    jj = jj < 0 ? jj + ny : (jj >= ny ? jj - ny : jj);
)NKSRC";
static const char *const k_grid_kernels_b[] = {R"NKSRC(    in[q] = true;
#else
    in[q] = ii >= 0 && ii < nx && jj >= 0 && jj < ny;
    ii = in[q] ? ii : i;
    jj = in[q] ? jj : j;
#endif
    idx[q] = jj * nx + ii;
  }
}

#if NK_GRID_SET == 0
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid_residual(int nx, int ny, const nk_real *__restrict__ p, )NKSRC",
    R"NKSRC(const nk_real *__restrict__ u, nk_real *__restrict__ f) {
  const int nn = nx * ny, node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  const int j = (int)((unsigned)node / (unsigned)nx), i = node - j * nx;
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(i, j, nx, ny, idx, in);
  nk_nbhd<nk_real> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]];
      nb.val[q * NK_DOF + c] = in[q] ? x : NK_R(0);
    }
  }
  nk_real out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = NK_R(0);
  const nk_site s = {i, j, nx, ny};
  nk_point<nk_real>(nb, )NKSRC", R"NKSRC(p, s, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) f[c * nn + node] = out[c];
}

// J(u)·v exactly: the value of every neighbour from u, its one partial from v
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid_jvp(int nx, int ny, const nk_real *__restrict__ p, )NKSRC",
    R"NKSRC(const nk_real *__restrict__ u, const nk_real *__restrict__ v,
            nk_real *__restrict__ jv) {
  const int nn = nx * ny, node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  const int j = (int)((unsigned)node / (unsigned)nx), i = node - j * nx;
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(i, j, nx, ny, idx, in);
  nk_nbhd<Dual> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]], d = v[c * nn + idx[q]];
      nb.val[q * NK_DOF + c].v = in[q] ? x : NK_R(0);
      nb.val[q * NK_DOF + c].d[0] = in[q] ? d : NK_R(0);
    }
  }
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  const nk_site s = {i, j, nx, ny};
  nk_point<Dual>(nb, )NKSRC", R"NKSRC(p, s, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) jv[c * nn + node] = out[c].d[0];
}
#else
// The values of J(u) on the stencil's CSR pattern (ascending columns): slot q·dof + c of the duals carries ∂/∂u_c(point q).
// Row c·nn + node holds, for c' = 0 … dof−1, its in-domain points in ascending node order: position c'·cnt + rank[q].
// NK_GRID_DIRECT = 0: the workgroup's rows of one component are one contiguous piece of the value array — they are put together
// in LDS and stored as whole lines (k_bratu_jac's way); 1: every thread stores its own partials, 8 bytes at a stride of a row.
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid_jac(int nx, int ny, const nk_real *__restrict__ p, )NKSRC",
    R"NKSRC(const nk_real *__restrict__ u, const int *__restrict__ rowptr,
            nk_real *__restrict__ vals) {
  const int nn = nx * ny, node0 = (int)blockIdx.x * NK_GRID_BLOCK, node_t = node0 + (int)threadIdx.x;
  if (node0 >= nn) return;   // (a workgroup past the grid; the launch has none)
  const bool live = node_t < nn;
#if NK_GRID_DIRECT
  if (!live) return;
#else
  __shared__ nk_real sv[NK_GRID_BLOCK * NK_NPTS * NK_DOF];
#endif
  const int node = live ? node_t : nn - 1;   // (past the end: the last node again, nothing of it is kept)
  const int j = (int)((unsigned)node / (unsigned)nx), i = node - j * nx;
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(i, j, nx, ny, idx, in);
  nk_nbhd<Dual> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]];
      nb.val[q * NK_DOF + c].v = in[q] ? x : NK_R(0);
#pragma unroll
      for (int k = 0; k < NK_CH; ++k) nb.val[q * NK_DOF + c].d[k] = (k == q * NK_DOF + c) ? NK_R(1) : NK_R(0);
    }
  }
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  const nk_site s = {i, j, nx, ny};
  nk_point<Dual>(nb, )NKSRC", R"NKSRC(p, s, out);
  int rank[NK_NPTS], cnt = 0;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NK_NPTS; ++t) r += (in[t] && idx[t] < idx[q]) ? 1 : 0;
    rank[q] = r;
    cnt += in[q] ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) {
    const int base = rowptr[c * nn + node];
#if NK_GRID_DIRECT
#pragma unroll
    for (int q = 0; q < NK_NPTS; ++q) {
      if (in[q]) {
#pragma unroll
        for (int c2 = 0; c2 < NK_DOF; ++c2) vals[base + c2 * cnt + rank[q]] = out[c].d[q * NK_DOF + c2];
      }
    }
#else
    // this workgroup's piece of component c: [p0, p1) ⊂ [0, nnz), at most NK_GRID_BLOCK·npts·dof values
    const int last = node0 + NK_GRID_BLOCK < nn ? node0 + NK_GRID_BLOCK : nn;
    const int p0 = rowptr[c * nn + node0], p1 = rowptr[c * nn + last];
    if (live) {
#pragma unroll
      for (int q = 0; q < NK_NPTS; ++q) {
        if (in[q]) {
#pragma unroll
          for (int c2 = 0; c2 < NK_DOF; ++c2) sv[base - p0 + c2 * cnt + rank[q]] = out[c].d[q * NK_DOF + c2];
        }
      }
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < p1 - p0; t += NK_GRID_BLOCK) vals[p0 + t] = sv[t];
    __syncthreads();
#endif
  }
}
#endif
)NKSRC"};

static const char *k_grid_contract =
    "the contract is `template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f)` "
    "with u(di, dj, c) the component c at node (i + di, j + dj), s = {i, j, nx, ny}, p the parameters and f the node's dof "
    "residuals (nk_real = double)";

// ----------------------------------------------------------------------------- fields (programs with -DNK_NFIELDS=1..4 only)
// Read-only data on the grid: NK_NFIELDS arrays of one double per node, read through the stencil's own offsets. This text follows
// the types string (it needs NK_NPTS and the offset tables, whichever stencil they describe), and the two pieces below go between
// the pieces of k_grid_kernels_b: one more pointer after `p` in every signature, the field neighbourhood in every nk_point call.
// nk_flds_load is an argument of that call, so its loads — unconditional, from the addresses nk_grid_geom made for u — are issued
// with u's, before the source runs; val is a fully unrolled register array filled from a __restrict__ const pointer, so a load
// whose value the source never reads is dropped by the compiler. No select: outside a Dirichlet boundary idx[q] is the node
// itself, and that is the value a field has there. A program without fields gets none of this text and neither piece.
static const char *k_grid_fields = R"NKSRC(
// ---- read-only fields on the grid: field k at the stencil's points (never a dual: a constant of the differentiation)
__device__ constexpr int nk_pt_find(int di, int dj) {
  for (int q = 0; q < NK_NPTS; ++q)
    if (nk_pt_di(q) == di && nk_pt_dj(q) == dj) return q;
  return -1;
}
struct nk_flds {
  nk_real val[NK_NPTS * NK_NFIELDS];
  // field k at node (i + di, j + dj): the offsets and the shape rule of u (outside the stencil's shape: NaN). Outside a
  // Dirichlet boundary a field reads as at the node itself; at a periodic one the index wraps
  __device__ __forceinline__ nk_real operator()(int di, int dj, int k = 0) const {
    const int q = nk_pt_find(di, dj);
    if (q < 0) return NK_R(__builtin_nan(""));
    return val[q * NK_NFIELDS + k];
  }
};
__device__ __forceinline__ nk_flds nk_flds_load(const nk_real *__restrict__ a, int nn, const int (&idx)[NK_NPTS]) {
  nk_flds fl;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int k = 0; k < NK_NFIELDS; ++k) fl.val[q * NK_NFIELDS + k] = a[k * nn + idx[q]];
  }
  return fl;
}
)NKSRC";
static const char *k_grid_fields_sig = "const nk_real *__restrict__ a, ";   // after `p` in the six kernel signatures
static const char *k_grid_fields_call = "nk_flds_load(a, nn, idx), ";       // after `nb` in the six nk_point calls
// the kernels' text: the pieces of k_grid_kernels_b / k_grid3_kernels_b with, for a program with fields, the signature piece
// after every even piece and the call piece after every odd one (signature, call; three kernels)
static std::string grid_join(const char *const (&pieces)[7], bool fields) {
  std::string s;
  for (int t = 0; t < 7; ++t) {
    s += pieces[t];
    if (fields && t < 6) s += t % 2 == 0 ? k_grid_fields_sig : k_grid_fields_call;
  }
  return s;
}

static const char *k_gridf_contract =
    "the contract of a problem with fields is `template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, "
    "const nk_flds &a, const nk_real *p, nk_site s, T *f)` with u(di, dj, c) the component c at node (i + di, j + dj), "
    "a(di, dj, k) the field k there (an nk_real, never a dual), s = {i, j, nx, ny}, p the parameters and f the node's dof "
    "residuals (nk_real = double)";

// ----------------------------------------------------------------------------- device source, three dimensions
static const char *k_grid3_types = R"NKSRC(
// ---- compiled grid problems in 3-D: the node's position and its neighbourhood
#if NK_BOX
#define NK_NPTS 27
#else
#define NK_NPTS 7
#endif
struct nk_site3 { int i, j, k, nx, ny, nz; };
// stencil point q → offset; q ascends with the node index ((k·ny + j)·nx + i) of the point inside the grid:
// star (0,0,−1) (0,−1,0) (−1,0,0) C (1,0,0) (0,1,0) (0,0,1); box plane by plane, row by row (dk outermost, di innermost)
__device__ constexpr int nk_pt_di(int q) { return NK_BOX ? q % 3 - 1 : (q == 2 ? -1 : (q == 4 ? 1 : 0)); }
__device__ constexpr int nk_pt_dj(int q) { return NK_BOX ? (q / 3) % 3 - 1 : (q == 1 ? -1 : (q == 5 ? 1 : 0)); }
__device__ constexpr int nk_pt_dk(int q) { return NK_BOX ? q / 9 - 1 : (q == 0 ? -1 : (q == 6 ? 1 : 0)); }
template <typename T>
struct nk_nbhd3 {
  T val[NK_NPTS * NK_DOF];
  // component c at node (i + di, j + dj, k + dk); di, dj, dk ∈ {−1, 0, 1} (compile-time constants keep val in registers)
  __device__ __forceinline__ T operator()(int di, int dj, int dk, int c = 0) const {
#if NK_BOX
    return val[(((dk + 1) * 3 + (dj + 1)) * 3 + (di + 1)) * NK_DOF + c];
#else
    // the star has neither edges nor corners: a wrong source shows at once
    if ((di != 0) + (dj != 0) + (dk != 0) > 1) return T(NK_R(__builtin_nan("")));
    return val[(dk != 0 ? 3 + 3 * dk : (dj != 0 ? 3 + 2 * dj : 3 + di)) * NK_DOF + c];
#endif
  }
};
)NKSRC";

static const char *k_grid3_types_r2 = R"NKSRC(
// ---- compiled grid problems in 3-D, radius 2 (the 13-point star): the node's position and its neighbourhood
#define NK_NPTS 13
struct nk_site3 { int i, j, k, nx, ny, nz; };
// stencil point q → offset; q ascends with the node index ((k·ny + j)·nx + i) of the point inside the grid:
// (0,0,−2) (0,0,−1) (0,−2,0) (0,−1,0) (−2,0,0) (−1,0,0) C (1,0,0) (2,0,0) (0,1,0) (0,2,0) (0,0,1) (0,0,2)
__device__ constexpr int nk_pt_di(int q) { return q >= 4 && q <= 8 ? q - 6 : 0; }
__device__ constexpr int nk_pt_dj(int q) { return q == 2 || q == 3 ? q - 4 : (q == 9 || q == 10 ? q - 8 : 0); }
__device__ constexpr int nk_pt_dk(int q) { return q < 2 ? q - 2 : (q > 10 ? q - 10 : 0); }
template <typename T>
struct nk_nbhd3 {
  T val[NK_NPTS * NK_DOF];
  // component c at node (i + di, j + dj, k + dk); one offset ∈ {−2, …, 2}, the others 0 (compile-time constants keep val in
  // registers). A read with more than one non-zero offset returns NaN: a wrong source shows at once
  __device__ __forceinline__ T operator()(int di, int dj, int dk, int c = 0) const {
    if ((di != 0) + (dj != 0) + (dk != 0) > 1 || di < -2 || di > 2 || dj < -2 || dj > 2 || dk < -2 || dk > 2)
      return T(NK_R(__builtin_nan("")));
    return val[(dk != 0 ? (dk < 0 ? 2 + dk : 10 + dk) : (dj != 0 ? (dj < 0 ? 4 + dj : 8 + dj) : 6 + di)) * NK_DOF + c];
  }
};
)NKSRC";

static const char *k_grid3_kernels_a = R"NKSRC(
// ---- generated kernels: one node per thread
#define NK_GRID_BLOCK 256
// node index of every stencil point (clamped to the node itself outside a Dirichlet boundary, wrapped at a periodic one) and
// whether the point is in the domain
__device__ __forceinline__ void nk_grid3_geom(int i, int j, int k, int nx, int ny, int nz, int (&idx)[NK_NPTS],
                                              bool (&in)[NK_NPTS]) {
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int ii = i + nk_pt_di(q), jj = j + nk_pt_dj(q), kk = k + nk_pt_dk(q);
#if NK_PERIODIC
)NKSRC";
static const char *k_grid3_wrap_r1 = R"NKSRC(    ii = ii < 0 ? nx - 1 : (ii >= nx ? 0 : ii);
    jj = jj < 0 ? ny - 1 : (jj >= ny ? 0 : jj);
    kk = kk < 0 ? nz - 1 : (kk >= nz ? 0 : kk);
)NKSRC";
static const char *k_grid3_wrap_r2 = R"NKSRC(    ii = ii < 0 ? ii + nx : (ii >= nx ? ii - nx : ii);
    jj = jj < 0 ? jj + ny : (jj >= ny ? jj - ny : jj);
    kk = kk < 0 ? kk + nz : (kk >= nz ? kk - nz : kk);
)NKSRC";
static const char *const k_grid3_kernels_b[] = {R"NKSRC(    in[q] = true;
#else
    in[q] = ii >= 0 && ii < nx && jj >= 0 && jj < ny && kk >= 0 && kk < nz;
    ii = in[q] ? ii : i;
    jj = in[q] ? jj : j;
    kk = in[q] ? kk : k;
#endif
    idx[q] = (kk * ny + jj) * nx + ii;
  }
}
// node → (i, j, k): node = (k·ny + j)·nx + i
#define NK_GRID3_SITE(node)                                                      \
  const int k = (int)((unsigned)(node) / (unsigned)(nx * ny));                   \
  const int rem_ = (node) - k * (nx * ny);                                       \
  const int j = (int)((unsigned)rem_ / (unsigned)nx), i = rem_ - j * nx

#if NK_GRID_SET == 0
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid3_residual(int nx, int ny, int nz, const nk_real *__restrict__ p, )NKSRC", R"NKSRC(const nk_real *__restrict__ u,
                  nk_real *__restrict__ f) {
  const int nn = nx * ny * nz, node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  NK_GRID3_SITE(node);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid3_geom(i, j, k, nx, ny, nz, idx, in);
  nk_nbhd3<nk_real> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]];
      nb.val[q * NK_DOF + c] = in[q] ? x : NK_R(0);
    }
  }
  nk_real out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = NK_R(0);
  const nk_site3 s = {i, j, k, nx, ny, nz};
  nk_point<nk_real>(nb, )NKSRC", R"NKSRC(p, s, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) f[c * nn + node] = out[c];
}

// J(u)·v exactly: the value of every neighbour from u, its one partial from v
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid3_jvp(int nx, int ny, int nz, const nk_real *__restrict__ p, )NKSRC", R"NKSRC(const nk_real *__restrict__ u,
             const nk_real *__restrict__ v, nk_real *__restrict__ jv) {
  const int nn = nx * ny * nz, node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  NK_GRID3_SITE(node);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid3_geom(i, j, k, nx, ny, nz, idx, in);
  nk_nbhd3<Dual> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]], d = v[c * nn + idx[q]];
      nb.val[q * NK_DOF + c].v = in[q] ? x : NK_R(0);
      nb.val[q * NK_DOF + c].d[0] = in[q] ? d : NK_R(0);
    }
  }
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  const nk_site3 s = {i, j, k, nx, ny, nz};
  nk_point<Dual>(nb, )NKSRC", R"NKSRC(p, s, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) jv[c * nn + node] = out[c].d[0];
}
#else
// The values of J(u) on the stencil's CSR pattern (ascending columns): slot q·dof + c of the duals carries ∂/∂u_c(point q).
// Row c·nn + node holds, for c' = 0 … dof−1, its in-domain points in ascending node order: position c'·cnt + rank[q].
// NK_GRID_DIRECT = 0: the workgroup's rows of one component are one contiguous piece of the value array — they are put together
// in LDS and stored as whole lines; 1: every thread stores its own partials, 8 bytes at a stride of a row.
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
nk_grid3_jac(int nx, int ny, int nz, const nk_real *__restrict__ p, )NKSRC", R"NKSRC(const nk_real *__restrict__ u,
             const int *__restrict__ rowptr, nk_real *__restrict__ vals) {
  const int nn = nx * ny * nz, node0 = (int)blockIdx.x * NK_GRID_BLOCK, node_t = node0 + (int)threadIdx.x;
  if (node0 >= nn) return;   // (a workgroup past the grid; the launch has none)
  const bool live = node_t < nn;
#if NK_GRID_DIRECT
  if (!live) return;
#else
  __shared__ nk_real sv[NK_GRID_BLOCK * NK_NPTS * NK_DOF];   // (at most 256·28 doubles: the star at dof 4)
#endif
  const int node = live ? node_t : nn - 1;   // (past the end: the last node again, nothing of it is kept)
  NK_GRID3_SITE(node);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid3_geom(i, j, k, nx, ny, nz, idx, in);
  nk_nbhd3<Dual> nb;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = u[c * nn + idx[q]];
      nb.val[q * NK_DOF + c].v = in[q] ? x : NK_R(0);
#pragma unroll
      for (int t = 0; t < NK_CH; ++t) nb.val[q * NK_DOF + c].d[t] = (t == q * NK_DOF + c) ? NK_R(1) : NK_R(0);
    }
  }
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  const nk_site3 s = {i, j, k, nx, ny, nz};
  nk_point<Dual>(nb, )NKSRC", R"NKSRC(p, s, out);
  int rank[NK_NPTS], cnt = 0;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NK_NPTS; ++t) r += (in[t] && idx[t] < idx[q]) ? 1 : 0;
    rank[q] = r;
    cnt += in[q] ? 1 : 0;
  }
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) {
    const int base = rowptr[c * nn + node];
#if NK_GRID_DIRECT
#pragma unroll
    for (int q = 0; q < NK_NPTS; ++q) {
      if (in[q]) {
#pragma unroll
        for (int c2 = 0; c2 < NK_DOF; ++c2) vals[base + c2 * cnt + rank[q]] = out[c].d[q * NK_DOF + c2];
      }
    }
#else
    // this workgroup's piece of component c: [p0, p1) ⊂ [0, nnz), at most NK_GRID_BLOCK·npts·dof values
    const int last = node0 + NK_GRID_BLOCK < nn ? node0 + NK_GRID_BLOCK : nn;
    const int p0 = rowptr[c * nn + node0], p1 = rowptr[c * nn + last];
    if (live) {
#pragma unroll
      for (int q = 0; q < NK_NPTS; ++q) {
        if (in[q]) {
#pragma unroll
          for (int c2 = 0; c2 < NK_DOF; ++c2) sv[base - p0 + c2 * cnt + rank[q]] = out[c].d[q * NK_DOF + c2];
        }
      }
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < p1 - p0; t += NK_GRID_BLOCK) vals[p0 + t] = sv[t];
    __syncthreads();
#endif
  }
}
#endif
)NKSRC"};

static const char *k_grid3_contract =
    "the contract is `template <typename T> __device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f)` "
    "with u(di, dj, dk, c) the component c at node (i + di, j + dj, k + dk), s = {i, j, k, nx, ny, nz}, p the parameters and f "
    "the node's dof residuals (nk_real = double)";

// fields in three dimensions: the same text over the 3-D offset tables, as nk_flds3 (the two pieces are the 2-D ones)
static const char *k_grid3_fields = R"NKSRC(
// ---- read-only fields on the grid: field k at the stencil's points (never a dual: a constant of the differentiation)
__device__ constexpr int nk_pt_find(int di, int dj, int dk) {
  for (int q = 0; q < NK_NPTS; ++q)
    if (nk_pt_di(q) == di && nk_pt_dj(q) == dj && nk_pt_dk(q) == dk) return q;
  return -1;
}
struct nk_flds3 {
  nk_real val[NK_NPTS * NK_NFIELDS];
  // field k at node (i + di, j + dj, k + dk): the offsets and the shape rule of u (outside the stencil's shape: NaN). Outside
  // a Dirichlet boundary a field reads as at the node itself; at a periodic one the index wraps
  __device__ __forceinline__ nk_real operator()(int di, int dj, int dk, int k = 0) const {
    const int q = nk_pt_find(di, dj, dk);
    if (q < 0) return NK_R(__builtin_nan(""));
    return val[q * NK_NFIELDS + k];
  }
};
__device__ __forceinline__ nk_flds3 nk_flds_load(const nk_real *__restrict__ a, int nn, const int (&idx)[NK_NPTS]) {
  nk_flds3 fl;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int k = 0; k < NK_NFIELDS; ++k) fl.val[q * NK_NFIELDS + k] = a[k * nn + idx[q]];
  }
  return fl;
}
)NKSRC";
static const char *k_grid3f_contract =
    "the contract of a problem with fields is `template <typename T> __device__ void nk_point(const nk_nbhd3<T> &u, "
    "const nk_flds3 &a, const nk_real *p, nk_site3 s, T *f)` with u(di, dj, dk, c) the component c at node (i + di, j + dj, "
    "k + dk), a(di, dj, dk, k) the field k there (an nk_real, never a dual), s = {i, j, k, nx, ny, nz}, p the parameters and f "
    "the node's dof residuals (nk_real = double)";

// ----------------------------------------------------------------------------- the stencil's CSR pattern (host only)
static inline int grid_radius(int stencil) { return stencil == NK_GRID_STAR2 || stencil == NK_GRID_DIAMOND2 ? 2 : 1; }
// points of a stencil (0: the dimension does not offer it)
static inline int grid_npts(int dim, int stencil) {
  switch (stencil) {
    case NK_GRID_STAR: return dim == 3 ? 7 : 5;
    case NK_GRID_BOX: return dim == 3 ? 27 : 9;
    case NK_GRID_STAR2: return dim == 3 ? 13 : 9;
    case NK_GRID_DIAMOND2: return dim == 3 ? 0 : 13;
  }
  return 0;
}

static int grid_check_shape(int dof, int stencil, int boundary) {
  NK_REQUIRE(stencil == NK_GRID_STAR || stencil == NK_GRID_BOX || stencil == NK_GRID_STAR2 || stencil == NK_GRID_DIAMOND2,
             "stencil = %d is none of NK_GRID_STAR, NK_GRID_BOX, NK_GRID_STAR2, NK_GRID_DIAMOND2", stencil);
  NK_REQUIRE(boundary == NK_GRID_DIRICHLET0 || boundary == NK_GRID_PERIODIC,
             "boundary = %d is neither NK_GRID_DIRICHLET0 nor NK_GRID_PERIODIC", boundary);
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per grid node)", dof);
  NK_REQUIRE(stencil != NK_GRID_BOX || dof <= 2, "dof = %d with the box stencil: the 9-point box is offered for dof <= 2 "
             "(a row has at most 20 partials)", dof);
  NK_REQUIRE(stencil != NK_GRID_STAR2 || dof <= 2, "dof = %d with the star2 stencil: the 9-point radius-2 star is offered for "
             "dof <= 2 (a row has at most 20 partials)", dof);
  NK_REQUIRE(stencil != NK_GRID_DIAMOND2 || dof == 1, "dof = %d with the diamond2 stencil: the 13-point diamond is offered for "
             "dof = 1 (a row has at most 20 partials)", dof);
  return NK_OK;
}
// stencil point q → offset, in pattern order (the device tables of k_grid_types / k_grid_types_r2)
static inline int grid_pt_di(int stencil, int q) {
  if (stencil == NK_GRID_STAR2) return q >= 2 && q <= 6 ? q - 4 : 0;
  if (stencil == NK_GRID_DIAMOND2) return q == 0 || q == 12 ? 0 : (q <= 3 ? q - 2 : (q <= 8 ? q - 6 : q - 10));
  return stencil == NK_GRID_BOX ? q % 3 - 1 : (q == 1 ? -1 : (q == 3 ? 1 : 0));
}
static inline int grid_pt_dj(int stencil, int q) {
  if (stencil == NK_GRID_STAR2) return q < 2 ? q - 2 : (q > 6 ? q - 6 : 0);
  if (stencil == NK_GRID_DIAMOND2) return q == 0 ? -2 : (q <= 3 ? -1 : (q <= 8 ? 0 : (q <= 11 ? 1 : 2)));
  return stencil == NK_GRID_BOX ? q / 3 - 1 : (q == 0 ? -1 : (q == 4 ? 1 : 0));
}
// periodic wrap of an index at most n outside [0, n)
static inline int64_t grid_wrap(int64_t ii, int64_t n) { return ii < 0 ? ii + n : (ii >= n ? ii - n : ii); }

extern "C" int nk_grid_pattern(int64_t nx, int64_t ny, int dof, int stencil, int boundary, int32_t *rowptr, int32_t *colind,
                               int64_t *nnz) {
  NK_REQUIRE(rowptr || nnz, "NULL argument");
  NK_TRY(grid_check_shape(dof, stencil, boundary));
  if (grid_radius(stencil) == 2)
    NK_REQUIRE(nx >= 5 && ny >= 5, "grid %lld x %lld: a radius-2 stencil needs nx >= 5 and ny >= 5 (five distinct columns per "
               "direction at a periodic edge)", (long long)nx, (long long)ny);
  NK_REQUIRE(nx >= 3 && ny >= 3, "grid %lld x %lld: a radius-1 stencil needs nx >= 3 and ny >= 3 (three distinct columns per "
             "row at a periodic edge)", (long long)nx, (long long)ny);
  const int npts = grid_npts(2, stencil);
  NK_REQUIRE(nx <= INT32_MAX / ny && nx * ny <= (int64_t)INT32_MAX / (dof * npts * dof),
             "grid %lld x %lld with dof = %d: the pattern's 32-bit indices cannot hold it", (long long)nx, (long long)ny, dof);
  const int64_t nn = nx * ny;
  int64_t pos = 0;
  for (int c = 0; c < dof; ++c)
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        int64_t nb[13];
        int cnt = 0;
        for (int q = 0; q < npts; ++q) {
          int64_t ii = i + grid_pt_di(stencil, q), jj = j + grid_pt_dj(stencil, q);
          if (boundary == NK_GRID_PERIODIC) {
            ii = grid_wrap(ii, nx);
            jj = grid_wrap(jj, ny);
          } else if (ii < 0 || ii >= nx || jj < 0 || jj >= ny) {
            continue;
          }
          // insertion keeps the node indices ascending (wrap-around reorders the points at a periodic edge)
          const int64_t k = jj * nx + ii;
          int t = cnt++;
          while (t > 0 && nb[t - 1] > k) { nb[t] = nb[t - 1]; --t; }
          nb[t] = k;
        }
        if (rowptr) rowptr[c * nn + j * nx + i] = (int32_t)pos;
        if (colind)
          for (int c2 = 0; c2 < dof; ++c2)
            for (int t = 0; t < cnt; ++t) colind[pos + (int64_t)c2 * cnt + t] = (int32_t)(c2 * nn + nb[t]);
        pos += (int64_t)cnt * dof;
      }
  if (rowptr) rowptr[dof * nn] = (int32_t)pos;
  if (nnz) *nnz = pos;
  return NK_OK;
}

// three dimensions: the 7-point star with dof 1..4, the 27-point box with dof 1, the 13-point radius-2 star with dof 1..2 — at
// most 28 partials per row
static int grid3_check_shape(int dof, int stencil, int boundary) {
  NK_REQUIRE(stencil != NK_GRID_DIAMOND2, "stencil = NK_GRID_DIAMOND2 (%d) is not offered in three dimensions (25 points); "
             "the radius-2 stencil of nk_problem_create_grid3 is NK_GRID_STAR2", stencil);
  NK_REQUIRE(stencil == NK_GRID_STAR || stencil == NK_GRID_BOX || stencil == NK_GRID_STAR2,
             "stencil = %d is none of NK_GRID_STAR, NK_GRID_BOX, NK_GRID_STAR2", stencil);
  NK_REQUIRE(boundary == NK_GRID_DIRICHLET0 || boundary == NK_GRID_PERIODIC,
             "boundary = %d is neither NK_GRID_DIRICHLET0 nor NK_GRID_PERIODIC", boundary);
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per grid node)", dof);
  NK_REQUIRE(stencil != NK_GRID_BOX || dof == 1, "dof = %d with the box stencil: the 27-point box is offered for dof = 1 "
             "(a row has at most 28 partials)", dof);
  NK_REQUIRE(stencil != NK_GRID_STAR2 || dof <= 2, "dof = %d with the star2 stencil: the 13-point radius-2 star is offered for "
             "dof <= 2 (a row has at most 28 partials)", dof);
  return NK_OK;
}
static inline int grid3_pt_di(int stencil, int q) {
  if (stencil == NK_GRID_STAR2) return q >= 4 && q <= 8 ? q - 6 : 0;
  return stencil == NK_GRID_BOX ? q % 3 - 1 : (q == 2 ? -1 : (q == 4 ? 1 : 0));
}
static inline int grid3_pt_dj(int stencil, int q) {
  if (stencil == NK_GRID_STAR2) return q == 2 || q == 3 ? q - 4 : (q == 9 || q == 10 ? q - 8 : 0);
  return stencil == NK_GRID_BOX ? (q / 3) % 3 - 1 : (q == 1 ? -1 : (q == 5 ? 1 : 0));
}
static inline int grid3_pt_dk(int stencil, int q) {
  if (stencil == NK_GRID_STAR2) return q < 2 ? q - 2 : (q > 10 ? q - 10 : 0);
  return stencil == NK_GRID_BOX ? q / 9 - 1 : (q == 0 ? -1 : (q == 6 ? 1 : 0));
}
// the refusal of a grid too small for the stencil's radius (both boundaries: 2·radius + 1 distinct columns per direction)
static int grid3_check_size(int64_t nx, int64_t ny, int64_t nz, int stencil) {
  if (grid_radius(stencil) == 2)
    NK_REQUIRE(nx >= 5 && ny >= 5 && nz >= 5, "grid %lld x %lld x %lld: a radius-2 stencil needs nx >= 5, ny >= 5 and nz >= 5 "
               "(five distinct columns per direction at a periodic edge)", (long long)nx, (long long)ny, (long long)nz);
  NK_REQUIRE(nx >= 3 && ny >= 3 && nz >= 3, "grid %lld x %lld x %lld: a radius-1 stencil needs nx >= 3, ny >= 3 and nz >= 3 "
             "(three distinct columns per direction at a periodic edge)", (long long)nx, (long long)ny, (long long)nz);
  return NK_OK;
}

extern "C" int nk_grid3_pattern(int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int32_t *rowptr,
                                int32_t *colind, int64_t *nnz) {
  NK_REQUIRE(rowptr || nnz, "NULL argument");
  NK_TRY(grid3_check_shape(dof, stencil, boundary));
  NK_TRY(grid3_check_size(nx, ny, nz, stencil));
  const int npts = grid_npts(3, stencil);
  NK_REQUIRE(nx <= INT32_MAX / ny && nx * ny <= INT32_MAX / nz && nx * ny * nz <= (int64_t)INT32_MAX / (dof * npts * dof),
             "grid %lld x %lld x %lld with dof = %d: the pattern's 32-bit indices cannot hold it", (long long)nx, (long long)ny,
             (long long)nz, dof);
  const int64_t nn = nx * ny * nz;
  int64_t pos = 0;
  for (int c = 0; c < dof; ++c)
    for (int64_t k = 0; k < nz; ++k)
      for (int64_t j = 0; j < ny; ++j)
        for (int64_t i = 0; i < nx; ++i) {
          int64_t nb[27];
          int cnt = 0;
          for (int q = 0; q < npts; ++q) {
            int64_t ii = i + grid3_pt_di(stencil, q), jj = j + grid3_pt_dj(stencil, q), kk = k + grid3_pt_dk(stencil, q);
            if (boundary == NK_GRID_PERIODIC) {
              ii = grid_wrap(ii, nx);
              jj = grid_wrap(jj, ny);
              kk = grid_wrap(kk, nz);
            } else if (ii < 0 || ii >= nx || jj < 0 || jj >= ny || kk < 0 || kk >= nz) {
              continue;
            }
            // insertion keeps the node indices ascending (wrap-around reorders the points at a periodic edge)
            const int64_t m = (kk * ny + jj) * nx + ii;
            int t = cnt++;
            while (t > 0 && nb[t - 1] > m) { nb[t] = nb[t - 1]; --t; }
            nb[t] = m;
          }
          if (rowptr) rowptr[c * nn + (k * ny + j) * nx + i] = (int32_t)pos;
          if (colind)
            for (int c2 = 0; c2 < dof; ++c2)
              for (int t = 0; t < cnt; ++t) colind[pos + (int64_t)c2 * cnt + t] = (int32_t)(c2 * nn + nb[t]);
          pos += (int64_t)cnt * dof;
        }
  if (rowptr) rowptr[dof * nn] = (int32_t)pos;
  if (nnz) *nnz = pos;
  return NK_OK;
}

// ----------------------------------------------------------------------------- compilation
enum { GSET_F = 0 /* nk_grid_residual + nk_grid_jvp, NK_CH = 1 */, GSET_JAC = 1 /* nk_grid_jac, NK_CH = npts·dof */ };

// dim = 2: nk_grid_residual / nk_grid_jvp / nk_grid_jac; dim = 3: the nk_grid3_ kernels. The 3-D programs carry -DNK_DIM=3 (it
// tells their cache entries from the 2-D ones of the same source); the 2-D programs get the text and the options they always had.
// nf = 0: the program without fields, from the text and the options it always had; nf = 1..4: the field text after the types,
// the two field pieces in the kernels and one more option, -DNK_NFIELDS=<nf>, which also keeps the cache entries apart.
static int grid_compile(const char *source, int dim, int dof, int stencil, int boundary, int np, int nf, int gset, bool direct,
                        std::vector<char> *code, std::string *log) {
  NK_REQUIRE(source, "NULL source");
  NK_TRY(dim == 3 ? grid3_check_shape(dof, stencil, boundary) : grid_check_shape(dof, stencil, boundary));
  NK_REQUIRE(np >= 0 && np <= 32, "nparams = %d outside 0..32", np);
  NK_REQUIRE(nf >= 0 && nf <= 4, "nfields = %d outside 0..4 (read-only fields of one double per node)", nf);
  const int npts = grid_npts(dim, stencil);
  const bool r2 = grid_radius(stencil) == 2;
  const char *types = dim == 3 ? (r2 ? k_grid3_types_r2 : k_grid3_types) : (r2 ? k_grid_types_r2 : k_grid_types);
  const std::string full = std::string(nk_dual_prelude) + types + (nf > 0 ? (dim == 3 ? k_grid3_fields : k_grid_fields) : "") +
                           "\n// ---- user source\n" + source + "\n" +
                           (dim == 3 ? k_grid3_kernels_a : k_grid_kernels_a) +
                           (dim == 3 ? (r2 ? k_grid3_wrap_r2 : k_grid3_wrap_r1) : (r2 ? k_grid_wrap_r2 : k_grid_wrap_r1)) +
                           (dim == 3 ? grid_join(k_grid3_kernels_b, nf > 0) : grid_join(k_grid_kernels_b, nf > 0));
  const std::string dd = "-DNK_DOF=" + std::to_string(dof), db = std::string("-DNK_BOX=") + (stencil == NK_GRID_BOX ? "1" : "0"),
                    dp = std::string("-DNK_PERIODIC=") + (boundary == NK_GRID_PERIODIC ? "1" : "0"),
                    dc = "-DNK_CH=" + std::to_string(gset == GSET_JAC ? npts * dof : 1), ds = "-DNK_GRID_SET=" + std::to_string(gset),
                    dr = std::string("-DNK_GRID_DIRECT=") + (direct ? "1" : "0");
  std::vector<const char *> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", dd.c_str(), db.c_str(),
                                    dp.c_str(), dc.c_str(), ds.c_str(), dr.c_str()};
  if (dim == 3) opts.push_back("-DNK_DIM=3");
  // radius 2: the stencil's code, which only these programs carry (it tells star2 from diamond2 in k_grid_types_r2 and keeps
  // their cache entries apart from the radius-1 programs of the same source)
  const std::string dn = "-DNK_STENCIL=" + std::to_string(stencil);
  if (r2) opts.push_back(dn.c_str());
  const std::string df = "-DNK_NFIELDS=" + std::to_string(nf);
  if (nf > 0) opts.push_back(df.c_str());
  // the same source with the same options gives the same code object: problems created again (another grid size, another
  // context) skip the compiler
  static std::mutex mtx;
  static std::map<std::string, std::vector<char>> cache;
  std::string key;
  for (const char *o : opts) { key += o; key += ' '; }
  key += '\n';
  key += source;
  {
    std::lock_guard<std::mutex> lock(mtx);
    auto it = cache.find(key);
    if (it != cache.end()) { *code = it->second; return NK_OK; }
  }
  bool failed = false;
  NK_TRY(nk_rtc_compile(full, "nk_grid_user.hip", opts, code, log, &failed));
  if (failed)
    NK_FAIL(NK_E_INVALID, "grid residual source does not compile (%s): %.900s",
            dim == 3 ? (nf > 0 ? k_grid3f_contract : k_grid3_contract) : (nf > 0 ? k_gridf_contract : k_grid_contract),
            log && !log->empty() ? log->c_str() : "(no log)");
  std::lock_guard<std::mutex> lock(mtx);
  cache[key] = *code;
  return NK_OK;
}

// A/B switch: every thread of the Jacobian fill stores its own partials (no staging in LDS)
static bool grid_fill_direct() {   // (read at every create: tools/grid_problem_bench.py builds both forms in one process)
  const char *e = getenv("NK_GRID_FILL_DIRECT");
  return e != nullptr && atoi(e) != 0;
}

// compile only (no device needed): both programs
static int grid_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                              int64_t *code_bytes) {
  std::vector<char> code;
  std::string log;
  int64_t total = 0;
  for (int gset : {GSET_F, GSET_JAC}) {
    log.clear();
    NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, gset, grid_fill_direct(), &code, &log));
    total += (int64_t)code.size();
  }
  if (code_bytes) *code_bytes = total;
  return NK_OK;
}
extern "C" int nk_grid_compile_check(const char *source, int dof, int stencil, int boundary, int nparams, int64_t *code_bytes) {
  return grid_compile_check(source, 2, dof, stencil, boundary, nparams, 0, code_bytes);
}
extern "C" int nk_grid3_compile_check(const char *source, int dof, int stencil, int boundary, int nparams, int64_t *code_bytes) {
  return grid_compile_check(source, 3, dof, stencil, boundary, nparams, 0, code_bytes);
}
extern "C" int nk_grid_fields_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams,
                                            int nfields, int64_t *code_bytes) {
  NK_REQUIRE(dim == 2 || dim == 3, "dim = %d is neither 2 nor 3", dim);
  return grid_compile_check(source, dim, dof, stencil, boundary, nparams, nfields, code_bytes);
}

// the code object of one program (jac = 0: the residual and JVP kernels; 1: the Jacobian fill) for inspection
static int grid_code_object(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields, int jac,
                            void *buf, int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, jac != 0 ? GSET_JAC : GSET_F, grid_fill_direct(), &code,
                      &log));
  *bytes = (int64_t)code.size();
  if (!buf) return NK_OK;
  NK_REQUIRE(capacity >= *bytes, "buffer of %lld bytes, the code object has %lld", (long long)capacity, (long long)*bytes);
  memcpy(buf, code.data(), code.size());
  return NK_OK;
}
extern "C" int nk_grid_code_object(const char *source, int dof, int stencil, int boundary, int nparams, int jac, void *buf,
                                   int64_t capacity, int64_t *bytes) {
  return grid_code_object(source, 2, dof, stencil, boundary, nparams, 0, jac, buf, capacity, bytes);
}
extern "C" int nk_grid3_code_object(const char *source, int dof, int stencil, int boundary, int nparams, int jac, void *buf,
                                    int64_t capacity, int64_t *bytes) {
  return grid_code_object(source, 3, dof, stencil, boundary, nparams, 0, jac, buf, capacity, bytes);
}
extern "C" int nk_grid_fields_code_object(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                                          int jac, void *buf, int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(dim == 2 || dim == 3, "dim = %d is neither 2 nor 3", dim);
  return grid_code_object(source, dim, dof, stencil, boundary, nparams, nfields, jac, buf, capacity, bytes);
}

// ----------------------------------------------------------------------------- the problem object
struct nk_grid_state {
  nk_ctx *ctx = nullptr;
  int nx = 0, ny = 0, nz = 0 /* 0: a 2-D problem */, dof = 0, np = 0, nfields = 0;
  hipModule_t mod_f = nullptr, mod_jac = nullptr;
  hipFunction_t fn_res = nullptr, fn_jvp = nullptr, fn_jac = nullptr;
  double *d_params = nullptr;   // np doubles (at least one allocated): the source's p
  double *d_fields = nullptr;   // nfields·nn doubles, field k of node m at k·nn + m (NULL without fields); zero at creation
  nk_csr *pattern = nullptr;    // the problem's user_pattern
};

void nk_grid_state_destroy(nk_grid_state *S) {
  if (!S) return;
  if (S->mod_f) hipModuleUnload(S->mod_f);
  if (S->mod_jac) hipModuleUnload(S->mod_jac);
  hipFree(S->d_params);
  hipFree(S->d_fields);
  nk_csr_destroy(S->pattern);
  delete S;
}

// One launch of a generated kernel on `stream`. Inside a profiled scope of the context (nk_problem_residual_dev,
// nk_problem_jvp_dev and nk_problem_jac_values_dev open one around the callback) the launch carries start / stop events like
// every NK_LAUNCH, so the generated kernels are timed by the same clock as the built-in ones.
static int grid_launch(nk_grid_state *S, hipFunction_t fn, void **args, void *stream) {
  const unsigned blocks = (unsigned)(((int64_t)S->nx * S->ny * (S->nz > 0 ? S->nz : 1) + 255) / 256);
  hipEvent_t e0, e1;
  hipError_t e;
  if (S->ctx->prof.on && (hipStream_t)stream == S->ctx->stream && nk_prof_next(S->ctx, &e0, &e1))
    e = hipExtModuleLaunchKernel(fn, blocks * 256u, 1, 1, 256, 1, 1, 0, (hipStream_t)stream, args, nullptr, e0, e1, 0);   // (sizes in threads)
  else
    e = hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, (hipStream_t)stream, args, nullptr);
  return e != hipSuccess;
}

// the callbacks of the problem: launches of the generated kernels on the stream they are handed. The argument list is
// nx, ny, [nz,] p, [fields,] and the kernel's own vectors: the sizes, then what the problem owns, then `rest`
static int grid_launch_args(nk_grid_state *S, hipFunction_t fn, std::initializer_list<void *> rest, void *stream) {
  void *args[10];
  int n = 0;
  args[n++] = &S->nx;
  args[n++] = &S->ny;
  if (S->nz > 0) args[n++] = &S->nz;
  args[n++] = &S->d_params;
  if (S->nfields > 0) args[n++] = &S->d_fields;
  for (void *a : rest) args[n++] = a;
  return grid_launch(S, fn, args, stream);
}
static int grid_cb_residual(void *user, const double *u, double *f, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  return grid_launch_args(S, S->fn_res, {&u, &f}, stream);
}
static int grid_cb_jvp(void *user, const double *v, const double *u, double *jv, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  return grid_launch_args(S, S->fn_jvp, {&u, &v, &jv}, stream);
}
static int grid_cb_jac(void *user, const double *u, double *vals, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  const int32_t *rowptr = S->pattern->d_rowptr;
  return grid_launch_args(S, S->fn_jac, {&u, &rowptr, &vals}, stream);
}

int nk_grid_set_params(nk_problem *P, const double *params, int nparams) {
  nk_grid_state *S = P->grid;
  NK_REQUIRE(nparams == S->np, "nparams mismatch (%d vs %d)", nparams, S->np);
  NK_HIP(hipSetDevice(S->ctx->device));
  if (nparams > 0) NK_HIP(nk_memcpy(S->ctx, S->d_params, params, (size_t)nparams * sizeof(double), hipMemcpyHostToDevice));
  for (int i = 0; i < nparams && i < 8; ++i) P->params[i] = params[i];   // (the first eight, for inspection; the kernels read d_params)
  P->params_version++;
  nk_problem_invalidate(P);   // a Jacobian cached for the same u belongs to the old parameters
  return NK_OK;
}

// field k of a problem with fields: its nn doubles on the device
static int grid_field_ptr(nk_problem *P, int k, double **d_field, size_t *bytes) {
  NK_REQUIRE(P, "NULL argument");
  NK_REQUIRE(P->grid, "the problem is not a compiled grid problem (kind %d): it has no fields", (int)P->kind);
  nk_grid_state *S = P->grid;
  NK_REQUIRE(S->nfields > 0, "the problem was created with nfields = %d: it has no fields (nk_problem_create_grid_fields)",
             S->nfields);
  NK_REQUIRE(k >= 0 && k < S->nfields, "field k = %d outside 0..%d", k, S->nfields - 1);
  const size_t nn = (size_t)S->nx * S->ny * (S->nz > 0 ? S->nz : 1);
  *d_field = S->d_fields + (size_t)k * nn;
  *bytes = nn * sizeof(double);
  return NK_OK;
}
extern "C" int nk_problem_set_field(nk_problem *P, int k, const double *data, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(grid_field_ptr(P, k, &d, &bytes));
  NK_REQUIRE(data, "NULL data");
  NK_REQUIRE(memspace == NK_HOST || memspace == NK_DEVICE, "memspace = %d is neither NK_HOST nor NK_DEVICE", memspace);
  NK_HIP(hipSetDevice(P->grid->ctx->device));
  NK_HIP(nk_memcpy(P->grid->ctx, d, data, bytes, memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  P->params_version++;
  nk_problem_invalidate(P);   // a Jacobian cached for the same u belongs to the old field
  return NK_OK;
}
extern "C" int nk_problem_get_field(nk_problem *P, int k, double *out, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(grid_field_ptr(P, k, &d, &bytes));
  NK_REQUIRE(out, "NULL out");
  NK_REQUIRE(memspace == NK_HOST || memspace == NK_DEVICE, "memspace = %d is neither NK_HOST nor NK_DEVICE", memspace);
  NK_HIP(hipSetDevice(P->grid->ctx->device));
  NK_HIP(nk_memcpy(P->grid->ctx, out, d, bytes, memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return NK_OK;
}

// nz = 0: a 2-D problem (nk_problem_create_grid); nz > 0: a 3-D one (nk_problem_create_grid3)
static int grid_create(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary,
                       const double *params, int nparams, int nfields, nk_problem **out) {
  const int dim = nz > 0 ? 3 : 2;
  NK_REQUIRE(ctx && source && out, "NULL argument");
  NK_REQUIRE(params || nparams == 0, "NULL params with nparams = %d", nparams);
  NK_REQUIRE(nfields >= 0 && nfields <= 4, "nfields = %d outside 0..4 (read-only fields of one double per node)", nfields);
  if (ctx->nranks > 1)
    NK_FAIL(NK_E_UNSUPPORTED, "compiled grid problems run on one rank (this context has %d): no halo exchange is generated",
            ctx->nranks);
  NK_HIP(hipSetDevice(ctx->device));
  // the pattern first: it validates the geometry before anything is compiled
  int64_t nnz = 0;
  const auto pattern = [&](int32_t *rowptr, int32_t *colind) {
    return dim == 3 ? nk_grid3_pattern(nx, ny, nz, dof, stencil, boundary, rowptr, colind, &nnz)
                    : nk_grid_pattern(nx, ny, dof, stencil, boundary, rowptr, colind, &nnz);
  };
  NK_TRY(pattern(nullptr, nullptr));
  const int64_t n = nx * ny * (dim == 3 ? nz : 1) * dof;
  std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
  NK_TRY(pattern(rp.data(), ci.data()));
  std::vector<char> code_f, code_j;
  std::string log;
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, GSET_F, false, &code_f, &log));
  log.clear();
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, GSET_JAC, grid_fill_direct(), &code_j, &log));

  nk_grid_state *S = new nk_grid_state();
  auto guard = nk_make_guard(S, nk_grid_state_destroy);
  S->ctx = ctx;
  S->nx = (int)nx;
  S->ny = (int)ny;
  S->nz = dim == 3 ? (int)nz : 0;
  S->dof = dof;
  S->np = nparams;
  S->nfields = nfields;
  if (hipModuleLoadData(&S->mod_f, code_f.data()) != hipSuccess || hipModuleLoadData(&S->mod_jac, code_j.data()) != hipSuccess)
    NK_FAIL(NK_E_HIP, "hipModuleLoadData failed");
  if (hipModuleGetFunction(&S->fn_res, S->mod_f, dim == 3 ? "nk_grid3_residual" : "nk_grid_residual") != hipSuccess ||
      hipModuleGetFunction(&S->fn_jvp, S->mod_f, dim == 3 ? "nk_grid3_jvp" : "nk_grid_jvp") != hipSuccess ||
      hipModuleGetFunction(&S->fn_jac, S->mod_jac, dim == 3 ? "nk_grid3_jac" : "nk_grid_jac") != hipSuccess)
    NK_FAIL(NK_E_HIP, "a generated grid kernel is missing from the compiled module");
  NK_TRY(nk_dev_alloc(&S->d_params, (size_t)(nparams > 0 ? nparams : 1)));
  if (nparams > 0) NK_HIP(nk_memcpy(ctx, S->d_params, params, (size_t)nparams * sizeof(double), hipMemcpyHostToDevice));
  if (nfields > 0) {   // zero until nk_problem_set_field: nothing is ever read uninitialised
    const size_t cnt = (size_t)nfields * (size_t)(n / dof);
    NK_TRY(nk_dev_alloc(&S->d_fields, cnt));
    NK_HIP(nk_memset(ctx, S->d_fields, 0, cnt * sizeof(double)));
  }
  std::vector<int64_t> gc(ci.begin(), ci.end());
  NK_TRY(nk_csr_create_local(ctx, n, n, 0, rp, gc, nullptr, &S->pattern));

  nk_problem *P = new nk_problem();
  P->ctx = ctx;
  P->kind = NK_PROBLEM_USER;
  P->n_local = P->n_global = n;
  P->row_begin = 0;
  P->nparams = nparams;
  for (int i = 0; i < nparams && i < 8; ++i) P->params[i] = params[i];
  P->cb.residual = grid_cb_residual;
  P->cb.jvp = grid_cb_jvp;
  P->cb.vjp = nullptr;   // Jᵀv: user_lin_J + the transposed SpMV
  P->cb.jac_values = grid_cb_jac;
  P->user = S;
  P->user_pattern = S->pattern;
  P->grid = guard.release();
  *out = P;
  return NK_OK;
}

extern "C" int nk_problem_create_grid(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int dof, int stencil, int boundary,
                                      const double *params, int nparams, nk_problem **out) {
  return grid_create(ctx, source, nx, ny, 0, dof, stencil, boundary, params, nparams, 0, out);
}

extern "C" int nk_problem_create_grid3(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil,
                                       int boundary, const double *params, int nparams, nk_problem **out) {
  // (grid_create tells the dimensions apart by nz > 0: a side below 3 must not fall through to the 2-D path)
  if (nz < 3) NK_TRY(grid3_check_size(nx, ny, nz, stencil));
  return grid_create(ctx, source, nx, ny, nz, dof, stencil, boundary, params, nparams, 0, out);
}

// fields: nz = 0 is the 2-D problem, nz >= 3 the 3-D one; nfields = 0 gives the problem of the two entry points above
extern "C" int nk_problem_create_grid_fields(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof,
                                             int stencil, int boundary, const double *params, int nparams, int nfields,
                                             nk_problem **out) {
  if (nz != 0 && nz < 3) NK_TRY(grid3_check_size(nx, ny, nz, stencil));
  return grid_create(ctx, source, nx, ny, nz, dof, stencil, boundary, params, nparams, nfields, out);
}
