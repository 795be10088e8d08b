// Compiled grid problems: a residual given pointwise on a 2-D or 3-D grid through a stencil, handed over as HIP C++ source
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
// it treats any callback problem. Jᵀv is user_lin_J + nk_csr_spmv_t_dev. On several ranks the grid is split into slabs of its
// outermost axis and a stencil point that leaves the slab through a cut reads ghost lines ("several ranks" below).
//
// One table, one text. k_grid_stencils lists every stencil the library offers — dimension, code, name, largest dof and the
// offsets (di, dj, dk) in pattern order — and everything that depends on the stencil is derived from it: the point count, the
// radius, the smallest side, the dof limits and their messages, the host pattern, and the few lines of device text
// (grid_stencil_text: NK_NPTS and the offset table nk_pt_off) that every program starts with. The device text proper is two
// strings, k_grid_types before the user's source and k_grid_kernels after it, the same for every program; what a program is
// comes from its options alone, and every program gets all of them: -DNK_DIM=2|3, -DNK_NFIELDS=0..4, -DNK_DOF, the kinds of the
// six sides -DNK_XLO … -DNK_ZHI, -DNK_CH, -DNK_GRID_SET (0: residual and JVP, 1: the fill) and -DNK_GRID_DIRECT. The dimension decides one block of
// k_grid_types (the site, the user-facing names, the arity of operator(), the node → site split and the index geometry) and
// nothing else; in three dimensions the kernels are nk_grid3_residual / _jvp / _jac over nk_nbhd3<T> / nk_site3 =
// {i, j, k, nx, ny, nz}, and unknown c of node (i, j, k) is element c·nn + (k·ny + j)·nx + i.
//
// Where a row's partials go: the pattern has ascending columns, i.e. component-major, then ascending node index. Inside the grid
// the stencil points are numbered in that order already; at a periodic edge wrap-around reorders them, at a Dirichlet edge some
// are missing. Each thread counts, for every stencil point, the in-domain points with a smaller node index (npts² integer
// compares on registers) instead of reading a per-node slot table: the fill is bound by its 8·nnz bytes of stores, and a table
// would add npts bytes per node to the stream for something 25 (81) compares give.
//
// Sides: every side of every axis has a kind of its own (Dirichlet-0, periodic, mirror about the outermost node, mirror about
// the face half a cell outside it), compile-time constants of the program. A mirrored ghost is another unknown, so several
// points of a row can land on one node: the pattern keeps that column once, and the fill of a program with a mirror side adds
// the partials of those points, in ascending point order, into the entry of the first of them (npts² more integer compares on
// registers; the LDS piece only gets shorter). The programs of the two uniform boundaries do not contain that step.
//
// Reading the neighbourhood: u(di, dj[, dk], c) looks its offsets up in nk_pt_off (nk_pt_find, a constexpr search the compiler
// folds: the offsets are literals in the user's source) and an offset that is no point of the stencil gives NaN, so a wrong
// source shows at once. At most 20 partials per row in 2-D and 28 in 3-D (staged fill: at most 256·28 doubles of LDS, 57344
// bytes). Every side >= 2·radius + 1, so that the offsets of a direction are distinct columns on the torus.
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
// line read by three lines of threads comes from cache, as for u). In the text a field is one more kernel parameter and one more
// nk_point argument, NK_FLDS_PARAM and NK_FLDS_ARG, both empty at NK_NFIELDS == 0.
//
// Levels (nk_grid_level_create): the state keeps the two code objects, and the same problem on smaller sides — a level of the
// geometric multigrid, nk_gridmg.hip — loads them again instead of compiling: the sides are kernel arguments, and a source that
// takes its spacing from the site (s.nx, s.ny, s.nz) discretises the same PDE on every level.
#include <ctype.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- the stencils (host table)
struct grid_stencil {
  int dim, code;
  const char *name;
  int max_dof, npts;
  signed char off[27][3];   // (di, dj, dk) of point q, q ascending with the node index (k·ny + j)·nx + i inside the grid
};
static const std::vector<grid_stencil> k_grid_stencils = [] {
  std::vector<grid_stencil> t = {
      {2, NK_GRID_STAR, "star", 4, 5, {{0, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}}},
      {2, NK_GRID_STAR2, "star2", 2, 9,
       {{0, -2, 0}, {0, -1, 0}, {-2, 0, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {0, 1, 0}, {0, 2, 0}}},
      {2, NK_GRID_DIAMOND2, "diamond2", 1, 13,
       {{0, -2, 0}, {-1, -1, 0}, {0, -1, 0}, {1, -1, 0}, {-2, 0, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {-1, 1, 0},
        {0, 1, 0}, {1, 1, 0}, {0, 2, 0}}},
      {3, NK_GRID_STAR, "star", 4, 7, {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}}},
      {3, NK_GRID_STAR2, "star2", 2, 13,
       {{0, 0, -2}, {0, 0, -1}, {0, -2, 0}, {0, -1, 0}, {-2, 0, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {0, 1, 0},
        {0, 2, 0}, {0, 0, 1}, {0, 0, 2}}},
  };
  for (int dim : {2, 3}) {   // the boxes: plane by plane, row by row (dk outermost, di innermost)
    grid_stencil b = {dim, NK_GRID_BOX, "box", dim == 3 ? 1 : 2, 0, {}};
    for (int dk = (dim == 3 ? -1 : 0); dk <= (dim == 3 ? 1 : 0); ++dk)
      for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
          signed char *o = b.off[b.npts++];
          o[0] = (signed char)di, o[1] = (signed char)dj, o[2] = (signed char)dk;
        }
    t.push_back(b);
  }
  return t;
}();

static const grid_stencil *grid_find(int dim, int code) {
  for (const grid_stencil &st : k_grid_stencils)
    if (st.dim == dim && st.code == code) return &st;
  return nullptr;
}
// the largest |offset|; a side has at least 2·radius + 1 nodes
static int grid_radius(const grid_stencil &st) {
  int r = 0;
  for (int q = 0; q < st.npts; ++q)
    for (int a = 0; a < 3; ++a) r = std::max(r, abs((int)st.off[q][a]));
  return r;
}
// "NK_GRID_STAR, NK_GRID_BOX, …": the stencils of a dimension (dim = 0: of any), as the header names them
static std::string grid_stencil_names(int dim, int code = -1) {
  std::string s;
  for (const grid_stencil &st : k_grid_stencils) {
    if ((dim != 0 && st.dim != dim) || (code >= 0 && st.code != code)) continue;
    std::string nm = "NK_GRID_";
    for (const char *c = st.name; *c; ++c) nm += (char)toupper(*c);
    if (s.find(nm) == std::string::npos) s += (s.empty() ? "" : ", ") + nm;
  }
  return s;
}
// "nx x ny" or "nx x ny x nz"
static std::string grid_dims(int dim, int64_t nx, int64_t ny, int64_t nz) {
  return std::to_string(nx) + " x " + std::to_string(ny) + (dim == 3 ? " x " + std::to_string(nz) : "");
}

// ----------------------------------------------------------------------------- the boundary code
// One int everywhere: 0 and 1 are the two uniform boundaries; NK_GRID_SIDES(...) packs one kind per side, 4 bits each, under the
// marker bit NK_GRID_SIDES_BIT. grid_sides is the canonical form, and the only one anything is keyed on: the kind of side
// 2·axis + (0: lo, 1: hi). A packed code whose sides are all Dirichlet-0 (all periodic) decodes to what 0 (1) decodes to, so its
// pattern, its program options, its code objects and its problem are those of the plain code.
struct grid_sides {
  int kind[6];   // x-lo, x-hi, y-lo, y-hi, z-lo, z-hi (2-D: the z sides are Dirichlet-0 and never met, every dk is 0)
};
static const char *const k_side_names[6] = {"x-lo", "x-hi", "y-lo", "y-hi", "z-lo", "z-hi"};
static const char *const k_kind_names[4] = {"NK_GRID_DIRICHLET0", "NK_GRID_PERIODIC", "NK_GRID_MIRROR_NODE", "NK_GRID_MIRROR_FACE"};

// the one decode and validate routine of the boundary code
static int grid_decode_boundary(int dim, int boundary, grid_sides *out) {
  grid_sides sd = {};
  if (boundary == NK_GRID_DIRICHLET0 || boundary == NK_GRID_PERIODIC) {
    for (int s = 0; s < 2 * dim; ++s) sd.kind[s] = boundary;
  } else {
    NK_REQUIRE(boundary > 0 && (boundary & NK_GRID_SIDES_BIT) != 0 && (boundary >> 25) == 0,
               "boundary = %d is neither NK_GRID_DIRICHLET0, NK_GRID_PERIODIC nor a code packed by NK_GRID_SIDES", boundary);
    for (int s = 0; s < 6; ++s) {
      const int k = (boundary >> (4 * s)) & 15;
      if (s >= 2 * dim) {   // (a typo shows: the z fields of a 2-D code are not silently dropped)
        NK_REQUIRE(k == 0, "boundary side %s = %d: a 2-D grid has no z sides (leave both z kinds 0 in NK_GRID_SIDES)",
                   k_side_names[s], k);
        continue;
      }
      NK_REQUIRE(k <= NK_GRID_MIRROR_FACE, "boundary side %s = %d is an unknown kind: none of NK_GRID_DIRICHLET0 (0), "
                 "NK_GRID_PERIODIC (1), NK_GRID_MIRROR_NODE (2), NK_GRID_MIRROR_FACE (3)", k_side_names[s], k);
      sd.kind[s] = k;
    }
  }
  for (int a = 0; a < dim; ++a) {
    const int lo = sd.kind[2 * a], hi = sd.kind[2 * a + 1];
    NK_REQUIRE((lo == NK_GRID_PERIODIC) == (hi == NK_GRID_PERIODIC), "boundary of the %c axis: %s is %s and %s is %s — an axis "
               "wraps as a whole, both of its sides must be NK_GRID_PERIODIC", "xyz"[a], k_side_names[2 * a], k_kind_names[lo],
               k_side_names[2 * a + 1], k_kind_names[hi]);
  }
  *out = sd;
  return NK_OK;
}

// Where index x + (an offset of at most radius) of an axis of n nodes lands: inside, x itself; at most radius outside a side,
// by that side's kind — wrapped, mirrored about the outermost node (−k ↦ k, n−1+k ↦ n−1−k) or about the face half a cell
// outside it (−k ↦ k−1, n−1+k ↦ n−k) — or −1 outside a Dirichlet-0 side. One reflection always lands inside the grid: k <=
// radius and n >= 2·radius + 1 give 0 <= k−1 < k <= radius < n and n−1−k >= n−1−radius >= radius >= 0.
static inline int64_t grid_side_map(int64_t x, int64_t n, int lo, int hi) {
  if (x < 0) return lo == NK_GRID_PERIODIC ? x + n : (lo == NK_GRID_MIRROR_NODE ? -x : (lo == NK_GRID_MIRROR_FACE ? -x - 1 : -1));
  if (x >= n)
    return hi == NK_GRID_PERIODIC ? x - n
                                  : (hi == NK_GRID_MIRROR_NODE ? 2 * (n - 1) - x : (hi == NK_GRID_MIRROR_FACE ? 2 * n - 1 - x : -1));
  return x;
}

// what the table refuses: a stencil the dimension does not offer, a boundary that is none, a dof beyond the stencil's largest
static int grid_check_shape(int dim, int dof, int stencil, int boundary, const grid_stencil **out, grid_sides *sides) {
  const grid_stencil *st = grid_find(dim, stencil);
  if (!st) {
    const std::string elsewhere = grid_stencil_names(0, stencil), offered = grid_stencil_names(dim);
    NK_FAIL(NK_E_INVALID, "stencil = %d%s%s%s is none of %s, the stencils offered in %d dimensions", stencil,
            elsewhere.empty() ? "" : " (", elsewhere.c_str(), elsewhere.empty() ? "" : ")", offered.c_str(), dim);
  }
  NK_TRY(grid_decode_boundary(dim, boundary, sides));
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per grid node)", dof);
  int most = 0;   // partials per row the dimension's programs are built for
  for (const grid_stencil &s : k_grid_stencils)
    if (s.dim == dim) most = std::max(most, s.npts * s.max_dof);
  NK_REQUIRE(dof <= st->max_dof, "dof = %d with the %s stencil: the %d-point %s is offered for dof %s %d (a row has at most %d "
             "partials)", dof, st->name, st->npts, st->name, st->max_dof == 1 ? "=" : "<=", st->max_dof, most);
  *out = st;
  return NK_OK;
}
// what the sizes add: every side >= 2·radius + 1 (both boundaries: that many distinct columns per direction), and a pattern
// that 32-bit indices can hold
static int grid_check_size(const grid_stencil &st, int64_t nx, int64_t ny, int64_t nz, int dof) {
  const int r = grid_radius(st), side = 2 * r + 1;
  const std::string dims = grid_dims(st.dim, nx, ny, nz);
  if (st.dim == 3)
    NK_REQUIRE(nx >= side && ny >= side && nz >= side, "grid %s: a radius-%d stencil needs nx >= %d, ny >= %d and nz >= %d (%d "
               "distinct columns per direction at a periodic edge)", dims.c_str(), r, side, side, side, side);
  else
    NK_REQUIRE(nx >= side && ny >= side, "grid %s: a radius-%d stencil needs nx >= %d and ny >= %d (%d distinct columns per "
               "direction at a periodic edge)", dims.c_str(), r, side, side, side);
  NK_REQUIRE(nx <= INT32_MAX / ny && nx * ny <= INT32_MAX / nz && nx * ny * nz <= (int64_t)INT32_MAX / (dof * st.npts * dof),
             "grid %s with dof = %d: the pattern's 32-bit indices cannot hold it", dims.c_str(), dof);
  return NK_OK;
}

// ----------------------------------------------------------------------------- several ranks: slabs of the outermost axis
// On a context of R > 1 ranks the grid is split along its outermost axis (y in 2-D, z in 3-D): rank r owns the lines (planes)
// [l0, l1) = nk_partition_range(n_outer, 1, R, r), the rule of the built-in grid problems. Local numbering is component-major on
// the slab — unknown c of slab node m is c·nn_loc + m, m = (kl·ny + j)·nx + i with kl the plane within the slab — and global
// numbering is row_begin + local with row_begin = dof · (nodes of all lower slabs): one contiguous row range per rank, a
// permutation of the one-rank numbering c·nn + node. What a rank's programs are is decided by (sides, R, r) alone (grid_cut): a
// side of the outermost axis that is a cut between two ranks gets the kind NK_BC_HALO, both sides if the axis is periodic, and
// the three zones of the slab extended by its ghost lines — low neighbour's, own, high neighbour's — get their order among
// the global columns. Every slab holds at least radius + 1 lines: ghost lines then come from the adjacent ranks only, and a
// mirror at a physical side of the split axis lands inside the rank's own slab.
enum { GRID_BC_HALO = 4 };   // NK_BC_HALO of the device text
struct grid_cut {
  int lo = 0, hi = 0;          // the program's kinds of the two sides of the outermost axis
  int zord[3] = {1, 0, 2};     // [own, low, high]: the zone's place among the row's columns
  int zgrp[3] = {1, 0, 2};     // the same with the zones of one owner sharing a number
  bool any() const { return lo == GRID_BC_HALO || hi == GRID_BC_HALO; }
};
static int grid_cut_make(int dim, const grid_sides &sd, int R, int r, grid_cut *out) {
  NK_REQUIRE(R >= 1 && r >= 0 && r < R, "rank %d of %d ranks", r, R);
  grid_cut c;
  const int klo = sd.kind[2 * (dim - 1)], khi = sd.kind[2 * (dim - 1) + 1];
  const bool periodic = klo == NK_GRID_PERIODIC;
  const bool cut_lo = R > 1 && (r > 0 || periodic), cut_hi = R > 1 && (r < R - 1 || periodic);
  c.lo = cut_lo ? (int)GRID_BC_HALO : klo;
  c.hi = cut_hi ? (int)GRID_BC_HALO : khi;
  // owners: a zone that is not there sorts where it would be on an interior rank. Equal owners (two ranks, periodic): the
  // peer's first lines — my high zone — come before its last
  const int owner[3] = {r, cut_lo ? (r > 0 ? r - 1 : R - 1) : -1, cut_hi ? (r < R - 1 ? r + 1 : 0) : R};
  const int tie[3] = {0, 1, 0};
  for (int z = 0; z < 3; ++z) {
    c.zord[z] = c.zgrp[z] = 0;
    for (int y = 0; y < 3; ++y) {
      c.zord[z] += (owner[y] < owner[z] || (owner[y] == owner[z] && tie[y] < tie[z])) ? 1 : 0;
      c.zgrp[z] += owner[y] < owner[z] ? 1 : 0;
    }
  }
  *out = c;
  return NK_OK;
}

struct grid_slab {
  int R = 1, r = 0, radius = 0;
  int64_t n_outer = 0, line = 0;     // lines (planes) of the split axis; nodes per line
  std::vector<int64_t> begin;        // begin[p] … begin[p + 1]: the lines of rank p
  int64_t l0 = 0, l1 = 0;
};
static int grid_slab_make(const grid_stencil &st, int64_t nx, int64_t ny, int64_t nz, int R, int r, grid_slab *out) {
  NK_REQUIRE(R >= 1 && r >= 0 && r < R, "rank %d of %d ranks", r, R);
  grid_slab sl;
  sl.R = R;
  sl.r = r;
  sl.radius = grid_radius(st);
  sl.n_outer = st.dim == 3 ? nz : ny;
  sl.line = st.dim == 3 ? nx * ny : nx;
  sl.begin.assign((size_t)R + 1, 0);
  int64_t thinnest = sl.n_outer;
  for (int p = 0; p < R; ++p) {
    int64_t b, e;
    NK_TRY(nk_partition_range(sl.n_outer, 1, R, p, &b, &e));
    sl.begin[p] = b;
    sl.begin[p + 1] = e;
    thinnest = std::min(thinnest, e - b);
  }
  if (R > 1)
    NK_REQUIRE(thinnest >= sl.radius + 1, "n_outer = %lld %s over %d ranks: the thinnest slab has %lld, a radius-%d stencil needs "
               "at least %d in every slab (ghost lines come from the adjacent ranks only, and a mirror at a wall lands inside the "
               "rank's own slab)", (long long)sl.n_outer, st.dim == 3 ? "planes" : "lines", R, (long long)thinnest, sl.radius,
               sl.radius + 1);
  sl.l0 = sl.begin[r];
  sl.l1 = sl.begin[r + 1];
  *out = sl;
  return NK_OK;
}

// the slab's rows of the pattern, columns in the global (rank-contiguous) numbering, ascending
static int grid_slab_pattern(int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int R, int r,
                             int64_t *line_begin, int64_t *line_end, int32_t *rowptr, int64_t *colind, int64_t *nnz) {
  NK_REQUIRE(rowptr || nnz || line_begin, "NULL argument");
  NK_REQUIRE(dim == 2 || dim == 3, "dim = %d is neither 2 nor 3", dim);
  if (dim == 2) nz = 1;
  const grid_stencil *st = nullptr;
  grid_sides sd;
  NK_TRY(grid_check_shape(dim, dof, stencil, boundary, &st, &sd));
  NK_TRY(grid_check_size(*st, nx, ny, nz, dof));
  grid_slab sl;
  NK_TRY(grid_slab_make(*st, nx, ny, nz, R, r, &sl));
  if (line_begin) *line_begin = sl.l0;
  if (line_end) *line_end = sl.l1;
  const int64_t nl = sl.l1 - sl.l0, nn_loc = sl.line * nl;
  int64_t pos = 0;
  for (int c = 0; c < dof; ++c)
    for (int64_t ol = 0; ol < nl; ++ol)          // the line (plane) within the slab
      for (int64_t m = 0; m < sl.line; ++m) {    // the node within the line
        const int64_t i = m % nx, j = dim == 3 ? m / nx : sl.l0 + ol, k = dim == 3 ? sl.l0 + ol : 0;
        struct landed { int owner; int64_t w; } nb[27];
        int cnt = 0;
        for (int q = 0; q < st->npts; ++q) {
          const int64_t ii = grid_side_map(i + st->off[q][0], nx, sd.kind[0], sd.kind[1]);
          const int64_t jj = grid_side_map(j + st->off[q][1], ny, sd.kind[2], sd.kind[3]);
          const int64_t kk = grid_side_map(k + st->off[q][2], nz, sd.kind[4], sd.kind[5]);
          if (ii < 0 || jj < 0 || kk < 0) continue;
          const int64_t o = dim == 3 ? kk : jj, in_line = dim == 3 ? jj * nx + ii : ii;
          const int owner = (int)(std::upper_bound(sl.begin.begin(), sl.begin.end(), o) - sl.begin.begin()) - 1;
          const landed e = {owner, (o - sl.begin[owner]) * sl.line + in_line};
          int t = cnt;
          while (t > 0 && (nb[t - 1].owner > e.owner || (nb[t - 1].owner == e.owner && nb[t - 1].w > e.w))) --t;
          if (t > 0 && nb[t - 1].owner == e.owner && nb[t - 1].w == e.w) continue;
          for (int x = cnt++; x > t; --x) nb[x] = nb[x - 1];
          nb[t] = e;
        }
        if (rowptr) rowptr[c * nn_loc + ol * sl.line + m] = (int32_t)pos;
        if (colind) {
          int64_t at = pos;
          for (int t0 = 0; t0 < cnt;) {   // one owner after the other: component-major on the owner's slab
            int t1 = t0;
            while (t1 < cnt && nb[t1].owner == nb[t0].owner) ++t1;
            const int64_t nn_p = (sl.begin[nb[t0].owner + 1] - sl.begin[nb[t0].owner]) * sl.line;
            const int64_t rb_p = (int64_t)dof * sl.begin[nb[t0].owner] * sl.line;
            for (int c2 = 0; c2 < dof; ++c2)
              for (int t = t0; t < t1; ++t) colind[at++] = rb_p + (int64_t)c2 * nn_p + nb[t].w;
            t0 = t1;
          }
        }
        pos += (int64_t)cnt * dof;
      }
  if (rowptr) rowptr[dof * nn_loc] = (int32_t)pos;
  if (nnz) *nnz = pos;
  return NK_OK;
}
extern "C" int nk_grid_slab_pattern(int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int nranks,
                                    int rank, int64_t *line_begin, int64_t *line_end, int32_t *rowptr, int64_t *colind_global,
                                    int64_t *nnz) {
  return grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, nranks, rank, line_begin, line_end, rowptr, colind_global, nnz);
}

// ----------------------------------------------------------------------------- the stencil's CSR pattern (host only)
// The whole grid's pattern is the slab pattern of one rank of one (R = 1, r = 0): the global column of component c2 of a node is
// then c2·nn + node. The columns come back as int64 and are narrowed into the caller's 32-bit array: grid_check_size has made
// sure they fit. dim = 2: nz is 1 and every dk is 0
static int grid_pattern_narrow(int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int32_t *rowptr,
                               int32_t *colind, int64_t *nnz) {
  NK_REQUIRE(rowptr || nnz, "NULL argument");
  int64_t n = 0;
  std::vector<int64_t> wide;
  if (colind) {   // (the sizes first: every refusal comes before anything is allocated)
    NK_TRY(grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, 1, 0, nullptr, nullptr, nullptr, nullptr, &n));
    wide.resize((size_t)n);
  }
  NK_TRY(grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, 1, 0, nullptr, nullptr, rowptr, colind ? wide.data() : nullptr,
                           &n));
  for (int64_t e = 0; colind && e < n; ++e) colind[e] = (int32_t)wide[(size_t)e];
  if (nnz) *nnz = n;
  return NK_OK;
}
extern "C" int nk_grid_pattern(int64_t nx, int64_t ny, int dof, int stencil, int boundary, int32_t *rowptr, int32_t *colind,
                               int64_t *nnz) {
  return grid_pattern_narrow(2, nx, ny, 1, dof, stencil, boundary, rowptr, colind, nnz);
}
extern "C" int nk_grid3_pattern(int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int32_t *rowptr,
                                int32_t *colind, int64_t *nnz) {
  return grid_pattern_narrow(3, nx, ny, nz, dof, stencil, boundary, rowptr, colind, nnz);
}

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)
// The program is: nk_dual_prelude, the stencil's lines (grid_stencil_text), k_grid_types, k_grid_fields (every program gets it;
// it is empty at NK_NFIELDS == 0), the user's source, k_grid_kernels.
//
// the stencil's lines, generated from its row of the table: NK_NPTS and the offsets in pattern order
static std::string grid_stencil_text(const grid_stencil &st) {
  std::string s = "\n// ---- the stencil: " + std::to_string(st.dim) + "-D " + st.name + ", point q -> (di, dj, dk), q ascending " +
                  "with the node index inside the grid\n#define NK_NPTS " + std::to_string(st.npts) +
                  "\n__device__ constexpr int nk_pt_off[NK_NPTS][3] = {";
  for (int q = 0; q < st.npts; ++q)
    s += std::string(q ? ", " : "") + "{" + std::to_string(st.off[q][0]) + ", " + std::to_string(st.off[q][1]) + ", " +
         std::to_string(st.off[q][2]) + "}";
  return s + "};\n";
}

static const char *k_grid_types = R"NKSRC(
// ---- compiled grid problems: the node's position and its neighbourhood
#define NK_GRID_BLOCK 256
// the kinds of a side (the header's NK_GRID_DIRICHLET0 … NK_GRID_MIRROR_FACE); NK_XLO … NK_ZHI are the program's six
enum { NK_BC_DIRICHLET0 = 0, NK_BC_PERIODIC = 1, NK_BC_MIRROR_NODE = 2, NK_BC_MIRROR_FACE = 3, NK_BC_HALO = 4 };
#define NK_BC_IS_MIRROR(k) ((k) == 2 || (k) == 3)
// NK_BC_HALO is no kind a user can ask for: it is what a side of the outermost axis (y in 2-D, z in 3-D: NK_OLO, NK_OHI) is in
// the program of a rank whose slab ends at a cut between two ranks. A point that leaves the slab through a cut is in the domain
// and keeps its index (nk_grid_land leaves it where it is, as it does outside a Dirichlet-0 side): the index is then one on the
// slab extended by the ghost lines, negative in the low ones and >= the slab's node count in the high ones
#define NK_BC_IS_HALO(k) ((k) == 4)
#define NK_BC_STAYS(k) ((k) == NK_BC_DIRICHLET0 || (k) == NK_BC_HALO)
#if NK_DIM == 3
#define NK_OLO NK_ZLO
#define NK_OHI NK_ZHI
#else
#define NK_OLO NK_YLO
#define NK_OHI NK_YHI
#endif
#define NK_ANY_CUT (NK_BC_IS_HALO(NK_OLO) || NK_BC_IS_HALO(NK_OHI))
// a mirror side lets several stencil points of a row land on one node: only then does the fill merge partials
#define NK_ANY_MIRROR                                                                                           \
  (NK_BC_IS_MIRROR(NK_XLO) || NK_BC_IS_MIRROR(NK_XHI) || NK_BC_IS_MIRROR(NK_YLO) || NK_BC_IS_MIRROR(NK_YHI) || \
   (NK_DIM == 3 && (NK_BC_IS_MIRROR(NK_ZLO) || NK_BC_IS_MIRROR(NK_ZHI))))
// Index x (a node's own plus an offset of at most the radius) of an axis of n nodes, by the kinds of the axis's two sides.
// NK_GRID_INSIDE: false only where x is outside a Dirichlet-0 side (the test of a side of another kind is a constant the
// front end drops; no outer parentheses: with the tests of the other axes it makes one && chain, the expression the programs of
// the two uniform boundaries have always had, and they compile to the instructions they always did). nk_grid_land: x wrapped,
// mirrored about the outermost node (−k -> k, n−1+k -> n−1−k) or about the face half a cell outside it (−k -> k−1, n−1+k -> n−k);
// a Dirichlet-0 side leaves x as it is and the caller clamps to the node. n >= 2·radius + 1, so one reflection lands inside:
// 0 <= k−1 < k <= radius < n and n−1−k >= radius.
#define NK_GRID_INSIDE(LO, HI, x, n) ((LO) != NK_BC_DIRICHLET0 || (x) >= 0) && ((HI) != NK_BC_DIRICHLET0 || (x) < (n))
template <int KIND>
__device__ __forceinline__ int nk_grid_below(int x, int n) {   // x < 0
  return KIND == NK_BC_PERIODIC ? x + n : (KIND == NK_BC_MIRROR_NODE ? -x : -x - 1);
}
template <int KIND>
__device__ __forceinline__ int nk_grid_above(int x, int n) {   // x >= n
  return KIND == NK_BC_PERIODIC ? x - n : (KIND == NK_BC_MIRROR_NODE ? 2 * (n - 1) - x : 2 * n - 1 - x);
}
template <int LO, int HI>
__device__ __forceinline__ int nk_grid_land(int x, int n) {
  if constexpr (NK_BC_STAYS(LO) && NK_BC_STAYS(HI)) return x;
  else if constexpr (NK_BC_STAYS(HI)) return x < 0 ? nk_grid_below<LO>(x, n) : x;
  else if constexpr (NK_BC_STAYS(LO)) return x >= n ? nk_grid_above<HI>(x, n) : x;
  else return x < 0 ? nk_grid_below<LO>(x, n) : (x >= n ? nk_grid_above<HI>(x, n) : x);
}
// everything the dimension decides: the site, the names the user's source sees, the arity of operator(), the sizes a kernel
// takes, node -> site, and the node index of every stencil point (clamped to the node itself outside a Dirichlet-0 side of any
// axis, otherwise wrapped or mirrored axis by axis) with whether the point is in the domain
#if NK_DIM == 3
struct nk_site3 { int i, j, k, nx, ny, nz; };
#define NK_SITE nk_site3
#define NK_NBHD nk_nbhd3
#define NK_FLDS nk_flds3
#define NK_KERNEL(name) nk_grid3_##name
#define NK_OFFSET int di, int dj, int dk
#define NK_OFFSET_SLOT nk_pt_find(di, dj, dk)
#define NK_SIZES int nx, int ny, int nz
#define NK_SIZE_ARGS nx, ny, nz
#define NK_SLAB_SIZES nx, ny, sl.nl
#define NK_SLAB_SITE(s) nk_site3{s.i, s.j, s.k + sl.l0, nx, ny, nz}
__device__ __forceinline__ int nk_grid_nn(int nx, int ny, int nz) { return nx * ny * nz; }
// node = (k·ny + j)·nx + i
__device__ __forceinline__ nk_site3 nk_grid_site(int node, int nx, int ny, int nz) {
  const int k = (int)((unsigned)node / (unsigned)(nx * ny)), rem = node - k * (nx * ny);
  const int j = (int)((unsigned)rem / (unsigned)nx), i = rem - j * nx;
  return {i, j, k, nx, ny, nz};
}
__device__ __forceinline__ void nk_grid_geom(const nk_site3 s, int (&idx)[NK_NPTS], bool (&in)[NK_NPTS]) {
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int ii = s.i + nk_pt_off[q][0], jj = s.j + nk_pt_off[q][1], kk = s.k + nk_pt_off[q][2];
    in[q] = NK_GRID_INSIDE(NK_XLO, NK_XHI, ii, s.nx) && NK_GRID_INSIDE(NK_YLO, NK_YHI, jj, s.ny) &&
            NK_GRID_INSIDE(NK_ZLO, NK_ZHI, kk, s.nz);
    ii = nk_grid_land<NK_XLO, NK_XHI>(ii, s.nx);
    jj = nk_grid_land<NK_YLO, NK_YHI>(jj, s.ny);
    kk = nk_grid_land<NK_ZLO, NK_ZHI>(kk, s.nz);
    ii = in[q] ? ii : s.i;
    jj = in[q] ? jj : s.j;
    kk = in[q] ? kk : s.k;
    idx[q] = (kk * s.ny + jj) * s.nx + ii;
  }
}
#else
struct nk_site { int i, j, nx, ny; };
#define NK_SITE nk_site
#define NK_NBHD nk_nbhd
#define NK_FLDS nk_flds
#define NK_KERNEL(name) nk_grid_##name
#define NK_OFFSET int di, int dj
#define NK_OFFSET_SLOT nk_pt_find(di, dj, 0)
#define NK_SIZES int nx, int ny
#define NK_SIZE_ARGS nx, ny
#define NK_SLAB_SIZES nx, sl.nl
#define NK_SLAB_SITE(s) nk_site{s.i, s.j + sl.l0, nx, ny}
__device__ __forceinline__ int nk_grid_nn(int nx, int ny) { return nx * ny; }
// node = j·nx + i
__device__ __forceinline__ nk_site nk_grid_site(int node, int nx, int ny) {
  const int j = (int)((unsigned)node / (unsigned)nx), i = node - j * nx;
  return {i, j, nx, ny};
}
__device__ __forceinline__ void nk_grid_geom(const nk_site s, int (&idx)[NK_NPTS], bool (&in)[NK_NPTS]) {
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int ii = s.i + nk_pt_off[q][0], jj = s.j + nk_pt_off[q][1];
    in[q] = NK_GRID_INSIDE(NK_XLO, NK_XHI, ii, s.nx) && NK_GRID_INSIDE(NK_YLO, NK_YHI, jj, s.ny);
    ii = nk_grid_land<NK_XLO, NK_XHI>(ii, s.nx);
    jj = nk_grid_land<NK_YLO, NK_YHI>(jj, s.ny);
    ii = in[q] ? ii : s.i;
    jj = in[q] ? jj : s.j;
    idx[q] = jj * s.nx + ii;
  }
}
#endif

// A slab of a grid split over several ranks along the outermost axis: its lines [l0, l0 + nl) of that axis and the ghost lines
// of each cut, `radius` lines per component as the neighbour sent them (gz nodes per component). The kernels of such a
// program run on the slab — nk_grid_site and nk_grid_geom get the slab's sizes, the own vectors have the component stride
// nn = the slab's nodes — and hand the user's source the site on the whole grid (NK_SLAB_SITE). A program without a cut has
// none of this: its kernels have the parameters and the instructions they always had.
#if NK_ANY_CUT
struct nk_slab {
  int l0, nl, gz, pad;
  const nk_real *ulo, *uhi, *vlo, *vhi, *alo, *ahi;   // ghost lines of u, v and the fields below and above (NULL: no cut there)
};
#define NK_SLAB_PARAM nk_slab sl,
#define NK_SLAB_ARG , sl
#define NK_LOCAL_SIZES NK_SLAB_SIZES
#define NK_USER_SITE(s) NK_SLAB_SITE(s)
// where the slab-extended index e of point q is: 0 the own slab, 1 the low ghost lines, 2 the high ones. Only a point with an
// offset along the outermost axis can leave through a cut, so for every other point this is the constant 0
__device__ __forceinline__ int nk_slab_zone(int q, int e, int nn) {
  int z = 0;
  if (NK_BC_IS_HALO(NK_OLO) && nk_pt_off[q][NK_DIM - 1] < 0) z = e < 0 ? 1 : z;
  if (NK_BC_IS_HALO(NK_OHI) && nk_pt_off[q][NK_DIM - 1] > 0) z = e >= nn ? 2 : z;
  return z;
}
// the element of component c (of `own` with stride nn, or of a ghost buffer with stride gz): base pointer and offset are
// selected, the load itself is unconditional
__device__ __forceinline__ nk_real nk_slab_read(const nk_real *__restrict__ own, const nk_real *lo, const nk_real *hi, int c, int z,
                                                int e, int nn, int gz) {
  const nk_real *b = z == 1 ? lo : (z == 2 ? hi : own);
  const int o = z == 1 ? e + gz : (z == 2 ? e - nn : e);
  return b[c * (z == 0 ? nn : gz) + o];
}
#else
#define NK_SLAB_PARAM
#define NK_SLAB_ARG
#define NK_LOCAL_SIZES NK_SIZE_ARGS
#define NK_USER_SITE(s) s
#endif

// the stencil point with this offset, -1 if the stencil has none (the offsets are literals in the user's source: the search
// is folded at compile time)
__device__ constexpr int nk_pt_find(int di, int dj, int dk) {
  for (int q = 0; q < NK_NPTS; ++q)
    if (nk_pt_off[q][0] == di && nk_pt_off[q][1] == dj && nk_pt_off[q][2] == dk) return q;
  return -1;
}
template <typename T>
struct NK_NBHD {
  T val[NK_NPTS * NK_DOF];
  // component c at the node offset by (di, dj[, dk]) (compile-time constants keep val in registers). An offset that is no
  // point of the stencil gives NaN: a wrong source shows at once
  __device__ __forceinline__ T operator()(NK_OFFSET, int c = 0) const {
    const int q = NK_OFFSET_SLOT;
    if (q < 0) return T(NK_R(__builtin_nan("")));
    return val[q * NK_DOF + c];
  }
};
)NKSRC";

// Read-only data on the grid: NK_NFIELDS arrays of one double per node, read through the stencil's own offsets. A field is one
// more pointer after `p` in every kernel's signature (NK_FLDS_PARAM) and the field neighbourhood in every nk_point call
// (NK_FLDS_ARG). nk_flds_load is an argument of that call, so its loads — unconditional, from the addresses nk_grid_geom made for
// u — are issued with u's, before the source runs; val is a fully unrolled register array filled from a __restrict__ const
// pointer, so a load whose value the source never reads is dropped by the compiler. No select: outside a Dirichlet boundary
// idx[q] is the node itself, and that is the value a field has there.
static const char *k_grid_fields = R"NKSRC(
#if NK_NFIELDS > 0
// ---- read-only fields on the grid: field k at the stencil's points (never a dual: a constant of the differentiation)
struct NK_FLDS {
  nk_real val[NK_NPTS * NK_NFIELDS];
  // field k at the node offset by (di, dj[, dk]): the offsets and the shape rule of u (no point of the stencil: NaN). Outside a
  // Dirichlet boundary a field reads as at the node itself; at a periodic one the index wraps
  __device__ __forceinline__ nk_real operator()(NK_OFFSET, int k = 0) const {
    const int q = NK_OFFSET_SLOT;
    if (q < 0) return NK_R(__builtin_nan(""));
    return val[q * NK_NFIELDS + k];
  }
};
#if NK_ANY_CUT
// through a cut a field reads the neighbour's value, from the ghost lines exchanged when the field was set
__device__ __forceinline__ NK_FLDS nk_flds_load(const nk_real *__restrict__ a, int nn, const int (&idx)[NK_NPTS], const nk_slab &sl) {
  NK_FLDS fl;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    const int z = nk_slab_zone(q, idx[q], nn);
#pragma unroll
    for (int k = 0; k < NK_NFIELDS; ++k) fl.val[q * NK_NFIELDS + k] = nk_slab_read(a, sl.alo, sl.ahi, k, z, idx[q], nn, sl.gz);
  }
  return fl;
}
#else
__device__ __forceinline__ NK_FLDS nk_flds_load(const nk_real *__restrict__ a, int nn, const int (&idx)[NK_NPTS]) {
  NK_FLDS fl;
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int k = 0; k < NK_NFIELDS; ++k) fl.val[q * NK_NFIELDS + k] = a[k * nn + idx[q]];
  }
  return fl;
}
#endif
#define NK_FLDS_PARAM const nk_real *__restrict__ a,
#define NK_FLDS_ARG nk_flds_load(a, nn, idx NK_SLAB_ARG),
#else
#define NK_FLDS_PARAM
#define NK_FLDS_ARG
#endif
)NKSRC";

static const char *k_grid_kernels = R"NKSRC(
// ---- generated kernels: one node per thread
// The neighbourhood of a node: component c of point q from u[c·nn + idx[q]], every load unconditional, zero outside a
// Dirichlet boundary. The partials of a dual: none to set (NK_SEED_NONE, T = nk_real), its one partial from v (NK_SEED_V),
// or the unit seed of slot q·dof + c (NK_SEED_UNIT)
enum { NK_SEED_NONE, NK_SEED_V, NK_SEED_UNIT };
#if NK_ANY_CUT
#define NK_SLAB_LOAD_PARAM , const nk_slab &sl
#define NK_READ_U(c, q) nk_slab_read(u, sl.ulo, sl.uhi, c, z, idx[q], nn, sl.gz)
#define NK_READ_V(c, q) nk_slab_read(v, sl.vlo, sl.vhi, c, z, idx[q], nn, sl.gz)
#else
#define NK_SLAB_LOAD_PARAM
#define NK_READ_U(c, q) u[c * nn + idx[q]]
#define NK_READ_V(c, q) v[c * nn + idx[q]]
#endif
__device__ __forceinline__ nk_real &nk_value(nk_real &x) { return x; }
__device__ __forceinline__ nk_real &nk_value(Dual &x) { return x.v; }
template <int SEED, typename T>
__device__ __forceinline__ void nk_grid_load(NK_NBHD<T> &nb, const nk_real *__restrict__ u, const nk_real *__restrict__ v,
                                             int nn, const int (&idx)[NK_NPTS], const bool (&in)[NK_NPTS] NK_SLAB_LOAD_PARAM) {
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#if NK_ANY_CUT
    const int z = nk_slab_zone(q, idx[q], nn);
#endif
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
      const nk_real x = NK_READ_U(c, q);
      nk_value(nb.val[q * NK_DOF + c]) = in[q] ? x : NK_R(0);
      if constexpr (SEED == NK_SEED_V) {
        const nk_real d = NK_READ_V(c, q);
        nb.val[q * NK_DOF + c].d[0] = in[q] ? d : NK_R(0);
      }
      if constexpr (SEED == NK_SEED_UNIT) {
#pragma unroll
        for (int t = 0; t < NK_CH; ++t) nb.val[q * NK_DOF + c].d[t] = (t == q * NK_DOF + c) ? NK_R(1) : NK_R(0);
      }
    }
  }
}

#if NK_GRID_SET == 0
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
NK_KERNEL(residual)(NK_SIZES, NK_SLAB_PARAM const nk_real *__restrict__ p, NK_FLDS_PARAM const nk_real *__restrict__ u,
                    nk_real *__restrict__ f) {
  const int nn = nk_grid_nn(NK_LOCAL_SIZES), node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  const NK_SITE s = nk_grid_site(node, NK_LOCAL_SIZES);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(s, idx, in);
  NK_NBHD<nk_real> nb;
  nk_grid_load<NK_SEED_NONE>(nb, u, nullptr, nn, idx, in NK_SLAB_ARG);
  nk_real out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = NK_R(0);
  nk_point<nk_real>(nb, NK_FLDS_ARG p, NK_USER_SITE(s), out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) f[c * nn + node] = out[c];
}

// J(u)·v exactly: the value of every neighbour from u, its one partial from v
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
NK_KERNEL(jvp)(NK_SIZES, NK_SLAB_PARAM const nk_real *__restrict__ p, NK_FLDS_PARAM const nk_real *__restrict__ u,
               const nk_real *__restrict__ v, nk_real *__restrict__ jv) {
  const int nn = nk_grid_nn(NK_LOCAL_SIZES), node = (int)blockIdx.x * NK_GRID_BLOCK + (int)threadIdx.x;
  if (node >= nn) return;
  const NK_SITE s = nk_grid_site(node, NK_LOCAL_SIZES);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(s, idx, in);
  NK_NBHD<Dual> nb;
  nk_grid_load<NK_SEED_V>(nb, u, v, nn, idx, in NK_SLAB_ARG);
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  nk_point<Dual>(nb, NK_FLDS_ARG p, NK_USER_SITE(s), out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) jv[c * nn + node] = out[c].d[0];
}
#else
// The values of J(u) on the stencil's CSR pattern (ascending columns): slot q·dof + c of the duals carries ∂/∂u_c(point q).
// Row c·nn + node holds, for c' = 0 … dof−1, its in-domain points in ascending node order: position c'·cnt + rank[q].
// NK_GRID_DIRECT = 0: the workgroup's rows of one component are one contiguous piece of the value array — they are put together
// in LDS and stored as whole lines (k_bratu_jac's way); 1: every thread stores its own partials, 8 bytes at a stride of a row.
extern "C" __global__ void __launch_bounds__(NK_GRID_BLOCK)
NK_KERNEL(jac)(NK_SIZES, NK_SLAB_PARAM const nk_real *__restrict__ p, NK_FLDS_PARAM const nk_real *__restrict__ u,
               const int *__restrict__ rowptr, nk_real *__restrict__ vals) {
  const int nn = nk_grid_nn(NK_LOCAL_SIZES), node0 = (int)blockIdx.x * NK_GRID_BLOCK, node_t = node0 + (int)threadIdx.x;
  if (node0 >= nn) return;   // (a workgroup past the grid; the launch has none)
  const bool live = node_t < nn;
#if NK_GRID_DIRECT
  if (!live) return;
#else
  __shared__ nk_real sv[NK_GRID_BLOCK * NK_NPTS * NK_DOF];   // (at most 256·28 doubles: the 3-D star at dof 4)
#endif
  const int node = live ? node_t : nn - 1;   // (past the end: the last node again, nothing of it is kept)
  const NK_SITE s = nk_grid_site(node, NK_LOCAL_SIZES);
  int idx[NK_NPTS];
  bool in[NK_NPTS];
  nk_grid_geom(s, idx, in);
  NK_NBHD<Dual> nb;
  nk_grid_load<NK_SEED_UNIT>(nb, u, nullptr, nn, idx, in NK_SLAB_ARG);
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  nk_point<Dual>(nb, NK_FLDS_ARG p, NK_USER_SITE(s), out);
  int rank[NK_NPTS], cnt = 0;
#if NK_ANY_CUT
  // Columns ascend in the global numbering, which is (owner rank, component, node within the owner's slab): the three zones
  // of the extended slab — the low neighbour's lines, the own slab, the high neighbour's — come in an order that is a constant
  // of the rank (NK_ZORD_*: under periodic wrap rank 0's low zone sorts after its slab, the last rank's high zone before its
  // own). key = ordinal of the zone · 2^29 + the offset within the zone orders and identifies the landed nodes (a grid has fewer
  // than 2^29 nodes: INT32_MAX / 5 at most), so everything below that compared idx compares key instead
  int key[NK_NPTS];
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    const int z = nk_slab_zone(q, idx[q], nn);
    key[q] = z == 1 ? (NK_ZORD_LO << 29) + idx[q] + sl.gz : (z == 2 ? (NK_ZORD_HI << 29) + idx[q] - nn : (NK_ZORD_OWN << 29) + idx[q]);
  }
#else
  const int (&key)[NK_NPTS] = idx;
#endif
#if NK_ANY_MIRROR
  // Several points of a row may land on one node. The first of them (smallest q) is the primary: it alone has a column, and its
  // value is the sum of the partials of all of them, added in ascending q. cnt and rank count primaries only
  bool prim[NK_NPTS];
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    bool first = in[q];
#pragma unroll
    for (int t = 0; t < q; ++t) first = first && !(in[t] && key[t] == key[q]);
    prim[q] = first;
  }
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NK_NPTS; ++t) r += (prim[t] && key[t] < key[q]) ? 1 : 0;
    rank[q] = r;
    cnt += prim[q] ? 1 : 0;
  }
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
#pragma unroll
    for (int t = q + 1; t < NK_NPTS; ++t) {
      const bool same = in[t] && key[t] == key[q];   // (only a primary's sum is stored; another q's is dropped with it)
#pragma unroll
      for (int c = 0; c < NK_DOF; ++c) {
#pragma unroll
        for (int c2 = 0; c2 < NK_DOF; ++c2) {
          const nk_real x = out[c].d[q * NK_DOF + c2];
          out[c].d[q * NK_DOF + c2] = same ? x + out[c].d[t * NK_DOF + c2] : x;
        }
      }
    }
  }
#define NK_FILL_KEEP(q) prim[q]
#else
#pragma unroll
  for (int q = 0; q < NK_NPTS; ++q) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NK_NPTS; ++t) r += (in[t] && key[t] < key[q]) ? 1 : 0;
    rank[q] = r;
    cnt += in[q] ? 1 : 0;
  }
#define NK_FILL_KEEP(q) in[q]
#endif
#if NK_ANY_CUT
  // Where a zone's columns start and how many each component has there. Zones of one owner form one group (NK_ZGRP_*: with two
  // ranks and a periodic axis both ghost zones are the one peer's, its first lines — the high zone — before its last): a row is
  // (group, component, node), so an entry sits at dof · (columns of earlier groups) + c' · (columns of its group) + its rank
  // within the group, and that rank is rank[q] less the columns of earlier groups, because key orders the groups too
  int slot[NK_NPTS], same[NK_NPTS];
  {
    int nz[3] = {0, 0, 0};   // columns per zone: own, low, high
#pragma unroll
    for (int q = 0; q < NK_NPTS; ++q) {
      const int z = nk_slab_zone(q, idx[q], nn);
#pragma unroll
      for (int y = 0; y < 3; ++y) nz[y] += (NK_FILL_KEEP(q) && z == y) ? 1 : 0;
    }
    constexpr int grp[3] = {NK_ZGRP_OWN, NK_ZGRP_LO, NK_ZGRP_HI};
    int before[3], with[3];
#pragma unroll
    for (int z = 0; z < 3; ++z) {
      before[z] = with[z] = 0;
#pragma unroll
      for (int y = 0; y < 3; ++y) {
        before[z] += grp[y] < grp[z] ? nz[y] : 0;
        with[z] += grp[y] == grp[z] ? nz[y] : 0;
      }
    }
#pragma unroll
    for (int q = 0; q < NK_NPTS; ++q) {
      const int z = nk_slab_zone(q, idx[q], nn);
      const int b = z == 1 ? before[1] : (z == 2 ? before[2] : before[0]);
      same[q] = z == 1 ? with[1] : (z == 2 ? with[2] : with[0]);
      slot[q] = NK_DOF * b + rank[q] - b;
    }
  }
#define NK_FILL_AT(q, c2) ((c2) * same[q] + slot[q])
#else
#define NK_FILL_AT(q, c2) ((c2) * cnt + rank[q])
#endif
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) {
    const int base = rowptr[c * nn + node];
#if NK_GRID_DIRECT
#pragma unroll
    for (int q = 0; q < NK_NPTS; ++q) {
      if (NK_FILL_KEEP(q)) {
#pragma unroll
        for (int c2 = 0; c2 < NK_DOF; ++c2) vals[base + NK_FILL_AT(q, c2)] = out[c].d[q * NK_DOF + c2];
      }
    }
#else
    // this workgroup's piece of component c: [p0, p1) ⊂ [0, nnz), at most NK_GRID_BLOCK·npts·dof values
    const int last = node0 + NK_GRID_BLOCK < nn ? node0 + NK_GRID_BLOCK : nn;
    const int p0 = rowptr[c * nn + node0], p1 = rowptr[c * nn + last];
    if (live) {
#pragma unroll
      for (int q = 0; q < NK_NPTS; ++q) {
        if (NK_FILL_KEEP(q)) {
#pragma unroll
          for (int c2 = 0; c2 < NK_DOF; ++c2) sv[base - p0 + NK_FILL_AT(q, c2)] = out[c].d[q * NK_DOF + c2];
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
)NKSRC";

// what the user's source is held to, for the message of a source that does not compile
static std::string grid_contract(int dim, int nfields) {
  const bool d3 = dim == 3;
  const std::string off = d3 ? "di, dj, dk" : "di, dj", flds = d3 ? "nk_flds3" : "nk_flds";
  return std::string(nfields > 0 ? "the contract of a problem with fields is" : "the contract is") +
         " `template <typename T> __device__ void nk_point(const " + (d3 ? "nk_nbhd3" : "nk_nbhd") + "<T> &u, " +
         (nfields > 0 ? "const " + flds + " &a, " : "") + "const nk_real *p, " + (d3 ? "nk_site3" : "nk_site") +
         " s, T *f)` with u(" + off + ", c) the component c at node " + (d3 ? "(i + di, j + dj, k + dk)" : "(i + di, j + dj)") +
         (nfields > 0 ? ", a(" + off + ", k) the field k there (an nk_real, never a dual)" : "") + ", s = " +
         (d3 ? "{i, j, k, nx, ny, nz}" : "{i, j, nx, ny}") + ", p the parameters and f the node's dof residuals (nk_real = double)";
}

// ----------------------------------------------------------------------------- compilation
enum { GSET_F = 0 /* nk_grid_residual + nk_grid_jvp, NK_CH = 1 */, GSET_JAC = 1 /* nk_grid_jac, NK_CH = npts·dof */ };

// One program: its text is the same for every stencil but the stencil's lines, and all of what else it is comes from its
// options, which every program gets in full (dim = 2: nk_grid_residual / nk_grid_jvp / nk_grid_jac; 3: the nk_grid3_ kernels)
static int grid_compile(const char *source, int dim, int dof, int stencil, int boundary, int np, int nf, int gset, bool direct,
                        std::vector<char> *code, std::string *log, int nranks = 1, int rank = 0) {
  NK_REQUIRE(source, "NULL source");
  const grid_stencil *st = nullptr;
  grid_sides sd;
  NK_TRY(grid_check_shape(dim, dof, stencil, boundary, &st, &sd));
  NK_REQUIRE(np >= 0 && np <= 32, "nparams = %d outside 0..32", np);
  NK_REQUIRE(nf >= 0 && nf <= 4, "nfields = %d outside 0..4 (read-only fields of one double per node)", nf);
  // several ranks: the two sides of the outermost axis are the rank's own, and a program with a cut gets the zone order too
  // (a program without one gets the options it always got)
  grid_cut cut;
  NK_TRY(grid_cut_make(dim, sd, nranks, rank, &cut));
  sd.kind[2 * (dim - 1)] = cut.lo;
  sd.kind[2 * (dim - 1) + 1] = cut.hi;
  const std::string stencil_text = grid_stencil_text(*st);
  const std::string full = std::string(nk_dual_prelude) + stencil_text + k_grid_types + k_grid_fields + "\n// ---- user source\n" +
                           source + "\n" + k_grid_kernels;
  std::vector<std::string> defs = {"-DNK_DIM=" + std::to_string(dim), "-DNK_NFIELDS=" + std::to_string(nf),
                                   "-DNK_DOF=" + std::to_string(dof),
                                   "-DNK_XLO=" + std::to_string(sd.kind[0]), "-DNK_XHI=" + std::to_string(sd.kind[1]),
                                   "-DNK_YLO=" + std::to_string(sd.kind[2]), "-DNK_YHI=" + std::to_string(sd.kind[3]),
                                   "-DNK_ZLO=" + std::to_string(sd.kind[4]), "-DNK_ZHI=" + std::to_string(sd.kind[5]),
                                   "-DNK_CH=" + std::to_string(gset == GSET_JAC ? st->npts * dof : 1),
                                   "-DNK_GRID_SET=" + std::to_string(gset), std::string("-DNK_GRID_DIRECT=") + (direct ? "1" : "0")};
  if (cut.any()) {
    const char *const zn[3] = {"OWN", "LO", "HI"};
    for (int z = 0; z < 3; ++z) {
      defs.push_back(std::string("-DNK_ZORD_") + zn[z] + "=" + std::to_string(cut.zord[z]));
      defs.push_back(std::string("-DNK_ZGRP_") + zn[z] + "=" + std::to_string(cut.zgrp[z]));
    }
  }
  // what varies between two grid programs beside the options: the stencil's lines and the user's source (the rest of the text is
  // the same for all)
  return nk_rtc_program(full, "nk_grid_user.hip", defs, stencil_text + source, "grid", grid_contract(dim, nf).c_str(), code, log);
}

// A/B switch: every thread of the Jacobian fill stores its own partials (no staging in LDS)
static bool grid_fill_direct() {   // (read at every create: tools/grid_problem_bench.py builds both forms in one process)
  const char *e = getenv("NK_GRID_FILL_DIRECT");
  return e != nullptr && atoi(e) != 0;
}

// compile only (no device needed): both programs
static int grid_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                              int64_t *code_bytes, int nranks = 1, int rank = 0) {
  std::vector<char> code;
  std::string log;
  int64_t total = 0;
  for (int gset : {GSET_F, GSET_JAC}) {
    log.clear();
    NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, gset, grid_fill_direct(), &code, &log, nranks, rank));
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
                            void *buf, int64_t capacity, int64_t *bytes, int nranks = 1, int rank = 0) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, jac != 0 ? GSET_JAC : GSET_F, grid_fill_direct(), &code,
                      &log, nranks, rank));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
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

// the programs of rank `rank` of `nranks`: (nranks, rank) decide which sides of the outermost axis are cuts and the zone order;
// nranks = 1 gives the programs of the calls above
extern "C" int nk_grid_slab_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                                          int nranks, int rank, int64_t *code_bytes) {
  NK_REQUIRE(dim == 2 || dim == 3, "dim = %d is neither 2 nor 3", dim);
  return grid_compile_check(source, dim, dof, stencil, boundary, nparams, nfields, code_bytes, nranks, rank);
}
extern "C" int nk_grid_slab_code_object(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                                        int nranks, int rank, int jac, void *buf, int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(dim == 2 || dim == 3, "dim = %d is neither 2 nor 3", dim);
  return grid_code_object(source, dim, dof, stencil, boundary, nparams, nfields, jac, buf, capacity, bytes, nranks, rank);
}

// ----------------------------------------------------------------------------- the problem object
// the device text's nk_slab, member for member: one kernel argument of a program with a cut
struct grid_slab_arg {
  int l0 = 0, nl = 0, gz = 0, pad = 0;
  const double *ulo = nullptr, *uhi = nullptr, *vlo = nullptr, *vhi = nullptr, *alo = nullptr, *ahi = nullptr;
};
struct nk_grid_state {
  nk_compiled c;   // the context, the programs, p and the pattern
  int nx = 0, ny = 0, nz = 0 /* 0: a 2-D problem */, dof = 0, nfields = 0;
  int stencil = 0, boundary = 0;   // as the problem was created (nk_grid_level_create builds the same problem on a smaller grid)
  std::vector<char> code_f, code_j;   // the two code objects, kept by a problem made from source: a level of the geometric multigrid
                                      // loads them again (nothing is compiled twice) and keeps no copy of its own
  double *d_fields = nullptr;   // nfields·nn doubles, field k of node m at k·nn + m (NULL without fields); zero at creation
  // several ranks (nranks > 1; on one rank the slab is the grid and none of the rest is used)
  int64_t l0 = 0, l1 = 0, nn_loc = 0;   // the slab's lines (planes) of the outermost axis and its nodes
  bool cut = false, cut_lo = false, cut_hi = false;
  int below = -1, above = -1;           // the ranks the ghost lines come from
  int64_t ghost = 0;                    // ghost nodes per component and cut: radius lines
  grid_slab_arg slab;                   // what the kernels of a program with a cut are handed
  nk_halo halo_u, halo_v, halo_a;       // ghost lines of u, of v (the JVP reads both: two receive areas) and of the fields
  hipEvent_t ev = nullptr;              // orders an exchange against a stream that is not the context's
};

void nk_grid_state_destroy(nk_grid_state *S) {
  if (!S) return;
  nk_compiled_free(&S->c);
  hipFree(S->d_fields);
  nk_halo_free(&S->halo_u);
  nk_halo_free(&S->halo_v);
  nk_halo_free(&S->halo_a);
  if (S->ev) hipEventDestroy(S->ev);
  delete S;
}

// the callbacks of the problem: launches of the generated kernels on the stream they are handed, one thread per node of the slab
// (one rank: the slab is the grid). The argument list is nx, ny, [nz,] [the slab,] p, [fields,] and the kernel's own vectors:
// the sizes, then what the problem owns, then `rest`
static int grid_launch_args(nk_grid_state *S, hipFunction_t fn, std::initializer_list<void *> rest, void *stream) {
  void *args[11];
  int n = 0;
  args[n++] = &S->nx;
  args[n++] = &S->ny;
  if (S->nz > 0) args[n++] = &S->nz;
  if (S->cut) args[n++] = &S->slab;
  args[n++] = &S->c.d_params;
  if (S->nfields > 0) args[n++] = &S->d_fields;
  for (void *a : rest) args[n++] = a;
  return nk_compiled_launch(&S->c, fn, S->nn_loc, args, stream);
}
// Where the low and the high ghost lines of a plan are in its receive area, after an exchange (the peer transport alternates
// between two areas). The layout rule of the built-in grid problems: a peer's block is [what serves as my low ghost][what
// serves as my high ghost], so with two ranks and a periodic axis, where the one peer is both, the high lines come second
static void grid_ghost_ptrs(const nk_grid_state *S, const nk_halo &H, int ncomp, const double **lo, const double **hi) {
  *lo = S->cut_lo ? H.d_recv + H.recv_off[S->below] : nullptr;
  *hi = S->cut_hi ? H.d_recv + H.recv_off[S->above] + (S->cut_lo && S->above == S->below ? S->ghost * ncomp : 0) : nullptr;
}
// The exchanges of a callback run on the context's stream (nk_halo_exchange: both transports, counted in stats.halo_exchanges).
// Every caller in the library hands that stream; another one is ordered against it with an event on both sides
static int grid_stream_order(nk_grid_state *S, hipStream_t from, hipStream_t to) {
  if (from == to) return NK_OK;
  if (!S->ev) NK_HIP(hipEventCreateWithFlags(&S->ev, hipEventDisableTiming));
  NK_HIP(hipEventRecord(S->ev, from));
  NK_HIP(hipStreamWaitEvent(to, S->ev, 0));
  return NK_OK;
}
// what a callback reads across the cuts, exchanged before its launch: u, and v for the JVP
static int grid_exchange(nk_grid_state *S, const double *u, const double *v, void *stream) {
  if (!S->cut) return NK_OK;
  nk_ctx *ctx = S->c.ctx;
  NK_TRY(grid_stream_order(S, (hipStream_t)stream, ctx->stream));
  NK_TRY(nk_halo_exchange(ctx, &S->halo_u, u));
  grid_ghost_ptrs(S, S->halo_u, S->dof, &S->slab.ulo, &S->slab.uhi);
  if (v) {
    NK_TRY(nk_halo_exchange(ctx, &S->halo_v, v));
    grid_ghost_ptrs(S, S->halo_v, S->dof, &S->slab.vlo, &S->slab.vhi);
  }
  return grid_stream_order(S, ctx->stream, (hipStream_t)stream);
}
static int grid_cb_residual(void *user, const double *u, double *f, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  if (grid_exchange(S, u, nullptr, stream) != NK_OK) return 1;
  return grid_launch_args(S, S->c.fn_res, {&u, &f}, stream);
}
static int grid_cb_jvp(void *user, const double *v, const double *u, double *jv, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  if (grid_exchange(S, u, v, stream) != NK_OK) return 1;
  return grid_launch_args(S, S->c.fn_jvp, {&u, &v, &jv}, stream);
}
static int grid_cb_jac(void *user, const double *u, double *vals, void *stream) {
  nk_grid_state *S = (nk_grid_state *)user;
  if (grid_exchange(S, u, nullptr, stream) != NK_OK) return 1;
  const int32_t *rowptr = S->c.pattern->d_rowptr;
  return grid_launch_args(S, S->c.fn_jac, {&u, &rowptr, &vals}, stream);
}

// field k of a problem with fields: its doubles on the device, one per node of the rank's slab (one rank: of the grid)
static int grid_field_ptr(nk_problem *P, int k, double **d_field, size_t *bytes) {
  NK_REQUIRE(P, "NULL argument");
  NK_REQUIRE(P->grid, "the problem is not a compiled grid problem (kind %d): it has no fields", (int)P->kind);
  nk_grid_state *S = P->grid;
  NK_REQUIRE(S->nfields > 0, "the problem was created with nfields = %d: it has no fields (nk_problem_create_grid_fields)",
             S->nfields);
  NK_REQUIRE(k >= 0 && k < S->nfields, "field k = %d outside 0..%d", k, S->nfields - 1);
  const size_t nn = (size_t)S->nn_loc;
  *d_field = S->d_fields + (size_t)k * nn;
  *bytes = nn * sizeof(double);
  return NK_OK;
}
static int grid_exchange_fields(nk_grid_state *S) {
  if (!S->cut || S->nfields == 0) return NK_OK;
  NK_TRY(nk_halo_exchange(S->c.ctx, &S->halo_a, S->d_fields));
  grid_ghost_ptrs(S, S->halo_a, S->nfields, &S->slab.alo, &S->slab.ahi);
  return NK_OK;
}
extern "C" int nk_problem_set_field(nk_problem *P, int k, const double *data, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(grid_field_ptr(P, k, &d, &bytes));
  NK_TRY(nk_compiled_data_copy(P, d, bytes, data, memspace, true));
  NK_TRY(grid_exchange_fields(P->grid));   // several ranks: the ghost lines of the fields, once, here (collective)
  nk_compiled_data_changed(P);
  return NK_OK;
}
extern "C" int nk_problem_get_field(nk_problem *P, int k, double *out, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(grid_field_ptr(P, k, &d, &bytes));
  return nk_compiled_data_copy(P, d, bytes, out, memspace, false);
}

// Several ranks: the halo plans of a slab. The last `radius` lines (planes) of every component go up, the first `radius` down
// — to the rank above they are its low ghost lines, to the rank below its high ones — component-major, radius·line nodes per
// component. A peer is sent first what serves as its low ghost, then what serves as its high one (two ranks, periodic: both).
// One plan per vector a launch reads (nk_halo has one receive area) and one over all fields; the fields' ghost lines are
// exchanged here once, so that they are the zeros of the fields themselves.
static int grid_setup_halos(nk_grid_state *S, int dim, int stencil, int boundary) {
  nk_ctx *ctx = S->c.ctx;
  const int R = ctx->nranks, r = ctx->rank;
  const grid_stencil *st = grid_find(dim, stencil);
  grid_sides sd;
  NK_TRY(grid_decode_boundary(dim, boundary, &sd));
  grid_cut cut;
  NK_TRY(grid_cut_make(dim, sd, R, r, &cut));
  const int radius = grid_radius(*st);
  const int64_t nl = S->l1 - S->l0, line = S->nn_loc / nl;
  S->cut_lo = cut.lo == GRID_BC_HALO;
  S->cut_hi = cut.hi == GRID_BC_HALO;
  S->cut = cut.any();
  S->below = S->cut_lo ? (r > 0 ? r - 1 : R - 1) : -1;
  S->above = S->cut_hi ? (r < R - 1 ? r + 1 : 0) : -1;
  S->ghost = radius * line;
  S->slab.l0 = (int)S->l0;
  S->slab.nl = (int)nl;
  S->slab.gz = (int)S->ghost;
  auto plan = [&](int ncomp, nk_halo *H) {
    std::vector<std::vector<int32_t>> send((size_t)R);
    std::vector<int64_t> recv((size_t)R, 0);
    auto push_lines = [&](std::vector<int32_t> &v, int64_t first) {   // `radius` lines from line `first` of the slab on
      for (int c = 0; c < ncomp; ++c)
        for (int64_t m = 0; m < S->ghost; ++m) v.push_back((int32_t)(c * S->nn_loc + first * line + m));
    };
    if (S->above >= 0) push_lines(send[S->above], nl - radius);
    if (S->below >= 0) push_lines(send[S->below], 0);
    if (S->below >= 0) recv[S->below] += S->ghost * ncomp;
    if (S->above >= 0) recv[S->above] += S->ghost * ncomp;
    return nk_halo_setup(ctx, H, send, recv);
  };
  NK_TRY(plan(S->dof, &S->halo_u));
  NK_TRY(plan(S->dof, &S->halo_v));
  if (S->nfields > 0) {
    NK_TRY(plan(S->nfields, &S->halo_a));
    NK_TRY(nk_halo_exchange(ctx, &S->halo_a, S->d_fields));
    grid_ghost_ptrs(S, S->halo_a, S->nfields, &S->slab.alo, &S->slab.ahi);
  }
  return NK_OK;
}

extern "C" int nk_problem_grid_slab(nk_problem *P, int64_t *line_begin, int64_t *line_end) {
  NK_REQUIRE(P && line_begin && line_end, "NULL argument");
  NK_REQUIRE(P->grid, "the problem is not a compiled grid problem (kind %d)", (int)P->kind);
  *line_begin = P->grid->l0;
  *line_end = P->grid->l1;
  return NK_OK;
}

// The problem object from its pattern and its two code objects. params: nparams host doubles, or NULL for a parameter buffer
// the caller fills on the device (nk_grid_level_create). nnz, l0, l1: the pattern's count and the slab's lines if the caller has them
// (its validating pass), nnz = −1 if not. keep_code: the state keeps the code objects (a problem made from source; a level reads its
// fine problem's)
static int grid_assemble(nk_ctx *ctx, int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary,
                         const double *params, int nparams, int nfields, const std::vector<char> &code_f,
                         const std::vector<char> &code_j, int64_t nnz, int64_t l0, int64_t l1, bool keep_code, nk_problem **out) {
  const int R = ctx->nranks, r = ctx->rank;
  // on one rank the slab is the grid, its pattern nk_grid_pattern's and its programs the ones without a cut
  if (nnz < 0) NK_TRY(grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, R, r, &l0, &l1, nullptr, nullptr, &nnz));
  const int64_t line = dim == 3 ? nx * ny : nx, nn_loc = line * (l1 - l0);
  const int64_t n = nn_loc * dof, n_global = nx * ny * nz * dof;
  std::vector<int32_t> rp((size_t)n + 1);
  std::vector<int64_t> gc((size_t)nnz);
  NK_TRY(grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, R, r, &l0, &l1, rp.data(), gc.data(), &nnz));

  nk_grid_state *S = new nk_grid_state();
  auto guard = nk_make_guard(S, nk_grid_state_destroy);
  S->c.ctx = ctx;
  S->nx = (int)nx;
  S->ny = (int)ny;
  S->nz = dim == 3 ? (int)nz : 0;
  S->dof = dof;
  S->nfields = nfields;
  S->stencil = stencil;
  S->boundary = boundary;
  if (keep_code) {
    S->code_f = code_f;
    S->code_j = code_j;
  }
  S->l0 = l0;
  S->l1 = l1;
  S->nn_loc = nn_loc;
  if (dim == 3)
    NK_TRY(nk_compiled_load(&S->c, code_f, code_j, "nk_grid3_residual", "nk_grid3_jvp", "nk_grid3_jac", "grid"));
  else
    NK_TRY(nk_compiled_load(&S->c, code_f, code_j, "nk_grid_residual", "nk_grid_jvp", "nk_grid_jac", "grid"));
  NK_TRY(nk_compiled_params_init(&S->c, params, nparams));
  // zero until nk_problem_set_field: nothing is ever read uninitialised
  if (nfields > 0) NK_TRY(nk_compiled_zeros(ctx, &S->d_fields, (size_t)nfields * (size_t)nn_loc));
  if (R > 1) NK_TRY(grid_setup_halos(S, dim, stencil, boundary));   // (collective, like the pattern's own plan below)
  NK_TRY(nk_csr_create_local(ctx, n, n_global, dof * line * l0, rp, gc, nullptr, &S->c.pattern));
  NK_TRY(nk_compiled_problem(&S->c, n, n_global, dof * line * l0, params, nparams,
                             {grid_cb_residual, grid_cb_jvp, nullptr, grid_cb_jac}, S, out));
  (*out)->grid = guard.release();
  return NK_OK;
}

// dim = 2: nz is not read (nk_problem_create_grid); dim = 3: nk_problem_create_grid3
static int grid_create(nk_ctx *ctx, const char *source, int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil,
                       int boundary, const double *params, int nparams, int nfields, nk_problem **out) {
  NK_REQUIRE(ctx && source && out, "NULL argument");
  NK_REQUIRE(params || nparams == 0, "NULL params with nparams = %d", nparams);
  NK_REQUIRE(nfields >= 0 && nfields <= 4, "nfields = %d outside 0..4 (read-only fields of one double per node)", nfields);
  NK_HIP(hipSetDevice(ctx->device));
  if (dim == 2) nz = 1;
  const int R = ctx->nranks, r = ctx->rank;
  // the pattern first: it validates the geometry (several ranks: and the slabs) before anything is compiled
  int64_t nnz = 0, l0 = 0, l1 = 0;
  NK_TRY(grid_slab_pattern(dim, nx, ny, nz, dof, stencil, boundary, R, r, &l0, &l1, nullptr, nullptr, &nnz));
  std::vector<char> code_f, code_j;
  std::string log;
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, GSET_F, false, &code_f, &log, R, r));
  log.clear();
  NK_TRY(grid_compile(source, dim, dof, stencil, boundary, nparams, nfields, GSET_JAC, grid_fill_direct(), &code_j, &log, R, r));
  return grid_assemble(ctx, dim, nx, ny, nz, dof, stencil, boundary, params, nparams, nfields, code_f, code_j, nnz, l0, l1, true, out);
}

// ----------------------------------------------------------------------------- what the geometric multigrid asks (nk_gridmg.hip)
int64_t nk_grid_side_map(int64_t x, int64_t n, int lo, int hi) { return grid_side_map(x, n, lo, hi); }

int nk_grid_shape(const nk_problem *P, nk_grid_shape_info *out) {
  NK_REQUIRE(P && P->grid && out, "the problem is not a compiled grid problem");
  const nk_grid_state *S = P->grid;
  const int dim = S->nz > 0 ? 3 : 2;
  grid_sides sd;
  NK_TRY(grid_decode_boundary(dim, S->boundary, &sd));
  out->dim = dim;
  out->n[0] = S->nx, out->n[1] = S->ny, out->n[2] = dim == 3 ? S->nz : 1;
  out->dof = S->dof;
  out->nfields = S->nfields;
  out->radius = grid_radius(*grid_find(dim, S->stencil));
  for (int s = 0; s < 6; ++s) out->kind[s] = sd.kind[s];
  out->d_fields = S->d_fields;
  return NK_OK;
}

// The problem of `fine` on an nx × ny [× nz] grid: same source, options and parameter count, the fine problem's code objects
// loaded again (the sizes are kernel arguments). One rank. Its p is a device copy of the fine problem's, its fields are zero.
int nk_grid_level_create(nk_problem *fine, int64_t nx, int64_t ny, int64_t nz, nk_problem **out) {
  NK_REQUIRE(fine && fine->grid && out, "the problem is not a compiled grid problem");
  nk_grid_state *F = fine->grid;
  NK_REQUIRE(!F->code_f.empty() && !F->code_j.empty(), "a level is built from a problem made from source, not from another level");
  NK_REQUIRE(F->c.ctx->nranks == 1, "a level of a compiled grid problem is built on one rank, the context has %d", F->c.ctx->nranks);
  NK_HIP(hipSetDevice(F->c.ctx->device));
  const int dim = F->nz > 0 ? 3 : 2;
  NK_TRY(grid_assemble(F->c.ctx, dim, nx, ny, dim == 3 ? nz : 1, F->dof, F->stencil, F->boundary, nullptr, F->c.np, F->nfields, F->code_f,
                       F->code_j, -1, 0, 0, false, out));
  const int st = nk_grid_level_sync_params(fine, *out);
  if (st != NK_OK) { nk_problem_destroy(*out); *out = nullptr; }
  return st;
}
// p of the fine problem, as it is now, into a level's
int nk_grid_level_sync_params(nk_problem *fine, nk_problem *level) {
  nk_grid_state *F = fine->grid, *S = level->grid;
  if (F->c.np > 0) NK_HIP(hipMemcpyAsync(S->c.d_params, F->c.d_params, (size_t)F->c.np * sizeof(double), hipMemcpyDeviceToDevice, F->c.ctx->stream));
  for (int i = 0; i < 8; ++i) level->params[i] = fine->params[i];
  nk_problem_invalidate(level);
  return NK_OK;
}

extern "C" int nk_problem_create_grid(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int dof, int stencil, int boundary,
                                      const double *params, int nparams, nk_problem **out) {
  return grid_create(ctx, source, 2, nx, ny, 1, dof, stencil, boundary, params, nparams, 0, out);
}

extern "C" int nk_problem_create_grid3(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil,
                                       int boundary, const double *params, int nparams, nk_problem **out) {
  return grid_create(ctx, source, 3, nx, ny, nz, dof, stencil, boundary, params, nparams, 0, out);
}

// fields: nz = 0 is the 2-D problem, any other nz the 3-D one with that many planes (so nz = 1 or 2 is refused as a 3-D grid
// too small, not taken for a 2-D one); nfields = 0 gives the problem of the two entry points above
extern "C" int nk_problem_create_grid_fields(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof,
                                             int stencil, int boundary, const double *params, int nparams, int nfields,
                                             nk_problem **out) {
  return grid_create(ctx, source, nz != 0 ? 3 : 2, nx, ny, nz, dof, stencil, boundary, params, nparams, nfields, out);
}
