// Compiled element problems: a finite-element / finite-volume residual given element by element on any mesh, handed over as
// HIP C++ source
//     template <typename T> __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f);
// and compiled at run time (hiprtc, gfx950) — the third compiled kind beside grids (nk_grid.hip) and graphs (nk_graph.hip). In
// the reference this is the ordinary assembly loop inside `f` with jac_prototype = the mesh's sparsity. An element reads the
// unknowns and the data of its NK_NPE nodes, does its quadrature ONCE and contributes to the residuals of all its nodes.
//
//   nk_elem_residual   T = nk_real                              one element per thread            → B
//   nk_elem_jvp        T = Dual, NK_CH = 1: value u, partial v  one element per thread            → B
//   nk_elem_jac        T = Dual, NK_CH = dof, unit seeds        one (element, local node b) pair  → M
//   k_elem_gather      (not generated) one output per thread: the sum of a list of buffer entries in ascending element order
//
// Layout. L = npe·dof numbers per element. The device copy of the connectivity is node-major, node a of element e at a·ne + e,
// so a wavefront's index loads are consecutive. B holds L streams of ne doubles, number (a, c) of element e at (a·dof + c)·ne + e;
// M holds L² streams, dF_{a,c}/du_{b,c2} of element e at ((a·dof + c)·L + b·dof + c2)·ne + e. Every store of a generated kernel
// is therefore one coalesced stream per register. Node datum k of node i is element k·nn + i, element datum k of element e
// element k·ne + e of two buffers the problem owns (zero at creation).
//
// The gather. Two nodes are adjacent when they share an element; the Jacobian's CSR is the graph pattern of that adjacency
// (nk_graph_pattern's slots and value layout). Built on the host at creation:
//   the row list of node i          one int32 per (element, a) with conn[e, a] = i:  a·dof·ne + e, elements ascending
//   the entry list of slot (i, j)   one int32 per (element, a, b) with conn[e, a] = i and conn[e, b] = j:
//                                   (a·dof·L + b·dof)·ne + e, elements ascending
// The component offsets are arithmetic (c·ne; (c·L + c2)·ne), so the lists are not multiplied by the components. One thread
// walks one list per component (pair) and adds in list order: no atomics, a fixed order, bit-reproducible. A node in 300
// elements is walked by one thread — correct, not fast (the stance nk_graph.hip takes for a hub).
//
// Fixed unknowns (nk_problem_set_elem_fixed): a mask and values of dof·nn entries, component-major. The gather writes
// F_r = u_r − g_r, (Jv)_r = v_r and the unit row (1 on the diagonal, 0 on the row's other structural entries) for a fixed row
// r; columns of fixed unknowns stay in the free rows, so J is nonsymmetric.
//
// Blocks (nk_problem_create_element_blocks). A mesh of up to 8 blocks, each with its own conn, npe, source and element data; nn,
// dof, p, the node data, the mask, the pattern and the outputs are shared. With TB = Σ npe_k·ne_k, TM = Σ npe_k²·ne_k and
// base_k, mbase_k the same sums over the blocks before k, the buffers of a problem of several blocks are component-major:
//   B   number (a, c) of element e of block k at        c·TB + base_k + a·ne_k + e
//   M   dF_{a,c}/du_{b,c2} of element e of block k at   (c·dof + c2)·TM + mbase_k + (a·npe_k + b)·ne_k + e
// so the component offset does not depend on the block and k_elem_gather runs unchanged with ne := TB (the fill: L := dof,
// ne := TM): its offsets c·ne and (c·L + c2)·ne are these strides. The list entries are base_k + a·ne_k + e and
// mbase_k + (a·npe_k + b)·ne_k + e, the lists walk block 0's elements ascending, then block 1's, …: the summation order. A
// callback is one generated launch per block (the kernels' block form, -DNK_ELEM_BLOCKS=1) and ONE gather. One block with
// npe >= 2 keeps the plain layout above: the same programs, buffers and launches as nk_problem_create_elements.
//
// The result is an NK_PROBLEM_USER problem with user_pattern set, exactly as nk_problem_create_graph builds one. One rank.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- the mesh (host only)
// A mesh is 1..8 blocks over one set of nodes; a plain problem (nk_problem_create_elements) is one block. `named`: the block
// entry points, whose messages name the block and which allow npe = 1 (a point element)
struct elem_mesh {
  int64_t nn;
  int nblocks;
  const int64_t *ne;
  const int *npe;
  const int32_t *const *conn;
  bool named;
};

static int elem_check_dof(int dof) {
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per node)", dof);
  return NK_OK;
}
static int elem_check_shape(int npe, int dof) {
  NK_REQUIRE(npe >= 2 && npe <= 8, "npe = %d outside 2..8 (nodes per element)", npe);
  NK_TRY(elem_check_dof(dof));
  NK_REQUIRE(npe * dof <= 16, "npe·dof = %d·%d = %d exceeds 16 (the numbers one element contributes)", npe, dof, npe * dof);
  return NK_OK;
}
static int elem_check_block_shape(int k, int npe, int dof) {
  NK_REQUIRE(npe >= 1 && npe <= 8, "block %d: npe = %d outside 1..8 (nodes per element; 1 is a point element)", k, npe);
  NK_REQUIRE(npe * dof <= 16, "block %d: npe·dof = %d·%d = %d exceeds 16 (the numbers one element contributes)", k, npe, dof,
             npe * dof);
  return NK_OK;
}

// every rule of the header, the first offending element (and its block) named
static int elem_validate(const elem_mesh &m, int dof) {
  if (m.named) {
    NK_REQUIRE(m.nblocks >= 1 && m.nblocks <= 8, "nblocks = %d outside 1..8 (element blocks of one mesh)", m.nblocks);
    NK_REQUIRE(m.ne && m.npe && m.conn, "NULL argument");
    NK_TRY(elem_check_dof(dof));
    for (int k = 0; k < m.nblocks; ++k) NK_TRY(elem_check_block_shape(k, m.npe[k], dof));
  } else {
    NK_TRY(elem_check_shape(m.npe[0], dof));
  }
  NK_REQUIRE(m.nn >= 1 && m.nn <= INT32_MAX, "nn = %lld: a mesh has 1..INT32_MAX nodes", (long long)m.nn);
  int64_t room = (int64_t)INT32_MAX / (dof * dof);   // for Σ npe²·ne
  for (int k = 0; k < m.nblocks; ++k) {
    const int64_t ne = m.ne[k], sq = (int64_t)m.npe[k] * m.npe[k];
    if (!m.named) {
      NK_REQUIRE(ne >= 1, "ne = %lld: a mesh has at least one element", (long long)ne);
      NK_REQUIRE(ne <= room / sq, "%lld elements with npe = %d, dof = %d: ne·(npe·dof)² exceeds INT32_MAX, the element-matrix "
                 "buffer's 32-bit indices cannot hold it", (long long)ne, m.npe[k], dof);
    } else {
      NK_REQUIRE(ne >= 1, "block %d: ne = %lld: a block has at least one element", k, (long long)ne);
      NK_REQUIRE(ne <= room / sq, "block %d: %lld elements with npe = %d, dof = %d: dof²·Σ npe²·ne over the blocks so far exceeds "
                 "INT32_MAX, the element-matrix buffer's 32-bit indices cannot hold it", k, (long long)ne, m.npe[k], dof);
    }
    room -= ne * sq;
  }
  for (int k = 0; k < m.nblocks; ++k) {
    char where[24] = "";
    if (m.named) snprintf(where, sizeof where, "block %d, ", k);
    const int32_t *conn = m.conn[k];
    const int npe = m.npe[k];
    NK_REQUIRE(conn, "%sNULL conn", m.named ? where : "");
    for (int64_t e = 0; e < m.ne[k]; ++e)
      for (int a = 0; a < npe; ++a) {
        const int64_t j = conn[e * npe + a];
        NK_REQUIRE(j >= 0 && j < m.nn, "%selement %lld: node %lld (local node %d) outside 0..%lld", where, (long long)e,
                   (long long)j, a, (long long)m.nn - 1);
        for (int b = 0; b < a; ++b)
          NK_REQUIRE(conn[e * npe + b] != j, "%selement %lld: node %lld twice (local nodes %d and %d) — the nodes of one element "
                     "are distinct", where, (long long)e, (long long)j, b, a);
      }
  }
  return NK_OK;
}

// the node graph of a validated mesh: i and j adjacent when an element of any block holds both; ascending columns, no self-loops
static int elem_adjacency_build(const elem_mesh &m, std::vector<int32_t> *rp, std::vector<int32_t> *ci) {
  const int64_t nn = m.nn;
  std::vector<int64_t> at((size_t)nn + 1, 0);
  for (int k = 0; k < m.nblocks; ++k)
    for (int64_t q = 0; q < m.ne[k] * m.npe[k]; ++q) at[(size_t)m.conn[k][q] + 1] += m.npe[k] - 1;
  for (int64_t i = 0; i < nn; ++i) at[(size_t)i + 1] += at[(size_t)i];
  std::vector<int32_t> all((size_t)at[(size_t)nn]);
  std::vector<int64_t> fill(at.begin(), at.end() - 1);
  for (int k = 0; k < m.nblocks; ++k) {
    const int32_t *conn = m.conn[k];
    const int npe = m.npe[k];
    for (int64_t e = 0; e < m.ne[k]; ++e)
      for (int a = 0; a < npe; ++a)
        for (int b = 0; b < npe; ++b)
          if (b != a) all[(size_t)fill[(size_t)conn[e * npe + a]]++] = conn[e * npe + b];
  }
  rp->assign((size_t)nn + 1, 0);
  int64_t total = 0;
  for (int64_t i = 0; i < nn; ++i) {
    int32_t *b = all.data() + at[(size_t)i], *e = all.data() + at[(size_t)i + 1];
    std::sort(b, e);
    const int64_t cnt = std::unique(b, e) - b;
    // (compacted in place: the rows before i have already shrunk, so `total` never passes at[i])
    std::copy(b, b + cnt, all.data() + total);
    total += cnt;
    NK_REQUIRE(total <= INT32_MAX, "the node graph of the mesh has more than INT32_MAX edges");
    (*rp)[(size_t)i + 1] = (int32_t)total;
  }
  all.resize((size_t)total);
  ci->swap(all);
  return NK_OK;
}

static int elem_adjacency_out(const elem_mesh &m, int32_t *rowptr, int32_t *colind, int64_t *nedges) {
  NK_REQUIRE(rowptr || nedges, "NULL argument");
  NK_TRY(elem_validate(m, 1));
  std::vector<int32_t> rp, ci;
  NK_TRY(elem_adjacency_build(m, &rp, &ci));
  if (rowptr) memcpy(rowptr, rp.data(), rp.size() * sizeof(int32_t));
  if (colind && !ci.empty()) memcpy(colind, ci.data(), ci.size() * sizeof(int32_t));
  if (nedges) *nedges = (int64_t)ci.size();
  return NK_OK;
}
// the Jacobian's CSR: nk_graph_pattern of the node graph (its slot numbering, its value layout, its int32 limit)
static int elem_pattern_out(const elem_mesh &m, int dof, int32_t *jrowptr, int32_t *jcolind, int64_t *nnz) {
  NK_REQUIRE(jrowptr || nnz, "NULL argument");
  NK_TRY(elem_validate(m, dof));
  std::vector<int32_t> rp, ci;
  NK_TRY(elem_adjacency_build(m, &rp, &ci));
  return nk_graph_pattern(m.nn, rp.data(), ci.data(), dof, jrowptr, jcolind, nnz);
}

extern "C" int nk_elem_adjacency(int64_t nn, int64_t ne, int npe, const int32_t *conn, int32_t *rowptr, int32_t *colind,
                                 int64_t *nedges) {
  return elem_adjacency_out(elem_mesh{nn, 1, &ne, &npe, &conn, false}, rowptr, colind, nedges);
}
extern "C" int nk_elem_pattern(int64_t nn, int64_t ne, int npe, const int32_t *conn, int dof, int32_t *jrowptr, int32_t *jcolind,
                               int64_t *nnz) {
  return elem_pattern_out(elem_mesh{nn, 1, &ne, &npe, &conn, false}, dof, jrowptr, jcolind, nnz);
}
extern "C" int nk_elem_blocks_adjacency(int64_t nn, int nblocks, const int64_t *ne, const int *npe, const int32_t *const *conn,
                                        int32_t *rowptr, int32_t *colind, int64_t *nedges) {
  return elem_adjacency_out(elem_mesh{nn, nblocks, ne, npe, conn, true}, rowptr, colind, nedges);
}
extern "C" int nk_elem_blocks_pattern(int64_t nn, int nblocks, const int64_t *ne, const int *npe, const int32_t *const *conn, int dof,
                                      int32_t *jrowptr, int32_t *jcolind, int64_t *nnz) {
  return elem_pattern_out(elem_mesh{nn, nblocks, ne, npe, conn, true}, dof, jrowptr, jcolind, nnz);
}

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)
// The program is: nk_dual_prelude, nk_seed_lift, k_elem_types, the user's source, k_elem_kernels. What a program is comes from
// its options: -DNK_NPE, -DNK_DOF, -DNK_NNODE, -DNK_NELEM (the data arrays per node and per element), -DNK_CH and -DNK_ELEM_SET =
// -DNK_SEED_SET (0: residual and JVP, 1: the fill), -DNK_BLOCK (the block the source belongs to; 0 in a plain problem) and, for
// the blocks of a problem of several, -DNK_ELEM_BLOCKS=1: the kernels take the block's base and the total stride as two further
// arguments and store in the block layout (the top of the file). Without it the compiler sees the text of a plain problem.
static const char *k_elem_types = R"NKSRC(
// ---- compiled element problems: the element and its nodes
#define NK_ELEM_BLOCK 256
struct nk_cell { int e, ne, nn; };
// What the source sees of element e. Unknowns are T, data are nk_real (constants of the differentiation). A local node a
// outside 0..NK_NPE-1, a component outside 0..NK_DOF-1 and a datum k outside the declared count read NaN (node(a): -1): a wrong
// source shows at once and reads nothing it does not own
template <typename T>
struct nk_elemv {
  const nk_real *__restrict__ nk_u;
  const nk_real *__restrict__ nk_v;
  const int *__restrict__ nk_conn;     // node-major, already at the element: local node a at nk_conn[a·ne]
  const nk_real *__restrict__ nk_nd;   // datum k of node j: nk_nd[k·nn + j]
  const nk_real *__restrict__ nk_ed;   // already at the element: datum k at nk_ed[k·ne]
  int nk_nn, nk_ne, nk_hot;            // nk_hot: the local node that carries the unit seeds (the fill), else -1
  __device__ __forceinline__ int node(int a) const { return (unsigned)a < (unsigned)NK_NPE ? nk_conn[(long)a * nk_ne] : -1; }
  __device__ __forceinline__ T at(int a, int c = 0) const {
    if ((unsigned)a >= (unsigned)NK_NPE || (unsigned)c >= (unsigned)NK_DOF) return T(NK_R(__builtin_nan("")));
    const int el = c * nk_nn + nk_conn[(long)a * nk_ne];
    return nk_lift<T>::at(nk_u[el], nk_v, el, c, nk_hot == a);
  }
  __device__ __forceinline__ nk_real x(int a, int k = 0) const {
    if ((unsigned)a >= (unsigned)NK_NPE || (unsigned)k >= (unsigned)NK_NNODE) return NK_R(__builtin_nan(""));
    return nk_nd[(long)k * nk_nn + nk_conn[(long)a * nk_ne]];
  }
  __device__ __forceinline__ nk_real w(int k = 0) const {
    if ((unsigned)k >= (unsigned)NK_NELEM) return NK_R(__builtin_nan(""));
    return nk_ed[(long)k * nk_ne];
  }
};
)NKSRC";

static const char *k_elem_kernels = R"NKSRC(
// ---- generated kernels
#define NK_EL (NK_NPE * NK_DOF)
// the mesh as every kernel gets it: nn, ne, the node-major connectivity, then p, the node data and the element data
#define NK_ELEM_PARAMS int nn, int ne, const int *__restrict__ conn, const nk_real *__restrict__ p, \
                       const nk_real *__restrict__ nd, const nk_real *__restrict__ ed
// where number q = a·NK_DOF + c of element e goes in B, and dF_q/du_(b,c2) in M: still one coalesced stream per register
#ifdef NK_ELEM_BLOCKS
#define NK_ELEM_OUT , int base, int stride
#define NK_ELEM_B_AT(q) ((q) % NK_DOF) * stride + base + ((q) / NK_DOF) * ne + e
#define NK_ELEM_M_AT(q, b, c2) (((q) % NK_DOF) * NK_DOF + (c2)) * stride + base + (((q) / NK_DOF) * NK_NPE + (b)) * ne + e
#else
#define NK_ELEM_OUT
#define NK_ELEM_B_AT(q) (q) * ne + e
#define NK_ELEM_M_AT(q, b, c2) ((q) * NK_EL + (b) * NK_DOF + (c2)) * ne + e
#endif
template <typename T>
__device__ __forceinline__ nk_elemv<T> nk_elem_view(int nn, int ne, const int *__restrict__ conn, const nk_real *__restrict__ nd,
                                                    const nk_real *__restrict__ ed, const nk_real *__restrict__ u,
                                                    const nk_real *__restrict__ v, int e, int hot) {
  nk_elemv<T> w;
  w.nk_u = u, w.nk_v = v, w.nk_conn = conn + e, w.nk_nd = nd, w.nk_ed = ed + e;
  w.nk_nn = nn, w.nk_ne = ne, w.nk_hot = hot;
  return w;
}

#if NK_ELEM_SET == 0
extern "C" __global__ void __launch_bounds__(NK_ELEM_BLOCK)
nk_elem_residual(NK_ELEM_PARAMS, const nk_real *__restrict__ u, nk_real *__restrict__ B NK_ELEM_OUT) {
  const int e = (int)blockIdx.x * NK_ELEM_BLOCK + (int)threadIdx.x;
  if (e >= ne) return;
  const nk_elemv<nk_real> w = nk_elem_view<nk_real>(nn, ne, conn, nd, ed, u, nullptr, e, -1);
  nk_real out[NK_EL];
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) out[q] = NK_R(0);
  nk_element<nk_real>(w, p, nk_cell{e, ne, nn}, out);
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) B[NK_ELEM_B_AT(q)] = out[q];
}

// the element's share of J(u)·v exactly: the value of every unknown from u, its one partial from v
extern "C" __global__ void __launch_bounds__(NK_ELEM_BLOCK)
nk_elem_jvp(NK_ELEM_PARAMS, const nk_real *__restrict__ u, const nk_real *__restrict__ v, nk_real *__restrict__ B NK_ELEM_OUT) {
  const int e = (int)blockIdx.x * NK_ELEM_BLOCK + (int)threadIdx.x;
  if (e >= ne) return;
  const nk_elemv<Dual> w = nk_elem_view<Dual>(nn, ne, conn, nd, ed, u, v, e, -1);
  Dual out[NK_EL];
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) out[q] = Dual(NK_R(0));
  nk_element<Dual>(w, p, nk_cell{e, ne, nn}, out);
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) B[NK_ELEM_B_AT(q)] = out[q].d[0];
}
#else
// The element matrices: thread t takes local node b = t / ne of element e = t − b·ne (consecutive threads, consecutive
// elements), seeds the dof unknowns of local node b and stores dF_{a,c}/du_{b,c2} for all a, c, c2 — one stream each
extern "C" __global__ void __launch_bounds__(NK_ELEM_BLOCK)
nk_elem_jac(NK_ELEM_PARAMS, const nk_real *__restrict__ u, nk_real *__restrict__ M NK_ELEM_OUT) {
  const unsigned tu = blockIdx.x * (unsigned)NK_ELEM_BLOCK + threadIdx.x;
  if (tu >= (unsigned)ne * (unsigned)NK_NPE) return;
  const int b = (int)(tu / (unsigned)ne), e = (int)(tu - (unsigned)b * (unsigned)ne);
  const nk_elemv<Dual> w = nk_elem_view<Dual>(nn, ne, conn, nd, ed, u, nullptr, e, b);
  Dual out[NK_EL];
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) out[q] = Dual(NK_R(0));
  nk_element<Dual>(w, p, nk_cell{e, ne, nn}, out);
#pragma unroll
  for (int q = 0; q < NK_EL; ++q) {
#pragma unroll
    for (int c2 = 0; c2 < NK_DOF; ++c2) M[NK_ELEM_M_AT(q, b, c2)] = out[q].d[c2];
  }
}
#endif
)NKSRC";

// what the user's source is held to, for the message of a source that does not compile
static const char *k_elem_contract =
    "the contract is `template <typename T> __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f)` "
    "with u.at(a, c) unknown c at the element's a-th node (a = 0..NK_NPE-1), u.node(a) that node's index, u.x(a, k) node datum k "
    "at that node, u.w(k) datum k of the element (data are nk_real, never duals), s = {e, ne, nn} (e and ne within the element's "
    "block, NK_BLOCK), p the parameters and "
    "f[a*NK_DOF + c] the element's contribution to residual c of its a-th node (nk_real = double)";

// ----------------------------------------------------------------------------- compilation
enum { ESET_F = 0 /* nk_elem_residual + nk_elem_jvp, NK_CH = 1 */, ESET_JAC = 1 /* nk_elem_jac, NK_CH = dof */ };

static int elem_check_data_counts(int np, int nnode) {
  NK_REQUIRE(np >= 0 && np <= 32, "nparams = %d outside 0..32", np);
  NK_REQUIRE(nnode >= 0 && nnode <= 4, "nnode = %d outside 0..4 (data arrays of one double per node)", nnode);
  return NK_OK;
}
static int elem_check_counts(int npe, int dof, int np, int nnode, int nelem) {
  NK_TRY(elem_check_shape(npe, dof));
  NK_TRY(elem_check_data_counts(np, nnode));
  NK_REQUIRE(nelem >= 0 && nelem <= 4, "nelem = %d outside 0..4 (data arrays of one double per element)", nelem);
  return NK_OK;
}
static int elem_check_block_counts(int k, int npe, int dof, int np, int nnode, int nelem) {
  NK_TRY(elem_check_dof(dof));
  NK_TRY(elem_check_block_shape(k, npe, dof));
  NK_TRY(elem_check_data_counts(np, nnode));
  NK_REQUIRE(nelem >= 0 && nelem <= 4, "block %d: nelem = %d outside 0..4 (data arrays of one double per element)", k, nelem);
  return NK_OK;
}

// One program of one block. block < 0: the plain problem (its counts checked by its own rules, NK_BLOCK = 0); block_form: the
// kernels of a problem of several blocks
static int elem_compile(const char *source, int block, bool block_form, int npe, int dof, int np, int nnode, int nelem, int eset,
                        std::vector<char> *code, std::string *log) {
  NK_REQUIRE(source, "NULL source");
  if (block < 0)
    NK_TRY(elem_check_counts(npe, dof, np, nnode, nelem));
  else
    NK_TRY(elem_check_block_counts(block, npe, dof, np, nnode, nelem));
  const std::string full = std::string(nk_dual_prelude) + nk_seed_lift + k_elem_types + "\n// ---- user source\n" + source + "\n" +
                           k_elem_kernels;
  std::vector<std::string> defs = {
      "-DNK_NPE=" + std::to_string(npe), "-DNK_DOF=" + std::to_string(dof), "-DNK_NNODE=" + std::to_string(nnode),
      "-DNK_NELEM=" + std::to_string(nelem), "-DNK_CH=" + std::to_string(eset == ESET_JAC ? dof : 1),
      "-DNK_ELEM_SET=" + std::to_string(eset), "-DNK_SEED_SET=" + std::to_string(eset),
      "-DNK_BLOCK=" + std::to_string(block < 0 ? 0 : block)};
  if (block_form) defs.push_back("-DNK_ELEM_BLOCKS=1");
  const std::string what = block < 0 ? std::string("element") : "element block " + std::to_string(block);
  return nk_rtc_program(full, "nk_elem_user.hip", defs, source, what.c_str(), k_elem_contract, code, log);
}

// compile only (no device needed): both programs
extern "C" int nk_elem_compile_check(const char *source, int npe, int dof, int nparams, int nnode, int nelem, int64_t *code_bytes) {
  std::vector<char> code;
  std::string log;
  int64_t total = 0;
  for (int eset : {ESET_F, ESET_JAC}) {
    log.clear();
    NK_TRY(elem_compile(source, -1, false, npe, dof, nparams, nnode, nelem, eset, &code, &log));
    total += (int64_t)code.size();
  }
  if (code_bytes) *code_bytes = total;
  return NK_OK;
}

// the code object of one program (jac = 0: the residual and JVP kernels; 1: the element-matrix kernel) for inspection
extern "C" int nk_elem_code_object(const char *source, int npe, int dof, int nparams, int nnode, int nelem, int jac, void *buf,
                                   int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(elem_compile(source, -1, false, npe, dof, nparams, nnode, nelem, jac != 0 ? ESET_JAC : ESET_F, &code, &log));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}
// the same for block `block` of a problem of several blocks: the block form of the kernels, npe = 1 allowed
extern "C" int nk_elem_block_code_object(const char *source, int block, int npe, int dof, int nparams, int nnode, int nelem, int jac,
                                         void *buf, int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  NK_REQUIRE(block >= 0 && block < 8, "block = %d outside 0..7", block);
  std::vector<char> code;
  std::string log;
  NK_TRY(elem_compile(source, block, true, npe, dof, nparams, nnode, nelem, jac != 0 ? ESET_JAC : ESET_F, &code, &log));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}

// ----------------------------------------------------------------------------- the gather
enum { GATHER_F = 0, GATHER_JV = 1, GATHER_J = 2 };

// One output per thread (x: the list, y: the component c, or the pair c·dof + c2): out = Σ buf[list[q] + offset] over the
// thread's list in list order (ascending elements), or what a fixed row holds instead.
//   GATHER_F / GATHER_JV  item t = node i, offset c·ne, out[c·nn + i]; fixed: x[r] − g[r] / x[r] with x = u / v
//   GATHER_J              item t = global slot of the pattern (node i = slotnode[t], slot s = t − (arp[i] + i)), offset
//                         (c·L + c2)·ne, out at nk_graph_pattern's value index; fixed row (c, i): 1 at c2 = c, s = spos[i], else 0
// Every index is below ne·L² or the pattern's entry count, both checked against INT32_MAX at creation.
__global__ void __launch_bounds__(256)
k_elem_gather(int mode, int items, int dof, int nn, int ne, int L, const int *__restrict__ lptr, const int *__restrict__ list,
              const double *__restrict__ buf, const int *__restrict__ mask, const double *__restrict__ x,
              const double *__restrict__ g, const int *__restrict__ slotnode, const int *__restrict__ arp,
              const int *__restrict__ spos, double *__restrict__ out) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= items) return;
  const int k = (int)blockIdx.y;
  int o, off;
  if (mode != GATHER_J) {
    o = k * nn + t;
    off = k * ne;
    if (mask[o] != 0) {
      out[o] = mode == GATHER_F ? x[o] - g[o] : x[o];
      return;
    }
  } else {
    const int c = k / dof, c2 = k - c * dof, i = slotnode[t];
    const int b = arp[i] + i, wd = arp[i + 1] - arp[i] + 1, s = t - b;
    o = c * dof * items + dof * b + c2 * wd + s;
    off = (c * L + c2) * ne;
    if (mask[c * nn + i] != 0) {
      out[o] = (c2 == c && s == spos[i]) ? 1.0 : 0.0;
      return;
    }
  }
  double sum = 0.0;
  const int q1 = lptr[t + 1];
  for (int q = lptr[t]; q < q1; ++q) sum += buf[list[q] + off];
  out[o] = sum;
}

__global__ void __launch_bounds__(256)
k_elem_fixed_values(int n, const int *__restrict__ mask, const double *__restrict__ g, double *__restrict__ u) {
  const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (r < n) u[r] = mask[r] != 0 ? g[r] : 0.0;
}

// ----------------------------------------------------------------------------- the problem object
// what a block owns: its connectivity, its element data, where its numbers start in B and M and, from block 1 on, its programs
// (block 0's are the nk_compiled's)
struct nk_elem_block {
  int ne = 0, npe = 0, nelem = 0;
  int base = 0, mbase = 0;        // Σ npe_j·ne_j and Σ npe_j²·ne_j over the blocks before this one
  int32_t *d_conn = nullptr;      // node-major: local node a of element e at a·ne + e
  double *d_elem = nullptr;       // nelem·ne doubles, zero at creation
  nk_compiled_programs prog;
};

struct nk_elem_state {
  nk_compiled c;                                     // the context, block 0's programs, p and the pattern
  int nn = 0, dof = 0, nnode = 0, nslots = 0;
  bool block_form = false;                           // the block layout of B and M (the top of the file); else the plain one
  int tb = 0, tm = 0;                                // Σ npe·ne and Σ npe²·ne over all blocks
  std::vector<nk_elem_block> blk;
  int32_t *d_arp = nullptr;                          // rowptr of the node graph (nn + 1)
  int32_t *d_slotnode = nullptr, *d_spos = nullptr;  // the node of every global slot; the self slot of every node
  int32_t *d_rptr = nullptr, *d_rlist = nullptr;     // the row lists: per node (nn + 1; Σ ne·npe)
  int32_t *d_eptr = nullptr, *d_elist = nullptr;     // the entry lists: per global slot (nslots + 1; Σ ne·npe²)
  int32_t *d_mask = nullptr;                         // dof·nn: 0 = free
  double *d_fixed = nullptr;                         // dof·nn: the value of a fixed unknown
  double *d_node = nullptr;                          // nnode·nn doubles, zero at creation
  double *d_B = nullptr;                             // dof·Σ npe·ne: the element vectors
  double *d_M = nullptr;                             // dof²·Σ npe²·ne: the element matrices
};

void nk_elem_state_destroy(nk_elem_state *S) {
  if (!S) return;
  nk_compiled_free(&S->c);
  for (nk_elem_block &b : S->blk) {
    nk_compiled_unload(&b.prog);
    hipFree(b.d_conn);
    hipFree(b.d_elem);
  }
  hipFree(S->d_arp);
  hipFree(S->d_slotnode);
  hipFree(S->d_spos);
  hipFree(S->d_rptr);
  hipFree(S->d_rlist);
  hipFree(S->d_eptr);
  hipFree(S->d_elist);
  hipFree(S->d_mask);
  hipFree(S->d_fixed);
  hipFree(S->d_node);
  hipFree(S->d_B);
  hipFree(S->d_M);
  delete S;
}

static const nk_compiled_programs &elem_programs(const nk_elem_state *S, int k) {
  return k == 0 ? static_cast<const nk_compiled_programs &>(S->c) : S->blk[(size_t)k].prog;
}

// One launch of a generated kernel of block k over `items` threads on `stream`: the block's mesh and what the problem owns, then
// `rest`, then — in the block form — where the block's numbers start in the output buffer and the buffer's component stride
static int elem_launch(nk_elem_state *S, int k, hipFunction_t fn, int64_t items, std::initializer_list<void *> rest, int *base,
                       int *stride, void *stream) {
  nk_elem_block &b = S->blk[(size_t)k];
  void *args[12] = {&S->nn, &b.ne, &b.d_conn, &S->c.d_params, &S->d_node, &b.d_elem};
  int n = 6;
  for (void *a : rest) args[n++] = a;
  if (S->block_form) args[n++] = base, args[n++] = stride;
  return nk_compiled_launch(&S->c, fn, items, args, stream);
}

// the gather of one callback on the same stream, timed the same way; its time goes to the family "elem_gather", so that the
// callback's family (residual, jvp, jacfill) holds the generated kernels alone and the launches can be told apart
static bool elem_gather_events(nk_ctx *ctx, void *stream, hipEvent_t *e0, hipEvent_t *e1) {
  nk_prof &p = ctx->prof;
  if (!p.on || (hipStream_t)stream != ctx->stream || p.cur_id < 0) return false;
  const int family = p.cur_id;
  p.cur_id = NK_K_ELEM_GATHER;
  const bool ok = nk_prof_next(ctx, e0, e1);
  p.cur_id = family;
  return ok;
}
// One gather for all blocks. In the block form the kernel's `ne` is the component stride of the buffer (Σ npe·ne; the fill:
// Σ npe²·ne) and its `L` the component count, so that its offsets c·ne and (c·L + c2)·ne are the block layout's.
static int elem_gather(nk_elem_state *S, int mode, const double *x, double *out, void *stream) {
  const bool jac = mode == GATHER_J;
  const int items = jac ? S->nslots : S->nn;
  const int ne = S->block_form ? (jac ? S->tm : S->tb) : S->blk[0].ne, L = S->block_form ? S->dof : S->blk[0].npe * S->dof;
  const dim3 grid((unsigned)((items + 255) / 256), (unsigned)(jac ? S->dof * S->dof : S->dof)), block(256);
  const int32_t *lptr = jac ? S->d_eptr : S->d_rptr, *list = jac ? S->d_elist : S->d_rlist;
  const double *buf = jac ? S->d_M : S->d_B;
  hipEvent_t e0, e1;
  if (elem_gather_events(S->c.ctx, stream, &e0, &e1))
    hipExtLaunchKernelGGL(k_elem_gather, grid, block, 0, (hipStream_t)stream, e0, e1, 0, mode, items, S->dof, S->nn, ne, L, lptr,
                          list, buf, S->d_mask, x, S->d_fixed, S->d_slotnode, S->d_arp, S->d_spos, out);
  else
    hipLaunchKernelGGL(k_elem_gather, grid, block, 0, (hipStream_t)stream, mode, items, S->dof, S->nn, ne, L, lptr, list, buf,
                       S->d_mask, x, S->d_fixed, S->d_slotnode, S->d_arp, S->d_spos, out);
  return hipGetLastError() != hipSuccess;
}

// a callback: one generated launch per block, then the one gather (never one gather per block: the sum would become a
// read-modify-write)
static int elem_cb_residual(void *user, const double *u, double *f, void *stream) {
  nk_elem_state *S = (nk_elem_state *)user;
  for (int k = 0; k < (int)S->blk.size(); ++k)
    if (elem_launch(S, k, elem_programs(S, k).fn_res, S->blk[(size_t)k].ne, {&u, &S->d_B}, &S->blk[(size_t)k].base, &S->tb, stream))
      return 1;
  return elem_gather(S, GATHER_F, u, f, stream);
}
static int elem_cb_jvp(void *user, const double *v, const double *u, double *jv, void *stream) {
  nk_elem_state *S = (nk_elem_state *)user;
  for (int k = 0; k < (int)S->blk.size(); ++k)
    if (elem_launch(S, k, elem_programs(S, k).fn_jvp, S->blk[(size_t)k].ne, {&u, &v, &S->d_B}, &S->blk[(size_t)k].base, &S->tb, stream))
      return 1;
  return elem_gather(S, GATHER_JV, v, jv, stream);
}
static int elem_cb_jac(void *user, const double *u, double *vals, void *stream) {
  nk_elem_state *S = (nk_elem_state *)user;
  for (int k = 0; k < (int)S->blk.size(); ++k) {
    nk_elem_block &b = S->blk[(size_t)k];
    if (elem_launch(S, k, elem_programs(S, k).fn_jac, (int64_t)b.ne * b.npe, {&u, &S->d_M}, &b.mbase, &S->tm, stream)) return 1;
  }
  return elem_gather(S, GATHER_J, u, vals, stream);
}

// zeros, with the values of the fixed unknowns written in
int nk_elem_initial_guess(nk_problem *P, double *d_u) {
  nk_elem_state *S = P->elem;
  const int n = S->nn * S->dof;
  NK_LAUNCH(S->c.ctx, k_elem_fixed_values, dim3((unsigned)((n + 255) / 256)), dim3(256), n, S->d_mask, S->d_fixed, d_u);
  NK_HIP(hipGetLastError());
  return NK_OK;
}

// datum k of the elements of a block (block < 0: of the nodes): its doubles on the device
static int elem_data_ptr(nk_problem *P, int block, int k, double **d, size_t *bytes) {
  NK_REQUIRE(P, "NULL argument");
  NK_REQUIRE(P->elem, "the problem is not a compiled element problem (kind %d): it has no node or element data", (int)P->kind);
  nk_elem_state *S = P->elem;
  if (block < 0) {
    NK_REQUIRE(k >= 0 && k < S->nnode, "node datum k = %d outside 0..%d (the problem was created with nnode = %d)", k,
               S->nnode - 1, S->nnode);
    *d = S->d_node + (size_t)k * (size_t)S->nn;
    *bytes = (size_t)S->nn * sizeof(double);
    return NK_OK;
  }
  NK_REQUIRE(block < (int)S->blk.size(), "block = %d outside 0..%d (the problem has %d element block%s)", block,
             (int)S->blk.size() - 1, (int)S->blk.size(), S->blk.size() == 1 ? "" : "s");
  const nk_elem_block &b = S->blk[(size_t)block];
  if (S->blk.size() == 1)
    NK_REQUIRE(k >= 0 && k < b.nelem, "element datum k = %d outside 0..%d (the problem was created with nelem = %d)", k,
               b.nelem - 1, b.nelem);
  else
    NK_REQUIRE(k >= 0 && k < b.nelem, "block %d: element datum k = %d outside 0..%d (the block was created with nelem = %d)", block,
               k, b.nelem - 1, b.nelem);
  *d = b.d_elem + (size_t)k * (size_t)b.ne;
  *bytes = (size_t)b.ne * sizeof(double);
  return NK_OK;
}
static int elem_data_set(nk_problem *P, int block, int k, const double *data, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(elem_data_ptr(P, block, k, &d, &bytes));
  NK_TRY(nk_compiled_data_copy(P, d, bytes, data, memspace, true));
  nk_compiled_data_changed(P);
  return NK_OK;
}
static int elem_data_get(nk_problem *P, int block, int k, double *out, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(elem_data_ptr(P, block, k, &d, &bytes));
  return nk_compiled_data_copy(P, d, bytes, out, memspace, false);
}
// on_elements = 1: block 0's element data, 0: the node data
extern "C" int nk_problem_set_elem_data(nk_problem *P, int on_elements, int k, const double *data, int memspace) {
  return elem_data_set(P, on_elements ? 0 : -1, k, data, memspace);
}
extern "C" int nk_problem_get_elem_data(nk_problem *P, int on_elements, int k, double *out, int memspace) {
  return elem_data_get(P, on_elements ? 0 : -1, k, out, memspace);
}
extern "C" int nk_problem_set_elem_block_data(nk_problem *P, int block, int k, const double *data, int memspace) {
  NK_REQUIRE(block >= 0, "block = %d is negative", block);
  return elem_data_set(P, block, k, data, memspace);
}
extern "C" int nk_problem_get_elem_block_data(nk_problem *P, int block, int k, double *out, int memspace) {
  NK_REQUIRE(block >= 0, "block = %d is negative", block);
  return elem_data_get(P, block, k, out, memspace);
}
// the blocks of an element problem: their count and, for the first `cap` of them, ne, npe and nelem (NULL arrays: the count only)
extern "C" int nk_problem_elem_blocks(nk_problem *P, int *nblocks, int cap, int64_t *ne, int *npe, int *nelem) {
  NK_REQUIRE(P && nblocks, "NULL argument");
  NK_REQUIRE(P->elem, "the problem is not a compiled element problem (kind %d): it has no element blocks", (int)P->kind);
  const nk_elem_state *S = P->elem;
  *nblocks = (int)S->blk.size();
  for (int k = 0; k < *nblocks && k < cap; ++k) {
    if (ne) ne[k] = S->blk[(size_t)k].ne;
    if (npe) npe[k] = S->blk[(size_t)k].npe;
    if (nelem) nelem[k] = S->blk[(size_t)k].nelem;
  }
  return NK_OK;
}

extern "C" int nk_problem_set_elem_fixed(nk_problem *P, const int32_t *mask, const double *values, int memspace) {
  NK_REQUIRE(P && mask, "NULL argument");
  NK_REQUIRE(P->elem, "the problem is not a compiled element problem (kind %d): it has no fixed unknowns", (int)P->kind);
  NK_REQUIRE(memspace == NK_HOST || memspace == NK_DEVICE, "memspace = %d is neither NK_HOST nor NK_DEVICE", memspace);
  nk_elem_state *S = P->elem;
  const size_t n = (size_t)S->nn * (size_t)S->dof;
  const hipMemcpyKind kind = memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  NK_HIP(hipSetDevice(S->c.ctx->device));
  NK_HIP(nk_memcpy(S->c.ctx, S->d_mask, mask, n * sizeof(int32_t), kind));
  if (values)
    NK_HIP(nk_memcpy(S->c.ctx, S->d_fixed, values, n * sizeof(double), kind));
  else
    NK_HIP(nk_memset(S->c.ctx, S->d_fixed, 0, n * sizeof(double)));
  nk_compiled_data_changed(P);   // a Jacobian cached for the same u has the old rows
  return NK_OK;
}
extern "C" int nk_problem_get_elem_fixed(nk_problem *P, int32_t *mask, double *values, int memspace) {
  NK_REQUIRE(P && (mask || values), "NULL argument");
  NK_REQUIRE(P->elem, "the problem is not a compiled element problem (kind %d): it has no fixed unknowns", (int)P->kind);
  NK_REQUIRE(memspace == NK_HOST || memspace == NK_DEVICE, "memspace = %d is neither NK_HOST nor NK_DEVICE", memspace);
  nk_elem_state *S = P->elem;
  const size_t n = (size_t)S->nn * (size_t)S->dof;
  const hipMemcpyKind kind = memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  NK_HIP(hipSetDevice(S->c.ctx->device));
  if (mask) NK_HIP(nk_memcpy(S->c.ctx, mask, S->d_mask, n * sizeof(int32_t), kind));
  if (values) NK_HIP(nk_memcpy(S->c.ctx, values, S->d_fixed, n * sizeof(double), kind));
  return NK_OK;
}

// The problem over a mesh of blocks. A plain problem (m.named false) and a named mesh of one block with npe >= 2 get the plain
// layout — the same programs, buffers and launches; every other mesh the block layout.
static int elem_create(nk_ctx *ctx, const elem_mesh &m, const char *const *sources, int dof, const int *nelem, const double *params,
                       int nparams, int nnode, nk_problem **out) {
  NK_REQUIRE(ctx && out, "NULL argument");
  NK_REQUIRE(params || nparams == 0, "NULL params with nparams = %d", nparams);
  // the mesh and the counts first: every refusal comes before anything is compiled or allocated
  NK_TRY(elem_validate(m, dof));
  NK_REQUIRE(sources && nelem, "NULL argument");
  for (int k = 0; k < m.nblocks; ++k) {
    if (m.named) {
      NK_REQUIRE(sources[k], "block %d: NULL source", k);
      NK_TRY(elem_check_block_counts(k, m.npe[k], dof, nparams, nnode, nelem[k]));
    } else {
      NK_REQUIRE(sources[k], "NULL argument");
      NK_TRY(elem_check_counts(m.npe[k], dof, nparams, nnode, nelem[k]));
    }
  }
  const int64_t nn = m.nn;
  std::vector<int32_t> arp, aci;
  NK_TRY(elem_adjacency_build(m, &arp, &aci));
  const int64_t nedges = (int64_t)aci.size(), slots = nedges + nn, n = nn * dof, nnz = (int64_t)dof * dof * slots;
  NK_REQUIRE(slots <= (int64_t)INT32_MAX / (dof * dof), "%lld nodes and %lld node pairs with dof = %d: the pattern's entry count "
             "dof·dof·(pairs + nn) exceeds INT32_MAX, its 32-bit indices cannot hold it", (long long)nn, (long long)nedges, dof);
  if (ctx->nranks > 1)
    NK_FAIL(NK_E_UNSUPPORTED, "a compiled element problem runs on one rank, the context has %d (partitioning a mesh is not "
            "built)", ctx->nranks);
  NK_HIP(hipSetDevice(ctx->device));
  const bool block_form = m.nblocks > 1 || m.npe[0] < 2;
  std::vector<std::vector<char>> code_f((size_t)m.nblocks), code_j((size_t)m.nblocks);
  std::string log;
  for (int k = 0; k < m.nblocks; ++k) {
    const int block = m.named ? k : -1;
    log.clear();
    NK_TRY(elem_compile(sources[k], block, block_form, m.npe[k], dof, nparams, nnode, nelem[k], ESET_F, &code_f[(size_t)k], &log));
    log.clear();
    NK_TRY(elem_compile(sources[k], block, block_form, m.npe[k], dof, nparams, nnode, nelem[k], ESET_JAC, &code_j[(size_t)k], &log));
  }

  // the pattern (nk_graph_pattern's), the slot tables, the node-major connectivities and the two sets of lists. Where the
  // contribution (a, c = 0) of element e of block k, and (a, b, c = c2 = 0), start in B and M:
  //   plain   a·dof·ne + e            (a·dof·L + b·dof)·ne + e            (L = npe·dof)
  //   blocks  base_k + a·ne_k + e     mbase_k + (a·npe_k + b)·ne_k + e
  std::vector<int64_t> base((size_t)m.nblocks + 1, 0), mbase((size_t)m.nblocks + 1, 0);
  for (int k = 0; k < m.nblocks; ++k) {
    base[(size_t)k + 1] = base[(size_t)k] + m.npe[k] * m.ne[k];
    mbase[(size_t)k + 1] = mbase[(size_t)k] + (int64_t)m.npe[k] * m.npe[k] * m.ne[k];
  }
  const int64_t tb = base[(size_t)m.nblocks], tm = mbase[(size_t)m.nblocks];
  std::vector<int32_t> rp((size_t)n + 1), slotnode, spos;
  std::vector<int64_t> gc((size_t)nnz);
  nk_graph_pattern_fill64(nn, nedges, arp.data(), aci.data(), dof, rp.data(), gc.data());
  nk_graph_slots(nn, arp.data(), aci.data(), &slotnode, &spos);
  std::vector<std::vector<int32_t>> connT((size_t)m.nblocks);
  std::vector<int32_t> rptr((size_t)nn + 1, 0), rlist((size_t)tb);
  std::vector<int32_t> eptr((size_t)slots + 1, 0), elist((size_t)tm), eslot((size_t)tm);
  for (int k = 0; k < m.nblocks; ++k) {
    const int32_t *conn = m.conn[k];
    const int64_t ne = m.ne[k];
    const int npe = m.npe[k];
    connT[(size_t)k].resize((size_t)(ne * npe));
    for (int64_t e = 0; e < ne; ++e)
      for (int a = 0; a < npe; ++a) {
        const int32_t i = conn[e * npe + a];
        connT[(size_t)k][(size_t)(a * ne + e)] = i;
        rptr[(size_t)i + 1]++;
        const int32_t *row = aci.data() + arp[(size_t)i], *end = aci.data() + arp[(size_t)i + 1];
        for (int b = 0; b < npe; ++b) {
          const int32_t j = conn[e * npe + b];
          int64_t s = spos[(size_t)i];
          if (j != i) {
            const int64_t pos = std::lower_bound(row, end, j) - row;
            s = pos + (pos >= spos[(size_t)i] ? 1 : 0);
          }
          const int64_t t = arp[(size_t)i] + i + s;
          eslot[(size_t)(mbase[(size_t)k] + (e * npe + a) * npe + b)] = (int32_t)t;
          eptr[(size_t)t + 1]++;
        }
      }
  }
  for (int64_t i = 0; i < nn; ++i) rptr[(size_t)i + 1] += rptr[(size_t)i];
  for (int64_t t = 0; t < slots; ++t) eptr[(size_t)t + 1] += eptr[(size_t)t];
  {
    std::vector<int32_t> rat(rptr.begin(), rptr.end() - 1), eat(eptr.begin(), eptr.end() - 1);
    for (int k = 0; k < m.nblocks; ++k) {   // blocks in order, elements ascending: the order every list is summed in
      const int32_t *conn = m.conn[k];
      const int64_t ne = m.ne[k], L = (int64_t)m.npe[k] * dof;
      const int npe = m.npe[k];
      for (int64_t e = 0; e < ne; ++e)
        for (int a = 0; a < npe; ++a) {
          rlist[(size_t)rat[(size_t)conn[e * npe + a]]++] =
              (int32_t)(block_form ? base[(size_t)k] + a * ne + e : (int64_t)a * dof * ne + e);
          for (int b = 0; b < npe; ++b)
            elist[(size_t)eat[(size_t)eslot[(size_t)(mbase[(size_t)k] + (e * npe + a) * npe + b)]]++] =
                (int32_t)(block_form ? mbase[(size_t)k] + ((int64_t)a * npe + b) * ne + e : ((int64_t)a * dof * L + b * dof) * ne + e);
        }
    }
  }

  nk_elem_state *S = new nk_elem_state();
  auto guard = nk_make_guard(S, nk_elem_state_destroy);
  S->c.ctx = ctx;
  S->nn = (int)nn;
  S->dof = dof;
  S->nnode = nnode;
  S->nslots = (int)slots;
  S->block_form = block_form;
  S->tb = (int)tb;
  S->tm = (int)tm;
  S->blk.resize((size_t)m.nblocks);
  for (int k = 0; k < m.nblocks; ++k) {
    nk_elem_block &b = S->blk[(size_t)k];
    b.ne = (int)m.ne[k];
    b.npe = m.npe[k];
    b.nelem = nelem[k];
    b.base = (int)base[(size_t)k];
    b.mbase = (int)mbase[(size_t)k];
    nk_compiled_programs *prog = k == 0 ? static_cast<nk_compiled_programs *>(&S->c) : &b.prog;
    NK_TRY(nk_compiled_load(prog, code_f[(size_t)k], code_j[(size_t)k], "nk_elem_residual", "nk_elem_jvp", "nk_elem_jac", "element"));
    NK_TRY(nk_upload(ctx, &b.d_conn, connT[(size_t)k]));
    NK_TRY(nk_compiled_zeros(ctx, &b.d_elem, (size_t)b.nelem * (size_t)b.ne));   // zero until the data are set
  }
  NK_TRY(nk_upload(ctx, &S->d_arp, arp));
  NK_TRY(nk_upload(ctx, &S->d_slotnode, slotnode));
  NK_TRY(nk_upload(ctx, &S->d_spos, spos));
  NK_TRY(nk_upload(ctx, &S->d_rptr, rptr));
  NK_TRY(nk_upload(ctx, &S->d_rlist, rlist));
  NK_TRY(nk_upload(ctx, &S->d_eptr, eptr));
  NK_TRY(nk_upload(ctx, &S->d_elist, elist));
  NK_TRY(nk_compiled_params_init(&S->c, params, nparams));
  NK_TRY(nk_compiled_zeros(ctx, &S->d_node, (size_t)nnode * (size_t)nn));   // zero until nk_problem_set_elem_data
  NK_TRY(nk_compiled_zeros(ctx, &S->d_mask, (size_t)n));                    // nothing fixed until nk_problem_set_elem_fixed
  NK_TRY(nk_compiled_zeros(ctx, &S->d_fixed, (size_t)n));
  NK_TRY(nk_dev_alloc(&S->d_B, (size_t)dof * (size_t)tb));
  NK_TRY(nk_dev_alloc(&S->d_M, (size_t)dof * (size_t)dof * (size_t)tm));
  NK_TRY(nk_csr_create_local(ctx, n, n, 0, rp, gc, nullptr, &S->c.pattern));
  NK_TRY(nk_compiled_problem(&S->c, n, n, 0, params, nparams, {elem_cb_residual, elem_cb_jvp, nullptr, elem_cb_jac}, S, out));
  (*out)->elem = guard.release();
  return NK_OK;
}

extern "C" int nk_problem_create_elements(nk_ctx *ctx, const char *source, int64_t nn, int64_t ne, int npe, const int32_t *conn,
                                          int dof, const double *params, int nparams, int nnode, int nelem, nk_problem **out) {
  NK_REQUIRE(ctx && source && out, "NULL argument");
  return elem_create(ctx, elem_mesh{nn, 1, &ne, &npe, &conn, false}, &source, dof, &nelem, params, nparams, nnode, out);
}

extern "C" int nk_problem_create_element_blocks(nk_ctx *ctx, int64_t nn, int dof, int nblocks, const char *const *sources,
                                                const int64_t *ne, const int *npe, const int32_t *const *conn, const int *nelem,
                                                const double *params, int nparams, int nnode, nk_problem **out) {
  return elem_create(ctx, elem_mesh{nn, nblocks, ne, npe, conn, true}, sources, dof, nelem, params, nparams, nnode, out);
}
