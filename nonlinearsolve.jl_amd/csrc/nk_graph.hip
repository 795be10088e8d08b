// Compiled graph problems: a residual given node by node over any sparse adjacency, handed over as HIP C++ source
//     template <typename T> __device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f);
// and compiled at run time (hiprtc, gfx950) into three kernels — what nk_grid.hip does for tensor-product grids, for the
// reference's ordinary use: NonlinearFunction(f; jac_prototype = any sparse pattern) with forward-mode duals and sparse AD.
// The user supplies a CSR graph of the nodes (0-based, columns strictly ascending within a row, no self-loops, possibly
// structurally nonsymmetric, possibly without edges) and loops over a node's edges in the source.
//
//   nk_graph_residual   T = nk_real                              one node per thread
//   nk_graph_jvp        T = Dual, NK_CH = 1: value u, partial v  one node per thread — exact, one launch
//   nk_graph_jac        T = Dual, NK_CH = dof, unit seeds        one SLOT per thread
//
// Numbering is component-major: unknown c of node i is element c·nn + i; edge datum k of edge e (its position in colind) is
// element k·ne + e and node datum k of node i element k·nn + i of two buffers the problem owns (zero at creation).
//
// Bytes. The edge loop is the user's, and nbr(e, c) is one gathered load u[c·nn + col[e]]. Algorithmic bytes per node:
// 16·dof + 4 + deg·(4 + 8·r_e) + 8·r_n, with r_e and r_n the edge and node data arrays the source reads (the JVP adds 8·dof)
// — the node's own unknowns and residuals, its row pointer, and per edge the column and the edge data. The neighbour values
// are expected from cache: that holds for a bandwidth-reducing ordering of the nodes (neighbours are then near in memory and
// shared between adjacent threads) and does not for a random one. The library does not reorder the user's graph.
//
// The pattern. Row (c, i) holds, for every component c2 in order, the node itself and its neighbours in ascending node order:
// dof·(deg_i + 1) entries with ascending columns c2·nn + node, structural even where a derivative vanishes. The deg_i + 1
// column nodes of node i are its slots; the self slot is spos_i = the number of neighbours smaller than i, edge e is slot
// e + (e >= spos_i). All ne + nn slots of the graph are numbered node after node — slot s of node i is rowptr[i] + i + s — and
// dF_c(i)/du_c2(slot s) is element c·dof·(ne + nn) + dof·(rowptr[i] + i) + c2·(deg_i + 1) + s of the value array.
//
// The fill. Thread t of ne + nn takes slot t: it finds its node in a slot → node array built at creation (4 bytes against the
// 8·dof² the thread stores) and the node's spos in a per-node array, evaluates nk_node for that node with unit seeds on the dof
// unknowns of its slot only, and stores the dof × dof block. Consecutive threads write consecutive elements of each of the
// dof² streams; the threads of one node re-read the same neighbourhood from cache. The work is Σ (deg_i + 1)·deg_i edge terms,
// not Σ deg_i: the price of a run-time degree with a compile-time dual width. No atomics anywhere, and every sum runs in the
// source's own edge order, so all three kernels are bit-reproducible from run to run.
//
// The result is an nk_problem of the callback kind NK_PROBLEM_USER whose callbacks are the three launchers below, with
// user_pattern set to the pattern above: every consumer treats it as any callback problem with a jac_prototype (matrix-free
// GMRES, the concrete-J path, the coloured assembly, Jᵀv through the transposed SpMV, every `precs` object). One rank.
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- the adjacency (host only)
// every rule of the header, the first offending row named; ne from rowptr[nn]
static int graph_validate(int64_t nn, const int32_t *rowptr, const int32_t *colind, int dof, int64_t *ne_out) {
  NK_REQUIRE(rowptr, "NULL rowptr");
  NK_REQUIRE(nn >= 1 && nn <= INT32_MAX, "nn = %lld: a graph has 1..INT32_MAX nodes", (long long)nn);
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per node)", dof);
  NK_REQUIRE(rowptr[0] == 0, "row 0: rowptr[0] = %d, the adjacency is 0-based and starts at 0", (int)rowptr[0]);
  for (int64_t i = 0; i < nn; ++i)
    NK_REQUIRE(rowptr[i + 1] >= rowptr[i], "row %lld: rowptr decreases (%d after %d)", (long long)i, (int)rowptr[i + 1],
               (int)rowptr[i]);
  const int64_t ne = rowptr[nn];
  NK_REQUIRE(colind || ne == 0, "NULL colind with %lld edges", (long long)ne);
  NK_REQUIRE(ne + nn <= (int64_t)INT32_MAX / (dof * dof), "%lld nodes and %lld edges with dof = %d: dof·dof·(ne + nn) exceeds "
             "INT32_MAX, the pattern's 32-bit indices cannot hold it", (long long)nn, (long long)ne, dof);
  for (int64_t i = 0; i < nn; ++i)
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int64_t j = colind[e];
      NK_REQUIRE(j >= 0 && j < nn, "row %lld: column %lld outside 0..%lld", (long long)i, (long long)j, (long long)nn - 1);
      NK_REQUIRE(j != i, "row %lld: a self-loop (column %lld) — the node itself is always an argument of its residual and always "
                 "a column, leave it out of the adjacency", (long long)i, (long long)j);
      if (e > rowptr[i])
        NK_REQUIRE(j > colind[e - 1], "row %lld: column %lld after %d — columns are strictly ascending within a row (no "
                   "duplicate, no descending column)", (long long)i, (long long)j, (int)colind[e - 1]);
    }
  *ne_out = ne;
  return NK_OK;
}

// the Jacobian's CSR of a validated adjacency (arrays nullable) and, per node, its self slot
template <class Col>
static void graph_pattern_fill(int64_t nn, int64_t ne, const int32_t *rowptr, const int32_t *colind, int dof, int32_t *jrowptr,
                               Col *jcolind) {
  const int64_t slots = ne + nn;
  for (int c = 0; c < dof; ++c)
    for (int64_t i = 0; i < nn; ++i) {
      const int64_t e0 = rowptr[i], dg = rowptr[i + 1] - e0, base = (int64_t)c * dof * slots + dof * (e0 + i);
      if (jrowptr) jrowptr[c * nn + i] = (int32_t)base;
      if (!jcolind) continue;
      for (int c2 = 0; c2 < dof; ++c2) {
        int64_t at = base + c2 * (dg + 1);
        bool self_done = false;
        for (int64_t e = 0; e < dg; ++e) {
          if (!self_done && colind[e0 + e] > i) { jcolind[at++] = (Col)(c2 * nn + i); self_done = true; }
          jcolind[at++] = (Col)(c2 * nn + colind[e0 + e]);
        }
        if (!self_done) jcolind[at++] = (Col)(c2 * nn + i);
      }
    }
  if (jrowptr) jrowptr[dof * nn] = (int32_t)((int64_t)dof * dof * slots);
}

extern "C" int nk_graph_pattern(int64_t nn, const int32_t *rowptr, const int32_t *colind, int dof, int32_t *jrowptr,
                                int32_t *jcolind, int64_t *nnz) {
  NK_REQUIRE(jrowptr || nnz, "NULL argument");
  int64_t ne = 0;
  NK_TRY(graph_validate(nn, rowptr, colind, dof, &ne));
  graph_pattern_fill<int32_t>(nn, ne, rowptr, colind, dof, jrowptr, jcolind);
  if (nnz) *nnz = (int64_t)dof * dof * (ne + nn);
  return NK_OK;
}
void nk_graph_pattern_fill64(int64_t nn, int64_t ne, const int32_t *rowptr, const int32_t *colind, int dof, int32_t *jrowptr,
                             int64_t *jcolind) {
  graph_pattern_fill<int64_t>(nn, ne, rowptr, colind, dof, jrowptr, jcolind);
}
// the node of every global slot and, per node, its self slot: the number of neighbours smaller than the node
void nk_graph_slots(int64_t nn, const int32_t *rowptr, const int32_t *colind, std::vector<int32_t> *slotnode, std::vector<int32_t> *spos) {
  slotnode->resize((size_t)(rowptr[nn] + nn));
  spos->resize((size_t)nn);
  for (int64_t i = 0; i < nn; ++i) {
    int32_t below = 0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1] && colind[e] < i; ++e) ++below;
    (*spos)[(size_t)i] = below;
    for (int64_t s = rowptr[i] + i; s < rowptr[i + 1] + i + 1; ++s) (*slotnode)[(size_t)s] = (int32_t)i;
  }
}

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)
// The program is: nk_dual_prelude, nk_seed_lift, k_graph_types, the user's source, k_graph_kernels. What a program is comes from
// its options: -DNK_DOF, -DNK_NEDGE, -DNK_NNODE (the data arrays per edge and per node), -DNK_CH, -DNK_GRAPH_SET = -DNK_SEED_SET
// (0: residual and JVP, 1: the fill) and -DNK_GRAPH_FILL_NODE (the A/B form of the fill).
static const char *k_graph_types = R"NKSRC(
// ---- compiled graph problems: the node and its neighbours
#define NK_GRAPH_BLOCK 256
struct nk_vertex { int i, nn, deg; };
// What the source sees of node i. Unknowns are T, data are nk_real (constants of the differentiation). An edge e outside
// 0..deg()-1, a component outside 0..NK_DOF-1 and a datum k outside the declared count read NaN (node(e): -1): a wrong source
// shows at once and reads nothing it does not own
template <typename T>
struct nk_nbrs {
  const nk_real *__restrict__ nk_u;
  const nk_real *__restrict__ nk_v;
  const int *__restrict__ nk_col;      // the node's edges: nk_col[0 .. nk_dg)
  const nk_real *__restrict__ nk_ew;   // datum k of the node's edge e: nk_ew[k·ne + e]
  const nk_real *__restrict__ nk_nd;   // datum k of node j: nk_nd[k·nn + j]
  int nk_nn, nk_ne, nk_i, nk_dg, nk_spos, nk_hot;   // nk_hot: the slot that carries the unit seeds (the fill), else -1
  __device__ __forceinline__ bool nk_edge_ok(int e) const { return (unsigned)e < (unsigned)nk_dg; }
  __device__ __forceinline__ int deg() const { return nk_dg; }
  __device__ __forceinline__ T self(int c = 0) const {
    if ((unsigned)c >= (unsigned)NK_DOF) return T(NK_R(__builtin_nan("")));
    return nk_lift<T>::at(nk_u[c * nk_nn + nk_i], nk_v, c * nk_nn + nk_i, c, nk_hot == nk_spos);
  }
  __device__ __forceinline__ T nbr(int e, int c = 0) const {
    if (!nk_edge_ok(e) || (unsigned)c >= (unsigned)NK_DOF) return T(NK_R(__builtin_nan("")));
    const int j = nk_col[e];
    return nk_lift<T>::at(nk_u[c * nk_nn + j], nk_v, c * nk_nn + j, c, nk_hot == e + (e >= nk_spos ? 1 : 0));
  }
  __device__ __forceinline__ int node(int e) const { return nk_edge_ok(e) ? nk_col[e] : -1; }
  __device__ __forceinline__ nk_real w(int e, int k = 0) const {
    if (!nk_edge_ok(e) || (unsigned)k >= (unsigned)NK_NEDGE) return NK_R(__builtin_nan(""));
    return nk_ew[(long)k * nk_ne + e];
  }
  __device__ __forceinline__ nk_real a(int k = 0) const {
    if ((unsigned)k >= (unsigned)NK_NNODE) return NK_R(__builtin_nan(""));
    return nk_nd[(long)k * nk_nn + nk_i];
  }
  __device__ __forceinline__ nk_real an(int e, int k = 0) const {
    if (!nk_edge_ok(e) || (unsigned)k >= (unsigned)NK_NNODE) return NK_R(__builtin_nan(""));
    return nk_nd[(long)k * nk_nn + nk_col[e]];
  }
};
)NKSRC";

static const char *k_graph_kernels = R"NKSRC(
// ---- generated kernels
// the graph as every kernel gets it: nn, ne, rowptr[nn + 1], colind[ne], then p, the edge data and the node data
#define NK_GRAPH_PARAMS int nn, int ne, const int *__restrict__ rowptr, const int *__restrict__ colind, \
                        const nk_real *__restrict__ p, const nk_real *__restrict__ ew, const nk_real *__restrict__ nd
template <typename T>
__device__ __forceinline__ nk_nbrs<T> nk_graph_view(int nn, int ne, const int *__restrict__ colind, const nk_real *__restrict__ ew,
                                                    const nk_real *__restrict__ nd, const nk_real *__restrict__ u,
                                                    const nk_real *__restrict__ v, int i, int e0, int dg, int spos, int hot) {
  nk_nbrs<T> nb;
  nb.nk_u = u, nb.nk_v = v, nb.nk_col = colind + e0, nb.nk_ew = ew + e0, nb.nk_nd = nd;
  nb.nk_nn = nn, nb.nk_ne = ne, nb.nk_i = i, nb.nk_dg = dg, nb.nk_spos = spos, nb.nk_hot = hot;
  return nb;
}

#if NK_GRAPH_SET == 0
extern "C" __global__ void __launch_bounds__(NK_GRAPH_BLOCK)
nk_graph_residual(NK_GRAPH_PARAMS, const nk_real *__restrict__ u, nk_real *__restrict__ f) {
  const int i = (int)blockIdx.x * NK_GRAPH_BLOCK + (int)threadIdx.x;
  if (i >= nn) return;
  const int e0 = rowptr[i], dg = rowptr[i + 1] - e0;
  const nk_nbrs<nk_real> nb = nk_graph_view<nk_real>(nn, ne, colind, ew, nd, u, nullptr, i, e0, dg, 0, -1);
  nk_real out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = NK_R(0);
  nk_node<nk_real>(nb, p, nk_vertex{i, nn, dg}, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) f[c * nn + i] = out[c];
}

// J(u)·v exactly: the value of every unknown from u, its one partial from v
extern "C" __global__ void __launch_bounds__(NK_GRAPH_BLOCK)
nk_graph_jvp(NK_GRAPH_PARAMS, const nk_real *__restrict__ u, const nk_real *__restrict__ v, nk_real *__restrict__ jv) {
  const int i = (int)blockIdx.x * NK_GRAPH_BLOCK + (int)threadIdx.x;
  if (i >= nn) return;
  const int e0 = rowptr[i], dg = rowptr[i + 1] - e0;
  const nk_nbrs<Dual> nb = nk_graph_view<Dual>(nn, ne, colind, ew, nd, u, v, i, e0, dg, 0, -1);
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  nk_node<Dual>(nb, p, nk_vertex{i, nn, dg}, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) jv[c * nn + i] = out[c].d[0];
}
#elif NK_GRAPH_FILL_NODE
// A/B form of the fill (NK_GRAPH_FILL_NODE=1 in the environment at creation): one NODE per thread with the slots in an inner
// loop — the same evaluations and the same stores, but a wavefront's stores are a row apart instead of consecutive
extern "C" __global__ void __launch_bounds__(NK_GRAPH_BLOCK)
nk_graph_jac(NK_GRAPH_PARAMS, const int *__restrict__ slotnode, const int *__restrict__ spos, const nk_real *__restrict__ u,
             nk_real *__restrict__ vals) {
  const int slots = ne + nn, i = (int)blockIdx.x * NK_GRAPH_BLOCK + (int)threadIdx.x;
  if (i >= nn) return;
  const int e0 = rowptr[i], dg = rowptr[i + 1] - e0, sp = spos[i];
  for (int s = 0; s <= dg; ++s) {
    const nk_nbrs<Dual> nb = nk_graph_view<Dual>(nn, ne, colind, ew, nd, u, nullptr, i, e0, dg, sp, s);
    Dual out[NK_DOF];
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
    nk_node<Dual>(nb, p, nk_vertex{i, nn, dg}, out);
#pragma unroll
    for (int c = 0; c < NK_DOF; ++c) {
#pragma unroll
      for (int c2 = 0; c2 < NK_DOF; ++c2) vals[c * NK_DOF * slots + NK_DOF * (e0 + i) + c2 * (dg + 1) + s] = out[c].d[c2];
    }
  }
}
#else
// The values of J(u) on the pattern: thread t takes global slot t = rowptr[i] + i + s of node i = slotnode[t], seeds the dof
// unknowns of slot s (self at s = spos[i], edge e at e + (e >= spos[i])) and stores dF_c(i)/du_c2(slot s) for all c, c2
extern "C" __global__ void __launch_bounds__(NK_GRAPH_BLOCK)
nk_graph_jac(NK_GRAPH_PARAMS, const int *__restrict__ slotnode, const int *__restrict__ spos, const nk_real *__restrict__ u,
             nk_real *__restrict__ vals) {
  const int slots = ne + nn;
  const unsigned tu = blockIdx.x * (unsigned)NK_GRAPH_BLOCK + threadIdx.x;
  if (tu >= (unsigned)slots) return;
  const int t = (int)tu, i = slotnode[t];
  const int e0 = rowptr[i], dg = rowptr[i + 1] - e0, s = t - (e0 + i);
  const nk_nbrs<Dual> nb = nk_graph_view<Dual>(nn, ne, colind, ew, nd, u, nullptr, i, e0, dg, spos[i], s);
  Dual out[NK_DOF];
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) out[c] = Dual(NK_R(0));
  nk_node<Dual>(nb, p, nk_vertex{i, nn, dg}, out);
#pragma unroll
  for (int c = 0; c < NK_DOF; ++c) {
#pragma unroll
    for (int c2 = 0; c2 < NK_DOF; ++c2) vals[c * NK_DOF * slots + NK_DOF * (e0 + i) + c2 * (dg + 1) + s] = out[c].d[c2];
  }
}
#endif
)NKSRC";

// what the user's source is held to, for the message of a source that does not compile
static const char *k_graph_contract =
    "the contract is `template <typename T> __device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f)` with "
    "u.self(c) the node's own unknown c, u.deg() its number of edges, u.nbr(e, c) unknown c of the e-th neighbour (e = 0..deg()-1), "
    "u.node(e) that neighbour's index, u.w(e, k) edge datum k, u.a(k) and u.an(e, k) node datum k of the node and of the neighbour "
    "(data are nk_real, never duals), s = {i, nn, deg}, p the parameters and f the node's dof residuals (nk_real = double)";

// ----------------------------------------------------------------------------- compilation
enum { GSET_F = 0 /* nk_graph_residual + nk_graph_jvp, NK_CH = 1 */, GSET_JAC = 1 /* nk_graph_jac, NK_CH = dof */ };

static int graph_check_counts(int dof, int np, int nedge, int nnode) {
  NK_REQUIRE(dof >= 1 && dof <= 4, "dof = %d outside 1..4 (components per node)", dof);
  NK_REQUIRE(np >= 0 && np <= 32, "nparams = %d outside 0..32", np);
  NK_REQUIRE(nedge >= 0 && nedge <= 4, "nedge = %d outside 0..4 (data arrays of one double per edge)", nedge);
  NK_REQUIRE(nnode >= 0 && nnode <= 4, "nnode = %d outside 0..4 (data arrays of one double per node)", nnode);
  return NK_OK;
}

// A/B switch: the fill runs one node per thread with an inner slot loop (tools/graph_problem_bench.py measures both forms;
// read at every create, so one process can build both)
static bool graph_fill_node() {
  const char *e = getenv("NK_GRAPH_FILL_NODE");
  return e != nullptr && atoi(e) != 0;
}

static int graph_compile(const char *source, int dof, int np, int nedge, int nnode, int gset, bool fill_node, std::vector<char> *code,
                         std::string *log) {
  NK_REQUIRE(source, "NULL source");
  NK_TRY(graph_check_counts(dof, np, nedge, nnode));
  const std::string full = std::string(nk_dual_prelude) + nk_seed_lift + k_graph_types + "\n// ---- user source\n" + source + "\n" +
                           k_graph_kernels;
  const std::vector<std::string> defs = {
      "-DNK_DOF=" + std::to_string(dof), "-DNK_NEDGE=" + std::to_string(nedge), "-DNK_NNODE=" + std::to_string(nnode),
      "-DNK_CH=" + std::to_string(gset == GSET_JAC ? dof : 1), "-DNK_GRAPH_SET=" + std::to_string(gset),
      "-DNK_SEED_SET=" + std::to_string(gset), std::string("-DNK_GRAPH_FILL_NODE=") + (fill_node ? "1" : "0")};
  return nk_rtc_program(full, "nk_graph_user.hip", defs, source, "graph", k_graph_contract, code, log);
}

// compile only (no device needed): both programs
extern "C" int nk_graph_compile_check(const char *source, int dof, int nparams, int nedge, int nnode, int64_t *code_bytes) {
  std::vector<char> code;
  std::string log;
  int64_t total = 0;
  for (int gset : {GSET_F, GSET_JAC}) {
    log.clear();
    NK_TRY(graph_compile(source, dof, nparams, nedge, nnode, gset, graph_fill_node(), &code, &log));
    total += (int64_t)code.size();
  }
  if (code_bytes) *code_bytes = total;
  return NK_OK;
}

// the code object of one program (jac = 0: the residual and JVP kernels; 1: the Jacobian fill) for inspection
extern "C" int nk_graph_code_object(const char *source, int dof, int nparams, int nedge, int nnode, int jac, void *buf,
                                    int64_t capacity, int64_t *bytes) {
  NK_REQUIRE(bytes, "NULL argument");
  std::vector<char> code;
  std::string log;
  NK_TRY(graph_compile(source, dof, nparams, nedge, nnode, jac != 0 ? GSET_JAC : GSET_F, graph_fill_node(), &code, &log));
  return nk_rtc_copy_out(code, buf, capacity, bytes);
}

// ----------------------------------------------------------------------------- the problem object
struct nk_graph_state {
  nk_compiled c;   // the context, the programs, p and the pattern
  int nn = 0, ne = 0, dof = 0, nedge = 0, nnode = 0;
  bool fill_node = false;   // the fill was compiled in its A/B form: one node per thread
  int32_t *d_rowptr = nullptr, *d_colind = nullptr;   // the adjacency
  int32_t *d_slotnode = nullptr, *d_spos = nullptr;   // the node of every global slot (ne + nn); the self slot of every node (nn)
  double *d_edge = nullptr;     // nedge·ne doubles, datum k of edge e at k·ne + e (at least one allocated); zero at creation
  double *d_node = nullptr;     // nnode·nn doubles, datum k of node i at k·nn + i (at least one allocated); zero at creation
};

void nk_graph_state_destroy(nk_graph_state *S) {
  if (!S) return;
  nk_compiled_free(&S->c);
  hipFree(S->d_rowptr);
  hipFree(S->d_colind);
  hipFree(S->d_slotnode);
  hipFree(S->d_spos);
  hipFree(S->d_edge);
  hipFree(S->d_node);
  delete S;
}

// One launch of a generated kernel over `items` threads on `stream`: the graph and what the problem owns, then `rest`
static int graph_launch(nk_graph_state *S, hipFunction_t fn, int64_t items, std::initializer_list<void *> rest, void *stream) {
  void *args[12] = {&S->nn, &S->ne, &S->d_rowptr, &S->d_colind, &S->c.d_params, &S->d_edge, &S->d_node};
  int n = 7;
  for (void *a : rest) args[n++] = a;
  return nk_compiled_launch(&S->c, fn, items, args, stream);
}
static int graph_cb_residual(void *user, const double *u, double *f, void *stream) {
  nk_graph_state *S = (nk_graph_state *)user;
  return graph_launch(S, S->c.fn_res, S->nn, {&u, &f}, stream);
}
static int graph_cb_jvp(void *user, const double *v, const double *u, double *jv, void *stream) {
  nk_graph_state *S = (nk_graph_state *)user;
  return graph_launch(S, S->c.fn_jvp, S->nn, {&u, &v, &jv}, stream);
}
static int graph_cb_jac(void *user, const double *u, double *vals, void *stream) {
  nk_graph_state *S = (nk_graph_state *)user;
  return graph_launch(S, S->c.fn_jac, S->fill_node ? (int64_t)S->nn : (int64_t)S->ne + S->nn, {&S->d_slotnode, &S->d_spos, &u, &vals}, stream);
}

// datum k of the edges or of the nodes: its doubles on the device
static int graph_data_ptr(nk_problem *P, int on_edges, int k, double **d, size_t *bytes) {
  NK_REQUIRE(P, "NULL argument");
  NK_REQUIRE(P->graph, "the problem is not a compiled graph problem (kind %d): it has no edge or node data", (int)P->kind);
  nk_graph_state *S = P->graph;
  const int cnt = on_edges ? S->nedge : S->nnode;
  NK_REQUIRE(k >= 0 && k < cnt, "%s datum k = %d outside 0..%d (the problem was created with %s = %d)", on_edges ? "edge" : "node", k,
             cnt - 1, on_edges ? "nedge" : "nnode", cnt);
  const size_t len = on_edges ? (size_t)S->ne : (size_t)S->nn;
  *d = (on_edges ? S->d_edge : S->d_node) + (size_t)k * len;
  *bytes = len * sizeof(double);
  return NK_OK;
}
extern "C" int nk_problem_set_graph_data(nk_problem *P, int on_edges, int k, const double *data, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(graph_data_ptr(P, on_edges, k, &d, &bytes));
  NK_TRY(nk_compiled_data_copy(P, d, bytes, data, memspace, true));
  nk_compiled_data_changed(P);
  return NK_OK;
}
extern "C" int nk_problem_get_graph_data(nk_problem *P, int on_edges, int k, double *out, int memspace) {
  double *d = nullptr;
  size_t bytes = 0;
  NK_TRY(graph_data_ptr(P, on_edges, k, &d, &bytes));
  return nk_compiled_data_copy(P, d, bytes, out, memspace, false);
}

extern "C" int nk_problem_create_graph(nk_ctx *ctx, const char *source, int64_t nn, const int32_t *rowptr, const int32_t *colind,
                                       int dof, const double *params, int nparams, int nedge, int nnode, nk_problem **out) {
  NK_REQUIRE(ctx && source && out, "NULL argument");
  NK_REQUIRE(params || nparams == 0, "NULL params with nparams = %d", nparams);
  // the adjacency and the counts first: every refusal comes before anything is compiled or allocated
  int64_t ne = 0;
  NK_TRY(graph_validate(nn, rowptr, colind, dof, &ne));
  NK_TRY(graph_check_counts(dof, nparams, nedge, nnode));
  if (ctx->nranks > 1)
    NK_FAIL(NK_E_UNSUPPORTED, "a compiled graph problem runs on one rank, the context has %d (partitioning an arbitrary graph is "
            "not built)", ctx->nranks);
  NK_HIP(hipSetDevice(ctx->device));
  std::vector<char> code_f, code_j;
  std::string log;
  NK_TRY(graph_compile(source, dof, nparams, nedge, nnode, GSET_F, false, &code_f, &log));
  log.clear();
  const bool fill_node = graph_fill_node();
  NK_TRY(graph_compile(source, dof, nparams, nedge, nnode, GSET_JAC, fill_node, &code_j, &log));

  const int64_t slots = ne + nn, n = nn * dof, nnz = (int64_t)dof * dof * slots;
  std::vector<int32_t> rp((size_t)n + 1), slotnode, spos;
  std::vector<int64_t> gc((size_t)nnz);
  graph_pattern_fill<int64_t>(nn, ne, rowptr, colind, dof, rp.data(), gc.data());
  nk_graph_slots(nn, rowptr, colind, &slotnode, &spos);

  nk_graph_state *S = new nk_graph_state();
  auto guard = nk_make_guard(S, nk_graph_state_destroy);
  S->c.ctx = ctx;
  S->nn = (int)nn;
  S->ne = (int)ne;
  S->dof = dof;
  S->nedge = nedge;
  S->nnode = nnode;
  S->fill_node = fill_node;
  NK_TRY(nk_compiled_load(&S->c, code_f, code_j, "nk_graph_residual", "nk_graph_jvp", "nk_graph_jac", "graph"));
  NK_TRY(nk_upload(ctx, &S->d_rowptr, std::vector<int32_t>(rowptr, rowptr + nn + 1)));
  NK_TRY(nk_upload(ctx, &S->d_colind, std::vector<int32_t>(colind, colind + ne)));
  NK_TRY(nk_upload(ctx, &S->d_slotnode, slotnode));
  NK_TRY(nk_upload(ctx, &S->d_spos, spos));
  NK_TRY(nk_compiled_params_init(&S->c, params, nparams));
  NK_TRY(nk_compiled_zeros(ctx, &S->d_edge, (size_t)nedge * (size_t)ne));   // zero until nk_problem_set_graph_data
  NK_TRY(nk_compiled_zeros(ctx, &S->d_node, (size_t)nnode * (size_t)nn));
  NK_TRY(nk_csr_create_local(ctx, n, n, 0, rp, gc, nullptr, &S->c.pattern));
  NK_TRY(nk_compiled_problem(&S->c, n, n, 0, params, nparams, {graph_cb_residual, graph_cb_jvp, nullptr, graph_cb_jac}, S, out));
  (*out)->graph = guard.release();
  return NK_OK;
}
