"""The table of the compiled graph problems' tests: the graphs, and every problem as HIP source beside the same formula in NumPy
(tests/graph_core.py runs the formula on arrays with the device's dual-number rules, and node by node on scalars).

Graphs
    single      nn = 1, ne = 0
    directed3   edges 0→1 and 2→1 only: one node of degree 0, structurally nonsymmetric
    tri(...)    a grid's 4 neighbours plus one random diagonal per cell, symmetric, degrees 2–8: 6×5 natural; 9×7, 17×15
                (nn = 255) and 16×16 (nn = 256, the workgroup edge) randomly renumbered
    ring257     the self slot is first at node 0, last at node 256 and in the middle elsewhere; one node past a workgroup
    hub301      node 150 joined to all 300 others, which also form a ring: a degree above 256 and above a wavefront, the self
                slot inside a long row, the fill's slots of one node across several workgroups

Problems
    sink        dof 1; edge datum w; node data κ, m; p = (p0, p1):  Σ w(u_i − u_j) + κ_i u_i + p0 m_i exp(u_i) − p1
    cubic       dof 1; edge datum w; node data κ, s; p = (p0,):     Σ w(d + p0 d³) + κ_i u_i − s_i,  d = u_i − u_j
    powerflow   dof 2 = (θ, V); edge data g, b; node data P, Q, slack flag:
                F_θ = Σ[g V_i² − V_i V_j (g cos d + b sin d)] − P_i,  F_V = Σ[−b V_i² − V_i V_j (g sin d − b cos d)] − Q_i,
                d = θ_i − θ_j; a slack node has F = (θ, V − 1)
    indexed     dof 1, no data; uses u.node(e), s.i, s.deg, s.nn (on directed3 and hub301)
    react4      dof 4, each component coupled to the next: u_c·u_{(c+1)%4}, on the node and across the edges

Data ranges (kept from the issue): w ∈ [0.5, 1.5], κ ∈ [0.05, 0.15], m ∈ [0.5, 1], s ∈ [−1, 1], p = (0.5, 1) for sink and
p0 = 2 for cubic, g ∈ [0.5, 1.5], b ∈ [−8, −4], P ∈ [−0.3, 0.3], Q ∈ [−0.1, 0.1], node 0 slack."""
import graph_core as GC
from graph_core import Problem, gcos, gexp, gsin

# ------------------------------------------------------------------------------------------------ graphs
GRAPHS = {g.name: g for g in (GC.single(), GC.directed3(), GC.ring(257), GC.hub(301, 150))}
GRAPHS["tri6x5"] = GC.tri(6, 5, 1, False)
GRAPHS["tri9x7p"] = GC.tri(9, 7, 1, True)
GRAPHS["tri17x15p"] = GC.tri(17, 15, 1, True)
GRAPHS["tri16x16p"] = GC.tri(16, 16, 1, True)

# ------------------------------------------------------------------------------------------------ sink
SINK_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  const T ui = u.self();
  T acc = T(0.0);
  for (int e = 0; e < u.deg(); ++e) acc = acc + u.w(e) * (ui - u.nbr(e));
  f[0] = acc + u.a(0) * ui + (p[0] * u.a(1)) * exp(ui) - p[1];
}
"""


def _sink(u, p, s):
    ui = u.self()
    acc = u.zero()
    for e in u.edges():
        acc = u.add(e, acc, u.w(e) * (ui - u.nbr(e)))
    return [acc + u.a(0) * ui + (p[0] * u.a(1)) * gexp(ui) - p[1]]


# ------------------------------------------------------------------------------------------------ cubic
CUBIC_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  const T ui = u.self();
  T acc = T(0.0);
  for (int e = 0; e < u.deg(); ++e) {
    const T d = ui - u.nbr(e);
    acc = acc + u.w(e) * (d + p[0] * (d * d * d));
  }
  f[0] = acc + u.a(0) * ui - u.a(1);
}
"""


def _cubic(u, p, s):
    ui = u.self()
    acc = u.zero()
    for e in u.edges():
        d = ui - u.nbr(e)
        acc = u.add(e, acc, u.w(e) * (d + p[0] * (d * d * d)))
    return [acc + u.a(0) * ui - u.a(1)]


# ------------------------------------------------------------------------------------------------ AC power flow
POWERFLOW_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  const T th = u.self(0), V = u.self(1);
  T fp = T(0.0), fq = T(0.0);
  for (int e = 0; e < u.deg(); ++e) {
    const nk_real g = u.w(e, 0), b = u.w(e, 1);
    const T d = th - u.nbr(e, 0), VV = V * u.nbr(e, 1), c = cos(d), sn = sin(d);
    fp = fp + (g * (V * V) - VV * (g * c + b * sn));
    fq = fq + ((-b) * (V * V) - VV * (g * sn - b * c));
  }
  const bool slack = u.a(2) != 0.0;
  f[0] = slack ? th : fp - u.a(0);
  f[1] = slack ? V - 1.0 : fq - u.a(1);
}
"""


def _powerflow(u, p, s):
    th, V = u.self(0), u.self(1)
    fp, fq = u.zero(), u.zero()
    for e in u.edges():
        g, b = u.w(e, 0), u.w(e, 1)
        d, VV = th - u.nbr(e, 0), V * u.nbr(e, 1)
        c, sn = gcos(d), gsin(d)
        fp = u.add(e, fp, g * (V * V) - VV * (g * c + b * sn))
        fq = u.add(e, fq, (-b) * (V * V) - VV * (g * sn - b * c))
    slack = u.a(2) != 0.0
    return [u.where(slack, th, fp - u.a(0)), u.where(slack, V - 1.0, fq - u.a(1))]


# ------------------------------------------------------------------------------------------------ indexed
INDEXED_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  const T ui = u.self();
  T acc = T(0.0);
  for (int e = 0; e < u.deg(); ++e) {
    const nk_real c = (nk_real)(1 + u.node(e)) / (nk_real)(1 + s.i + s.nn);
    acc = acc + c * (ui * u.nbr(e));
  }
  f[0] = acc + (nk_real)(s.deg + 1) * ui - (nk_real)s.i / (nk_real)s.nn;
}
"""


def _indexed(u, p, s):
    ui = u.self()
    acc = u.zero()
    for e in u.edges():
        c = u.real(1 + u.node(e)) / u.real(1 + s.i + s.nn)
        acc = u.add(e, acc, c * (ui * u.nbr(e)))
    return [acc + u.real(s.deg + 1) * ui - u.real(s.i) / u.real(s.nn)]


# ------------------------------------------------------------------------------------------------ react4
REACT4_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = (c + 1) % 4;
    const T uc = u.self(c);
    T acc = T(0.0);
    for (int e = 0; e < u.deg(); ++e) acc = acc + (uc - u.nbr(e, c)) * u.nbr(e, n);
    f[c] = acc + uc * u.self(n) + p[0] * uc - 1.0;
  }
}
"""


def _react4(u, p, s):
    out = []
    for c in range(4):
        n = (c + 1) % 4
        uc = u.self(c)
        acc = u.zero()
        for e in u.edges():
            acc = u.add(e, acc, (uc - u.nbr(e, c)) * u.nbr(e, n))
        out.append(acc + uc * u.self(n) + p[0] * uc - 1.0)
    return out


# ------------------------------------------------------------------------------------------------ the table
W_RANGE, KAPPA, MASS, SOURCE = (0.5, 1.5), (0.05, 0.15), (0.5, 1.0), (-1.0, 1.0)
PROBLEMS = {
    "sink": Problem("sink", SINK_SRC, 1, [0.5, 1.0], _sink, [W_RANGE], [KAPPA, MASS]),
    "cubic": Problem("cubic", CUBIC_SRC, 1, [2.0], _cubic, [W_RANGE], [KAPPA, SOURCE]),
    "powerflow": Problem("powerflow", POWERFLOW_SRC, 2, [], _powerflow, [(0.5, 1.5), (-8.0, -4.0)],
                         [(-0.3, 0.3), (-0.1, 0.1), "slack"]),
    "indexed": Problem("indexed", INDEXED_SRC, 1, [], _indexed),
    "react4": Problem("react4", REACT4_SRC, 4, [1.5], _react4),
}
CASES = [(p, g) for p in ("sink", "cubic", "powerflow", "react4") for g in sorted(GRAPHS)] + \
        [("indexed", "directed3"), ("indexed", "hub301")]

# a source written against the grid contract, and one that does not parse
GRID_CONTRACT_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) { f[0] = u(0, 0); }
"""
SYNTAX_ERROR_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) { f[0] = no_such_symbol(u.self()); }
"""
# reads an edge datum and a node datum beyond the declared count
UNDECLARED_DATA_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) { f[0] = u.self() + u.a(1); }
"""
