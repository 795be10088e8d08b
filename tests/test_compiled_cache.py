"""The cache of run-time compiled programs, without a GPU (hiprtc runs on the host): the same program fetched twice is the same
bytes, a program that differs in one option only is another program, and two problem kinds never hand out each other's program
— not even for one and the same source text."""
import ctypes as C

import graph_reference as GR
from nonlinearsolve_jl_amd import _lib as L


def _fetch(fn, *args):
    nb = C.c_int64()
    assert fn(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert fn(*args, buf, nb.value, C.byref(nb)) == 0, L.lib().nk_last_error()
    return buf.raw[:nb.value]


def _graph(src, dof, nparams, nedge, nnode, jac):
    return _fetch(L.lib().nk_graph_code_object, src.encode(), dof, nparams, nedge, nnode, jac)


def _elem(src, npe, dof, nparams, nnode, nelem, jac):
    return _fetch(L.lib().nk_elem_code_object, src.encode(), npe, dof, nparams, nnode, nelem, jac)


def test_the_same_program_twice_is_the_same_bytes():
    p = GR.PROBLEMS["sink"]
    for jac in (0, 1):
        a = _graph(p.source, p.dof, len(p.params), p.nedge, p.nnode, jac)
        assert a[:4] == b"\x7fELF" and a == _graph(p.source, p.dof, len(p.params), p.nedge, p.nnode, jac)
    # and the two programs of one source are not each other
    assert _graph(p.source, p.dof, len(p.params), p.nedge, p.nnode, 0) != _graph(p.source, p.dof, len(p.params), p.nedge, p.nnode, 1)


# reads edge datum 0: with nedge = 0 that read is the constant NaN, with nedge = 1 a load — two programs of one text
EDGE_DATUM_SRC = r"""
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  T acc = u.self();
  for (int e = 0; e < u.deg(); ++e) acc = acc + u.w(e, 0) * u.nbr(e);
  f[0] = acc;
}
"""


def test_one_option_apart_is_another_program():
    for jac in (0, 1):
        with_datum = _graph(EDGE_DATUM_SRC, 1, 0, 1, 0, jac)
        without = _graph(EDGE_DATUM_SRC, 1, 0, 0, 0, jac)
        assert with_datum != without
        # in whatever order they were asked for first, each is still itself
        assert _graph(EDGE_DATUM_SRC, 1, 0, 0, 0, jac) == without and _graph(EDGE_DATUM_SRC, 1, 0, 1, 0, jac) == with_datum


# One text that is a graph source and an element source at once: the neighbourhood and the site are template parameters, so
# nk_node<T>(…) of the graph kernels and nk_element<T>(…) of the element kernels both find their function in it
BOTH_KINDS_SRC = r"""
template <typename T, typename U, typename S>
__device__ void nk_node(const U &u, const nk_real *p, S s, T *f) { f[0] = T(p[0]); }
template <typename T, typename U, typename S>
__device__ void nk_element(const U &u, const nk_real *p, S s, T *f) { f[0] = T(p[0]); }
"""
NODE_ONLY_SRC = r"""
template <typename T, typename U, typename S>
__device__ void nk_node(const U &u, const nk_real *p, S s, T *f) { f[0] = T(p[0]); }
"""
GRAPH_KERNELS = {0: (b"nk_graph_residual", b"nk_graph_jvp"), 1: (b"nk_graph_jac",)}
ELEM_KERNELS = {0: (b"nk_elem_residual", b"nk_elem_jvp"), 1: (b"nk_elem_jac",)}


def _assert_kind(code, own, other):
    assert code[:4] == b"\x7fELF"
    assert all(k in code for k in own) and not any(k in code for k in other)


def test_two_kinds_never_share_a_program():
    # the same text, and the counts both kinds have (dof, nparams, nnode) the same
    for jac in (0, 1):
        g = _graph(BOTH_KINDS_SRC, 1, 1, 0, 0, jac)
        e = _elem(BOTH_KINDS_SRC, 2, 1, 1, 0, 0, jac)
        _assert_kind(g, GRAPH_KERNELS[jac], ELEM_KERNELS[jac])
        _assert_kind(e, ELEM_KERNELS[jac], GRAPH_KERNELS[jac])
        # both are cached now: asked again, in the other order, each kind gets its own
        assert _elem(BOTH_KINDS_SRC, 2, 1, 1, 0, 0, jac) == e and _graph(BOTH_KINDS_SRC, 1, 1, 0, 0, jac) == g
    # texts that differ in the function's name only
    node_src = NODE_ONLY_SRC
    elem_src = node_src.replace("nk_node", "nk_element")
    assert node_src != elem_src and node_src.replace("nk_node", "") == elem_src.replace("nk_element", "")
    _assert_kind(_graph(node_src, 1, 1, 0, 0, 0), GRAPH_KERNELS[0], ELEM_KERNELS[0])
    _assert_kind(_elem(elem_src, 2, 1, 1, 0, 0, 0), ELEM_KERNELS[0], GRAPH_KERNELS[0])
    _assert_kind(_graph(node_src, 1, 1, 0, 0, 0), GRAPH_KERNELS[0], ELEM_KERNELS[0])
