"""The geometric multigrid `precs` of compiled grid problems without a GPU: the library's axis tables (nk_grid_mg_axis, host
only) against the NumPy restatement tests/gridmg_reference.py, the properties of the transfers, and the restatement's own
mesh-independent GMRES counts."""
import numpy as np
import pytest

import gridmg_reference as GM

AXIS_SIZES = (5, 6, 7, 8, 9, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("lo,hi", GM.SIDE_PAIRS)
def test_axis_tables_match_the_restatement(lo, hi):
    """all 10 side pairs × 10 sizes: nc and the indices exactly, the weights to 1e-14"""
    import nonlinearsolve_jl_amd as nls
    for n in AXIS_SIZES:
        nc, idx, w = nls.grid_mg_axis(n, lo, hi)
        rnc, ridx, rw = GM.axis_table(n, lo, hi)
        assert nc == rnc, (n, nc, rnc)
        assert np.array_equal(idx, ridx), (n, idx, ridx)
        assert np.max(np.abs(w - rw)) <= 1e-14, (n, np.max(np.abs(w - rw)))


@pytest.mark.parametrize("lo,hi", GM.SIDE_PAIRS)
def test_axis_table_properties(lo, hi):
    """restriction rows sum to 1; prolongation rows sum to 1 except where a Dirichlet ghost was dropped; without a Dirichlet
    side the prolongation reproduces a constant; the coarse axis follows the geometry"""
    import nonlinearsolve_jl_amd as nls
    for n in AXIS_SIZES:
        nc, idx, w = nls.grid_mg_axis(n, lo, hi)
        assert np.all((idx >= -1) & (idx < nc)) and np.all(w[idx < 0] == 0.0) and np.all(w[idx >= 0] > 0.0)
        rows, cols = np.nonzero(idx >= 0)
        P = np.zeros((n, nc))
        np.add.at(P, (rows, idx[rows, cols]), w[rows, cols])
        Rm = P.T / P.T.sum(axis=1, keepdims=True)
        assert np.max(np.abs(Rm.sum(axis=1) - 1.0)) <= 1e-14
        rs = P.sum(axis=1)
        a = GM.OFFSET[lo] + GM.OFFSET[hi]
        L = n if lo == "periodic" else n - 1 + a
        Lc = nc if lo == "periodic" else nc - 1 + a
        # a row lost weight only where its interval reaches past a Dirichlet wall's first ghost: the nodes nearer to the
        # wall than one coarse spacing
        pos = np.arange(n) if lo == "periodic" else GM.OFFSET[lo] + np.arange(n)
        H = L / Lc
        near = np.zeros(n, dtype=bool)
        if lo == "dirichlet":
            near |= pos < H - 1e-9
        if hi == "dirichlet":
            near |= (L - pos) < H - 1e-9
        assert np.max(np.abs(rs[~near] - 1.0)) <= 1e-14, (n, rs)
        assert np.all(rs[near] < 1.0) and np.all(rs > 0.0)
        if "dirichlet" not in (lo, hi):
            assert np.max(np.abs(P @ np.ones(nc) - 1.0)) <= 1e-14
        assert 2 <= nc < n and abs(H - 2.0) <= 2.0 / Lc + 1e-12      # the coarse spacing is two fine ones, up to the rounding of nc


def test_axis_errors():
    import nonlinearsolve_jl_amd as nls
    with pytest.raises(nls.NKError, match="wraps as a whole"):
        nls.grid_mg_axis(9, "periodic", "dirichlet")
    with pytest.raises(ValueError):
        nls.grid_mg_axis(9, "dirichlet", "neumann")
    with pytest.raises(nls.NKError):
        nls.grid_mg_axis(2, "dirichlet", "dirichlet")


def test_level_shapes_stop_at_the_stencil_side_and_at_coarse_max():
    assert GM.level_shapes((21, 21), ("dirichlet",) * 4, 2, 4) == [(21, 21), (10, 10), (5, 5)]       # radius 2: nc = 2 < 5
    assert GM.level_shapes((33, 32), ("dirichlet",) * 4, 1, 4) == [(33, 32), (16, 16), (8, 8), (4, 4)]
    assert GM.level_shapes((12, 9), ("periodic",) * 4, 1, 5) == [(12, 9), (6, 5), (3, 5)]
    # one axis already at coarse_max keeps its side while the other goes on
    assert GM.level_shapes((40, 5), ("mirror_node",) * 4, 1, 5) == [(40, 5), (21, 5), (11, 5), (6, 5), (4, 5)]


def test_transfers_are_tensor_products_with_unit_restriction_rows():
    prob = GM.PROBLEMS["star3"]
    fine, coarse = (9, 10, 12), (4, 5, 6)
    P, Rm = GM.transfers(fine, coarse, prob.boundary)
    assert P.shape == (9 * 10 * 12, 4 * 5 * 6) and Rm.shape == P.shape[::-1]
    assert np.max(np.abs(np.asarray(Rm.sum(axis=1)).ravel() - 1.0)) <= 1e-14
    # the z axis is mirrored: a function of z alone that is constant is reproduced along z (x, y Dirichlet lose weight at the walls)
    Pz = GM.axis_prolongation(12, "mirror_face", "mirror_face")
    assert np.max(np.abs(Pz @ np.ones(6) - 1.0)) <= 1e-14


# the restatement's own GMRES(30) counts to rtol 1e-9 with its V-cycle as M (ν = 2, coarse_max = 8) at three sizes
COUNTS = {
    "bratu": {(33, 32): 7, (65, 64): 8, (129, 128): 8},
    "channel": {(32, 33): 7, (64, 65): 7, (128, 129): 7},
    "mixed": {(33, 28): 8, (65, 56): 8, (129, 112): 8},
    "coupled": {(32, 32): 7, (64, 64): 7, (128, 128): 7},
    "star3": {(9, 10, 12): 8, (17, 18, 20): 8, (33, 34, 36): 8},
    "fourth": {(33, 33): 8, (65, 65): 9, (129, 129): 9},
}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_reference_counts_are_mesh_independent(name):
    sizes = sorted(COUNTS[name], key=lambda s: int(np.prod(s)))
    got = {}
    for shape in sizes:
        ref = GM.reference(name, shape, 8)
        got[shape] = ref.iters
        assert np.linalg.norm(ref.J @ ref.x - ref.b) <= 1.01e-9 * np.linalg.norm(ref.b)
    print(name, got)
    assert got == COUNTS[name]
    assert got[sizes[-1]] - got[sizes[0]] <= 3


@pytest.mark.parametrize("name", sorted(GM.PROBLEMS))
def test_reference_jacobian_is_the_derivative_of_its_residual(name):
    """the NumPy problems themselves: J(u) v against a central difference of the residual"""
    prob = GM.PROBLEMS[name]
    shape = (7, 6, 5) if prob.dim == 3 else (9, 7)
    u = GM.linearisation_point(prob, shape)
    fields = prob.fields(shape)
    v = np.random.default_rng(3).standard_normal(u.size)
    J = prob.jac(shape, u, fields)
    eps = 1e-6
    fd = (prob.residual(shape, u + eps * v, fields) - prob.residual(shape, u - eps * v, fields)) / (2 * eps)
    assert np.max(np.abs(J @ v - fd)) <= 1e-6 * np.max(np.abs(fd))


@pytest.mark.parametrize("name", sorted(GM.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    prob = GM.PROBLEMS[name]
    assert nls.grid_compile_check(prob.source, prob.dof, prob.stencil, prob.boundary, len(prob.params), dim=prob.dim,
                                  fields=prob.nfields) > 1000
