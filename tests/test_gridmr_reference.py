"""Compiled grid problems on several ranks, without a GPU: nk_grid_slab_pattern against the restatement
tests/gridmr_reference.py for every rank of 1..4 (every stencil of both dimensions, dof 1, 2 and 4 where offered, the five kinds
of the split axis, the x axis periodic and mirrored), the union of the ranks' patterns against the one-rank nk_grid_pattern, one
rank against nk_grid_pattern and nk_partition_range, the refusal of a slab thinner than radius + 1 lines, the programs of every
kind of rank through nk_grid_slab_compile_check for gfx950 with no private segment in their code objects, and the one-rank
programs unchanged: nk_grid_slab_code_object(nranks = 1) returns the bytes of the three older entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_core as GC
import grid_reference as G1
import gridf_reference as GF
import gridmr_reference as R
import nonlinearsolve_jl_amd as nls
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
KERNELS = {2: {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)},
           3: {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}}
MN, MF, DI, PE = R.MN, R.MF, R.DI, R.PE
# (dim, stencil, dof): every stencil the table offers, dof 1, 2 and 4 where allowed
_STENCILS = [(2, "star", 1), (2, "star", 2), (2, "star", 4), (2, "box", 1), (2, "box", 2), (2, "star2", 1), (2, "star2", 2),
             (2, "diamond2", 1), (3, "star", 1), (3, "star", 2), (3, "star", 4), (3, "box", 1), (3, "star2", 1), (3, "star2", 2)]
_OUTER = [(DI, DI), (PE, PE), (MN, MN), (MF, MF), (MF, DI)]
_XKINDS = [(PE, PE), (MF, MN)]


def _shape(dim, stencil, nranks):
    """the smallest shape that splits into legal slabs: 4 × 5 | 5 × 7 for two ranks, 3–5 nodes on the other axes in 3-D"""
    rad = R.RADIUS[stencil]
    n_outer = {1: 2 * rad + 1, 2: 2 * rad + 3, 3: 7 if rad == 1 else 9}.get(nranks, (rad + 1) * nranks)
    inner = ((4, 3) if rad == 1 else (5, 5)) if dim == 3 else ((4,) if rad == 1 else (5,))
    return inner + (n_outer,)


def _sides(dim, xk, ok):
    return xk + ((DI, MN) if dim == 3 else ()) + ok


def _device_pattern(shape, dof, stencil, sides, nranks, rank):
    return nls.grid_slab_pattern(shape[0], shape[1], dof, stencil, sides, nz=shape[2] if len(shape) == 3 else None,
                                 nranks=nranks, rank=rank)


@pytest.mark.parametrize("dim,stencil,dof", _STENCILS, ids=[f"{d}d-{s}-dof{k}" for d, s, k in _STENCILS])
def test_slab_pattern_parity_and_union(dim, stencil, dof):
    """every rank of R = 1..4: lines, rowptr and the global columns equal the restatement's (the permuted one-rank pattern's rows,
    columns renumbered and sorted); then the union check — the library's own slab patterns mapped back through the permutation
    give exactly the one-rank nk_grid_pattern, which catches every zone-order and wrap mistake"""
    offs = GC.STENCILS[(dim, stencil)]
    for nranks in (1, 2, 3, 4):
        shape = _shape(dim, stencil, nranks)
        for xk in _XKINDS:
            for ok in _OUTER:
                sides = _sides(dim, xk, ok)
                got = []
                for rank in range(nranks):
                    S = R.Slab(shape, dof, offs, sides, nranks, rank)
                    lines, rp, ci = _device_pattern(shape, dof, stencil, sides, nranks, rank)
                    tag = (shape, sides, nranks, rank)
                    assert lines == S.lines, tag
                    assert rp.dtype == np.int32 and ci.dtype == np.int64
                    assert np.array_equal(rp, S.rowptr), tag
                    assert np.array_equal(ci, S.colind), tag
                    assert all(np.all(np.diff(ci[rp[t]:rp[t + 1]]) > 0) for t in range(rp.size - 1)), tag
                    S.rowptr, S.colind = rp, ci          # (the union below is of what the library returned)
                    got.append(S)
                urp, uci = R.union_pattern(got)
                frp, fci = nls.grid_pattern(shape[0], shape[1], dof, stencil, sides, nz=shape[2] if dim == 3 else None)
                assert np.array_equal(urp, frp) and np.array_equal(uci, fci), (shape, sides, nranks)


def test_the_restatement_s_permutation_and_ranges():
    """written out: 7 lines over 3 ranks are 2|2|3, and the rank-contiguous order of a 2 × 3 grid at dof 2 over 2 ranks (slabs of
    1 and 2 lines): rank 0's component 0, its component 1, then rank 1's"""
    assert R.slab_ranges(7, 3) == [(0, 2), (2, 4), (4, 7)] and R.slab_ranges(5, 2) == [(0, 2), (2, 5)]
    assert list(R.permutation((2, 3), 2, 2)) == [0, 1, 6, 7, 2, 3, 4, 5, 8, 9, 10, 11]
    for nranks in (1, 2, 3, 4):
        for r, (a, b) in enumerate(R.slab_ranges(9, nranks)):
            assert (a, b) == tuple(nls.partition_range(9, 1, nranks, r))
    # the core helpers agree with the restatement
    assert np.array_equal(nls.core._slab_permutation(4, 3, 5, 2, 2), R.permutation((4, 3, 5), 2, 2))
    assert np.array_equal(nls.core._slab_permutation(4, 7, None, 2, 3), R.permutation((4, 7), 2, 3))


@pytest.mark.parametrize("dim,stencil", [(2, "star"), (2, "diamond2"), (3, "box"), (3, "star2")])
def test_one_rank_is_grid_pattern(dim, stencil):
    shape = _shape(dim, stencil, 2)
    for sides in (_sides(dim, (PE, PE), (PE, PE)), _sides(dim, (MF, MN), (MF, DI))):
        lines, rp, ci = _device_pattern(shape, 1, stencil, sides, 1, 0)
        frp, fci = nls.grid_pattern(shape[0], shape[1], 1, stencil, sides, nz=shape[2] if dim == 3 else None)
        assert lines == tuple(nls.partition_range(shape[-1], 1, 1, 0)) == (0, shape[-1])
        assert np.array_equal(rp, frp) and np.array_equal(ci, fci.astype(np.int64))


def test_a_thin_slab_is_refused_with_the_numbers():
    """every slab holds at least radius + 1 lines: NK_E_INVALID naming n_outer, R, the thinnest slab and the radius; a slab of
    exactly radius + 1 lines is accepted"""
    with pytest.raises(nls.NKError) as ex:
        nls.grid_slab_pattern(4, 5, 1, "star", "dirichlet", nranks=3, rank=0)          # 1|2|2
    msg = str(ex.value)
    assert "n_outer = 5" in msg and "3 ranks" in msg and "thinnest slab has 1" in msg and "radius-1" in msg
    assert L.lib().nk_grid_slab_pattern(2, 4, 5, 1, 1, 0, 0, 3, 0, None, None, None, None, C.byref(C.c_int64())) == -1   # NK_E_INVALID
    with pytest.raises(nls.NKError) as ex:
        nls.grid_slab_pattern(5, 5, 1, "star2", "periodic", nz=8, nranks=3, rank=1)    # 2|3|3 planes at radius 2
    msg = str(ex.value)
    assert "n_outer = 8" in msg and "3 ranks" in msg and "thinnest slab has 2" in msg and "radius-2" in msg
    for nranks, n_outer, stencil in ((2, 4, "star"), (3, 6, "star"), (2, 6, "star2"), (3, 9, "diamond2")):
        for rank in range(nranks):
            lines, _rp, _ci = nls.grid_slab_pattern(5, n_outer, 1, stencil, "periodic", nranks=nranks, rank=rank)
            assert lines[1] - lines[0] == R.RADIUS[stencil] + 1
    with pytest.raises(nls.NKError):
        nls.grid_slab_pattern(4, 5, 1, "star", "dirichlet", nranks=2, rank=2)          # no such rank


# ------------------------------------------------------------------------------------------------ the programs
_SOURCES = {   # a Bratu source, a 2-component source and a fields source
    "bratu": (G1.PROBLEMS["bratu"], 2, 0),
    "brusselator": (G1.PROBLEMS["brusselator"], 2, 0),
    "vardiff": (GF.PROBLEMS["vardiff"], 2, 3),
}


def _code_object(p, dim, nfields, boundary, nranks, rank, jac):
    args = (p.source.encode(), dim, p.dof, GC.STENCIL_ID[p.stencil], boundary, len(p.params), nfields, nranks, rank, jac)
    nb = C.c_int64()
    assert L.lib().nk_grid_slab_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_grid_slab_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


def _private_segments(code, dim, jac, tmp_path):
    """{kernel: private_segment_fixed_size} from the code object's notes"""
    path = tmp_path / "k.co"
    path.write_bytes(code)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(path)], capture_output=True, text=True,
                           check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        name, priv = re.search(r"\.name:\s+(\w+)", block), re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        if name and priv and name.group(1) in KERNELS[dim][jac]:
            out[name.group(1)] = int(priv.group(1))
    return out


@pytest.mark.parametrize("name", sorted(_SOURCES))
def test_programs_of_every_kind_of_rank_compile_without_a_private_segment(name, tmp_path):
    """rank 0, the middle rank and the last rank of three (a cut above, both, below) and both ranks of two on a periodic axis
    (both sides cuts, the one peer's zones in either order)"""
    p, dim, nfields = _SOURCES[name]
    for sides, ranks in (((DI, DI, MF, DI), [(3, 0), (3, 1), (3, 2)]), ((MF, MF, PE, PE), [(2, 0), (2, 1)])):
        bd = GC.sides_code(sides)
        for nranks, rank in ranks:
            assert nls.grid_compile_check(p.source, p.dof, p.stencil, sides, len(p.params), dim=dim, fields=nfields,
                                          nranks=nranks, rank=rank) > 0
            for jac in (0, 1):
                priv = _private_segments(_code_object(p, dim, nfields, bd, nranks, rank, jac), dim, jac, tmp_path)
                assert sorted(priv) == sorted(KERNELS[dim][jac]), (name, nranks, rank, jac, priv)
                assert all(v == 0 for v in priv.values()), (name, nranks, rank, jac, priv)
    # the programs of a middle rank and of an end rank are different programs
    assert _code_object(p, dim, nfields, GC.sides_code((DI, DI, MF, DI)), 3, 0, 0) != \
        _code_object(p, dim, nfields, GC.sides_code((DI, DI, MF, DI)), 3, 1, 0)


def test_one_rank_programs_are_the_older_entry_points(tmp_path):
    """nk_grid_code_object, nk_grid3_code_object and nk_grid_fields_code_object still succeed, and nk_grid_slab_code_object with
    nranks = 1 returns their bytes"""
    import grid3_reference as G3
    lib = L.lib()

    def older(fn, *args):
        nb = C.c_int64()
        assert fn(*args, None, 0, C.byref(nb)) == 0, lib.nk_last_error()
        buf = C.create_string_buffer(nb.value)
        assert fn(*args, buf, nb.value, C.byref(nb)) == 0
        return buf.raw[:nb.value]
    p2, p3, pf = G1.PROBLEMS["brusselator"], G3.PROBLEMS["brusselator3"], GF.PROBLEMS["vardiff"]
    for jac in (0, 1):
        for bd in (0, 1, GC.sides_code((PE, PE, MF, DI))):
            a = older(lib.nk_grid_code_object, p2.source.encode(), p2.dof, 0, bd, len(p2.params), jac)
            assert a == _code_object(p2, 2, 0, bd, 1, 0, jac)
        a = older(lib.nk_grid3_code_object, p3.source.encode(), p3.dof, 0, 1, len(p3.params), jac)
        assert a == _code_object(p3, 3, 0, 1, 1, 0, jac)
        a = older(lib.nk_grid_fields_code_object, pf.source.encode(), 2, pf.dof, 0, 0, len(pf.params), 3, jac)
        assert a == _code_object(pf, 2, 3, 0, 1, 0, jac)
        assert all(v == 0 for v in _private_segments(a, 2, jac, tmp_path).values())
