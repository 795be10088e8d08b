"""The resident matrix-powers kernel's operand table (csrc/nk_pw_pack.h) is plain host arithmetic, so it is checked here without
a GPU: tests/pw_pack_dump.cpp is compiled with g++ against the header, packs a pattern and writes the table back decoded through
the accessors the kernel uses. Every row's length, row start and W LDS offsets and every slice's extents are compared with the
straightforward translation of what the kernel's load phase used to derive from rowptr / col in every launch, written out below.
The same program is built once more with -fsanitize=address,undefined and run on every pattern."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HALO = 1024, 1024
OK, E_ARG, E_LEN, E_RANGE, E_HALO, E_EXTENT = 0, 1, 2, 3, 4, 5


def _build(tmp, name, extra):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(ROOT, "nonlinearsolve.jl_amd", "csrc"), os.path.join(ROOT, "tests", "pw_pack_dump.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pw_pack")
    return [_build(tmp, "pw_pack_dump", []),
            _build(tmp, "pw_pack_dump_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])], tmp


def _run(dumps, rowptr, col, rpt, w, nb, hvl=None):
    """status and, when the pattern was accepted, (len, start, off[W]) per row and (kb, ke) per slice — from both builds"""
    exes, tmp = dumps
    n = len(rowptr) - 1
    hvl = np.zeros(0, np.int32) if hvl is None else np.asarray(hvl, np.int32)
    path = str(tmp / "pattern.bin")
    np.concatenate([np.array([n, len(col), rpt, w, nb, len(hvl)], np.int32), np.asarray(rowptr, np.int32),
                    np.asarray(col, np.int32), hvl]).tofile(path)
    outs = []
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        outs.append(np.frombuffer(r.stdout, np.int32))
    assert np.array_equal(outs[0], outs[1])
    out = outs[0]
    if out[0] != OK:
        assert out.size == 1
        return int(out[0]), None, None
    rows = nb * rpt * T
    assert out.size == 1 + rows * (2 + w) + nb * rpt * 2
    return OK, out[1:1 + rows * (2 + w)].reshape(rows, 2 + w), out[1 + rows * (2 + w):].reshape(nb * rpt, 2)


def _expected(rowptr, col, rpt, w, nb, hvl=None):
    """what k_spmv_powers' load phase derived per launch: row r of band b = r // RB, slice (r % RB) // T"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n, RB = len(rowptr) - 1, T * rpt
    rows = nb * RB
    rec = np.zeros((rows, 2 + w), np.int64)
    ext = np.zeros((nb * rpt, 2), np.int64)
    for sl in range(nb * rpt):
        rfirst = sl * T
        if rfirst < n:
            ext[sl] = rowptr[rfirst], rowptr[min(rfirst + T, n)]
    for r in range(rows):
        r0 = (r // RB) * RB
        own = HALO + (r - r0)
        rec[r, 2:] = own                                  # slots past the row's end: the row's own offset
        if r >= n:
            continue                                      # a row past the matrix' end is an empty row
        k0, k1 = rowptr[r], rowptr[r + 1]
        rec[r, 0] = k1 - k0
        rec[r, 1] = k0 - ext[r // T, 0]
        for j in range(k1 - k0):
            c = col[k0 + j]
            if c >= n:
                c = hvl[c - n]                            # a halo slot → its row next door (relative to this rank's first row)
            rec[r, 2 + j] = c - (r0 - HALO)
    return rec, ext


def _check(dumps, rowptr, col, rpt, w, hvl=None):
    n = len(rowptr) - 1
    nb = -(-n // (T * rpt))
    rc, rec, ext = _run(dumps, rowptr, col, rpt, w, nb, hvl)
    assert rc == OK
    erec, eext = _expected(rowptr, col, rpt, w, nb, hvl)
    assert np.array_equal(ext, eext)
    bad = np.nonzero((rec != erec).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], rec[bad[:2]], erec[bad[:2]])
    XN = T * rpt + 2 * HALO
    assert rec[:, 2:].min() >= 0 and rec[:, 2:].max() < XN
    return rec, ext


def _bratu(ns):
    """the 5-point pattern, rows lexicographic, columns ascending"""
    rowptr, col = [0], []
    for j in range(ns):
        for i in range(ns):
            r = j * ns + i
            col += [c for c, ok in ((r - ns, j > 0), (r - 1, i > 0), (r, True), (r + 1, i + 1 < ns), (r + ns, j + 1 < ns)) if ok]
            rowptr.append(len(col))
    return np.array(rowptr), np.array(col)


@pytest.mark.parametrize("ns,rpt", [(3, 1), (3, 2), (33, 1), (33, 2), (257, 1), (257, 2), (257, 4), (257, 6)])
def test_bratu_patterns(dumps, ns, rpt):
    """257²: 66 049 rows — a ragged last slice and, at 2 / 4 / 6 slices per band, a ragged last band"""
    rowptr, col = _bratu(ns)
    rec, _ = _check(dumps, rowptr, col, rpt, 5)
    assert rec[: ns * ns, 0].min() == 3 and rec[: ns * ns, 0].max() == (5 if ns > 2 else 4)


def _banded(n, rpt, w, seed):
    """random rows of 0 … w entries inside their band's window; slice 0 full (exactly T·w entries), slice 1 with fewer than T
    entries and an empty first and last row; per band one column at each end of the window (LDS offsets 0 and XN − 1) where the
    matrix has those rows"""
    rng = np.random.default_rng(seed)
    RB = T * rpt
    lens = rng.integers(0, w + 1, size=n)
    lens[:T] = w
    if n > T:
        e = min(2 * T, n)
        lens[T:e] = 0
        lens[T + 1:e - 1:7] = 1
    first_lo, last_hi = {}, {}
    for b in range(-(-n // RB)):
        b0 = b * RB
        lo, hi = b0 - HALO, b0 + RB + HALO - 1
        ra, rb_ = b0 + min(3, n - 1 - b0), min(b0 + RB, n) - 1 - min(2, min(b0 + RB, n) - 1 - b0)
        if lo >= 0:
            first_lo[ra] = lo
            lens[ra] = max(lens[ra], 1)
        if hi < n and rb_ != ra:
            last_hi[rb_] = hi
            lens[rb_] = max(lens[rb_], 1)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(rowptr[-1], np.int64)
    for r in range(n):
        b0 = (r // RB) * RB
        lo, hi = max(0, b0 - HALO), min(n, b0 + RB + HALO)
        c = np.sort(rng.integers(lo, hi, size=lens[r]))
        if r in first_lo:
            c[0] = first_lo[r]
        if r in last_hi:
            c[-1] = last_hi[r]
        col[rowptr[r]:rowptr[r + 1]] = c
    return rowptr, col


@pytest.mark.parametrize("rpt,w", [(1, 5), (2, 5), (4, 5), (6, 5), (1, 8), (2, 8), (1, 16)])
def test_random_banded_rows(dumps, rpt, w):
    for n in (1, 1023, 1024, 1025, 1024 * rpt + 1, 3 * 1024 * rpt + 100):
        rowptr, col = _banded(n, rpt, w, seed=n + w)
        rec, ext = _check(dumps, rowptr, col, rpt, w)
        lens = np.diff(rowptr)
        if n >= T:
            assert ext[0, 1] - ext[0, 0] == T * w                       # a slice with exactly T·w entries …
        if n >= 2 * T:
            assert 0 < ext[1, 1] - ext[1, 0] < T                        # … one with fewer than T …
            assert lens[T] == 0 and lens[2 * T - 1] == 0                # … whose first and last rows are empty
            assert rec[T, 1] == 0 and rec[2 * T - 1, 1] == ext[1, 1] - ext[1, 0]
        if n > T * rpt + HALO:
            assert rec[:, 2:].min() == 0 and rec[:, 2:].max() == T * rpt + 2 * HALO - 1   # both ends of the window
        if n >= 3 * T:
            assert set(np.unique(lens)) == set(range(w + 1))            # every length from 0 to W


def test_two_rank_halo_map(dumps):
    """a middle rank's share: 2 bands of 1024 rows, halo slots 0 … 1023 are the last rows of the rank above (−1024 … −1), slots
    1024 … 2047 the first rows of the rank below (n … n + 1023) — the record holds the row next door, not the slot"""
    n, w = 2048, 5
    rng = np.random.default_rng(7)
    hvl = np.concatenate([np.arange(-1024, 0), np.arange(n, n + 1024)]).astype(np.int32)
    rng.shuffle(hvl[:1024])
    rng.shuffle(hvl[1024:])
    rowptr, col = [0], []
    for r in range(n):
        own = sorted(rng.integers(max(0, r - 500), min(n, r + 500), size=3).tolist())
        halo = (rng.integers(0, 1024, size=2) + (0 if r < 1024 else 1024) + n).tolist()
        col += own + sorted(halo)
        rowptr.append(len(col))
    rec, _ = _check(dumps, np.array(rowptr), np.array(col), 1, w, hvl)
    assert rec[:1024, 5:7].max() < HALO and rec[1024:, 5:7].min() >= HALO + 1024   # above band 0, below band 1
    inv_up = int(np.nonzero(hvl == -1024)[0][0])
    col2 = np.array(col)
    col2[3] = n + inv_up
    rec2, _ = _check(dumps, np.array(rowptr), col2, 1, w, hvl)
    assert rec2[0, 2 + 3] == 0


def test_patterns_that_do_not_fit_are_rejected(dumps):
    rowptr, col = _bratu(40)                       # 1600 rows
    n = len(rowptr) - 1
    assert _run(dumps, rowptr, col, 1, 5, 2)[0] == OK
    assert _run(dumps, rowptr, col, 1, 5, 3)[0] == E_ARG          # not the band count of this layout
    assert _run(dumps, rowptr, col, 1, 7, 2)[0] == E_ARG          # no such record format
    c = col.copy()
    c[rowptr[10]] = n + 5
    assert _run(dumps, rowptr, c, 1, 5, 2)[0] == E_HALO           # a halo slot and no map
    assert _run(dumps, rowptr, c, 1, 5, 2, hvl=[0, 0, 0])[0] == E_HALO
    assert _run(dumps, rowptr, c, 1, 5, 2, hvl=[0, 0, 0, 0, 0, -1025])[0] == E_RANGE   # a row next door outside the window
    assert _run(dumps, rowptr, c, 1, 5, 2, hvl=[0, 0, 0, 0, 0, -1024])[0] == OK
    c = col.copy()
    c[rowptr[1500]] = -1
    assert _run(dumps, rowptr, c, 1, 5, 2)[0] == E_RANGE
    # a row of six entries under W = 5
    lens = np.diff(rowptr)
    lens[7] = 6
    rp6 = np.concatenate([[0], np.cumsum(lens)])
    assert _run(dumps, rp6, np.zeros(rp6[-1], np.int64), 1, 5, 2)[0] == E_LEN
    assert _run(dumps, rp6, np.zeros(rp6[-1], np.int64), 1, 8, 2)[0] == OK
    # a column 1025 rows above its band
    rowptr, col = _banded(4096, 1, 5, 3)
    c = col.copy()
    c[rowptr[2048 + 9]] = 1023
    assert _run(dumps, rowptr, c, 1, 5, 4)[0] == E_RANGE
    c[rowptr[2048 + 9]] = 1024
    assert _run(dumps, rowptr, c, 1, 5, 4)[0] == OK
    # a row pointer that runs backwards
    rp = rowptr.copy()
    rp[100] = rp[99] - 1
    assert _run(dumps, rp, col, 1, 5, 4)[0] in (E_LEN, E_EXTENT)
