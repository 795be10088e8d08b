"""The resident matrix-powers kernel with its load phase driven by the plan's packed operand table (csrc/nk_pw_pack.h; the
table's content is checked without a GPU in tests/test_pw_pack.py). The kernel no longer reads rowptr / col: what it gathers and
which values it picks comes from a table built once per pattern — so every word of every column is compared with the library's
STREAMING launches (one child process with NK_SPMV_POWERS=0 computes them all, once) and with the oracle's CSR-order row sums, on
the packer test's patterns: Bratu 3² / 33² / 257², ragged random rows of ≤ 5 / 8 / 16 entries with empty rows at slice ends, a full
and a nearly empty slice, columns at both ends of a band's window, n = 1, 1023, 1024, 1025, 3172. At these sizes (n ≤ 66 049) a band
is one slice; the two-buffer staging of bands with 2 – 6 slices runs in tests/test_gpu_powers.py (1024², 300 000 … 1 300 000 rows),
which passes unchanged."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.test_pw_pack import _banded, _bratu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_LIST = (1, 2, 15)


@functools.lru_cache(maxsize=None)
def _cases():
    """name → (rowptr, col, val, x)"""
    out = {}
    for ns in (3, 33, 257):
        rowptr, col = _bratu(ns)
        out[f"bratu{ns}"] = (rowptr, col)
    for w in (5, 8, 16):
        for n in (1, 1023, 1024, 1025, 3 * 1024 + 100):
            out[f"banded_w{w}_n{n}"] = _banded(n, 1, w, seed=n + w)
    full = {}
    for k, (name, (rowptr, col)) in enumerate(sorted(out.items())):
        rng = np.random.default_rng(100 + k)
        n = len(rowptr) - 1
        full[name] = (np.asarray(rowptr, np.int32), np.asarray(col, np.int32), rng.standard_normal(len(col)) * 0.3,
                      rng.standard_normal(n))
    return full


CASES = sorted(_cases())


def _theta_scale(rowptr, val, s, shifted):
    rowsum = np.zeros(len(rowptr) - 1)
    np.add.at(rowsum, np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), np.abs(val))
    lam = max(1.0, float(rowsum.max()))
    return ((0.5 + 0.4 * np.cos(np.arange(s))) * lam if shifted else None), (2.0 / lam if shifted else 1.0)


def _ref(rowptr, col, val, x, s, theta, scale):
    """s sequential applications with the oracle's CSR-order row sum; epilogue as the streaming kernel forms it"""
    out = np.empty((s, x.size))
    cur = x
    for p in range(s):
        y = CO.spmv(rowptr, col, val, cur)
        if theta is not None:
            y = y - theta[p] * cur
        y = scale * y
        out[p] = y
        cur = y
    return out


def _launch(nls, A, rowptr, val, x, s, shifted):
    import torch
    theta, scale = _theta_scale(rowptr, val, s, shifted)
    Y, resident = A.powers(torch.tensor(x, device="cuda"), s, theta=theta, scale=scale)
    return Y.cpu().numpy(), resident, theta, scale


def _streaming_main(path):
    """child process (NK_SPMV_POWERS=0): every case's streaming launches → one .npz"""
    import nonlinearsolve_jl_amd as nls
    out = {}
    for name, (rowptr, col, val, x) in _cases().items():
        A = nls.CSRMatrix.from_arrays(rowptr, col, val)
        for s in S_LIST:
            for shifted in (True, False):
                Y, resident, _, _ = _launch(nls, A, rowptr, val, x, s, shifted)
                assert not resident
                out[f"{name}|{s}|{int(shifted)}"] = Y
    np.savez(path, **out)


@pytest.fixture(scope="module")
def streaming(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pw_pack_gpu") / "streaming.npz")
    r = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r}); "
                        f"from tests.test_gpu_powers_pack import _streaming_main; _streaming_main({path!r})"],
                       env=dict(os.environ, NK_SPMV_POWERS="0"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("name", CASES)
def test_table_driven_load_is_bit_exact(nls, dev, streaming, name):
    rowptr, col, val, x = _cases()[name]
    A = nls.CSRMatrix.from_arrays(rowptr, col, val)
    for s in S_LIST:
        for shifted in (True, False):
            theta, scale = _theta_scale(rowptr, val, s, shifted)
            ref, stream = _ref(rowptr, col, val, x, s, theta, scale), streaming[f"{name}|{s}|{int(shifted)}"]
            for rep in range(2):
                Y, resident, _, _ = _launch(nls, A, rowptr, val, x, s, shifted)
                assert resident, (name, s, shifted)
                assert np.array_equal(Y, stream), (name, s, shifted, rep, "streaming launches")
                assert np.array_equal(Y, ref), (name, s, shifted, rep, "CSR-order row sums")


def test_values_refreshed_in_place_are_seen_by_the_next_launch(nls, dev):
    """the table holds no values: set_values between two launches, the same plan, the new columns"""
    rowptr, col, val, x = _cases()["banded_w8_n3172"]
    A = nls.CSRMatrix.from_arrays(rowptr, col, val)
    Y, resident, theta, scale = _launch(nls, A, rowptr, val, x, 15, True)
    assert resident and np.array_equal(Y, _ref(rowptr, col, val, x, 15, theta, scale))
    val2 = np.random.default_rng(9).standard_normal(val.size) * 0.3
    A.set_values(val2)
    Y2, resident, theta2, scale2 = _launch(nls, A, rowptr, val2, x, 15, True)
    assert resident and np.array_equal(Y2, _ref(rowptr, col, val2, x, 15, theta2, scale2))
    assert not np.array_equal(Y, Y2)


def test_two_live_matrices_of_equal_shape_launched_alternately(nls, dev):
    """each plan owns its table: same n, same W, same band layout, different rows and columns"""
    n, w = 3 * 1024 + 100, 5
    rng = np.random.default_rng(21)
    mats = []
    for seed in (1, 2):
        rowptr, col = _banded(n, 1, w, seed=seed)
        rowptr, col = np.asarray(rowptr, np.int32), np.asarray(col, np.int32)
        val = rng.standard_normal(col.size) * 0.3
        mats.append((nls.CSRMatrix.from_arrays(rowptr, col, val), rowptr, col, val))
    assert not np.array_equal(mats[0][2][:5000], mats[1][2][:5000])
    x = rng.standard_normal(n)
    refs = [None, None]
    for rep in range(6):
        A, rowptr, col, val = mats[rep % 2]
        Y, resident, theta, scale = _launch(nls, A, rowptr, val, x, 7, rep % 3 != 0)
        assert resident
        assert np.array_equal(Y, _ref(rowptr, col, val, x, 7, theta, scale)), rep
        refs[rep % 2] = Y
    assert refs[0].shape == refs[1].shape


def test_peer_bands_take_their_halo_rows_from_the_table(nls):
    """two ranks, Bratu 64² (the multi-rank harness at its smallest size): the halo slot → neighbour row map is folded into the
    records — every column equals the serial oracle's, the blocks keep one exchange protocol per launch"""
    from tests import test_gpu_multirank as MR
    ctx = MR.mp.get_context("spawn")
    q = ctx.Queue()
    port = MR._free_port()
    procs = [ctx.Process(target=MR._powers_worker, args=(r, 2, port, q, 64, "1")) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=280) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res
    assert len({r[2] for r in res}) == 1
