"""Cases, the reference and the assertions for the aggregation AMG (csrc/nk_amg.hip), in plain NumPy / SciPy.
tests/test_gpu_amg_direct.py hands the device's hierarchy and V-cycles to the check_* functions below;
tests/test_amg_reference.py hands them the oracle's float64 restatement (oracle.reference_restatement.AggregationAMG, which must
pass) and float64 copies of the reference with one planted defect each (which must fail), without a GPU.

The reference runs on a GIVEN structure (`Structure`): the aggregates of every level and the entry maps R.amg_galerkin derives
from them. The aggregates are integer-exact results of R.amg_handshake_pass / R.amg_pairwise_pass under the device's variant rule
(that is: of R.AggregationAMG), so no tolerance applies to them. On that structure
  * `numbers(S, v, dtype)` forms every level's values (Galerkin sums in ascending fine position), D⁻¹ and λmax =
    max_i (Σ_j |a_ij| in stored order) / |a_ii|, sequentially, in `dtype`. In float64 these are BIT-EXACT references: the library
    is built with -ffp-contract=off and without fast-math and its kernels sum sequentially in the same order.
  * `VCycle(S, v, dtype)` is the V-cycle in `dtype` (np.longdouble: the reference of every apply check; np.float64: the stand-in
    where the long-double one is too slow): ν Chebyshev steps on D⁻¹A, the residual, the restriction over members in ascending
    row order, the coarse solve — Gaussian elimination with partial pivoting in `dtype` on a dense coarsest level, 4ν Chebyshev
    steps on a coarsest level that is not dense —, the prolongation with ω, ν steps again.

Matrices (every case carries a second value set on the same pattern for `update()`):
  chain(n, σ)       tridiag(−1, 2 + σ, −1); σ = 0.5 is well conditioned. n = 0 … 128: one dense level, the identity border of
                    k_amg_dense_fill where n is no multiple of 8; 129 … 257: the first coarsening; 2047 … 4096 (and 4094 / 4096
                    with passes = 1: nc + 1 = 2048 / 2049): the scan's tile edges. chain(128, 0): the one ill-conditioned dense case.
  bratu(ns)         the Bratu Jacobian of the oracle at a seeded random u; random3000sym: the ragged matrix of test_gpu_amg.py
  signs             −bratu(48) (every diagonal negative), rows of bratu(20) with alternating sign (non-symmetric), a chain with
                    stored explicit zeros and rows that hold only their diagonal entry
  stall600          diagonal 3, −1 inside the pairs (2k, 2k+1), +0.5 between neighbouring pairs, passes = 1: sizes [600, 300], the
                    level-1 matrix has no negative coupling left — a coarsest level that is not dense (4ν steps)
  gershgorin(p)     262144 + 257 rows, mostly diagonal (coarsening stalls at level 0: fewer than 600 rows have a neighbour, so
                    more than 0.8·n aggregates under any matching), the row of the largest bound planted at p ∈ {0, 255, 256,
                    n − 1}: workgroup edges of k_amg_diag and its wrapped grid-stride loop. Apply: the LONG-DOUBLE V-cycle is used
                    (one level, 8 steps: under a second).
  chain4(11)        chain(4**11, 0.5): n + 1 > 2048², the scan's third level. Closed form (`closed_chain4`): aggregates
                    arange(n_l) // 4 on every level, sizes 4**11 … 4**3, level l = tridiag(−1, 2 + 0.5·4**l, −1) exactly (every
                    partial sum is a small dyadic number). Apply there is compared with the module's FLOAT64 V-cycle; its row
                    of TABLE is the deviation of that float64 V-cycle from the long-double one, recorded once by
                        python tests/amg_reference.py chain4
                    (ten seconds on a CPU, too long for a test that runs with every suite); the CPU test recomputes every other row.

Tolerances. TABLE holds one row per apply case: the largest max-norm relative deviation of the float64 restatement from the
long-double V-cycle over the case's right-hand sides (seeded random, e_0, e_{n−1}), both value sets and both matchings, with the
restatement's dense coarsest solve once as inv @ b and once as np.linalg.solve, rounded UP to a power of two. The device bound is
FACTOR = 100 times the row and never below FLOOR = 1e-14 (the margin and floor of tests/gmres_reference.py): the device differs
from the restatement by reformulations of the size of the restatement's own rounding (lane-order row sums in the SpMV,
Gauss–Jordan instead of LU). No bound may exceed LIMIT = 2e-12. Regenerate with

    python tests/amg_reference.py

The pattern of a device level matrix cannot be read back through the ABI (nk_csr has no pattern getter); check_structure takes
either the arrays (the restatement) or the level's SpMV: with the value array equal bit for bit in stored order, equal n and nnz,
a product with a seeded vector of distinct entries in [1, 2) must agree with the reference pattern's product to rounding
(γ = 2·(row length + 1)·2⁻⁵³ relative to Σ|a_ij x_j|) — a misplaced column or row boundary moves it by |a_ij|·|x_j − x_j'|."""
import functools
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reference_restatement as R  # noqa: E402

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
FACTOR, FLOOR, LIMIT = 100.0, 1e-14, 2e-12
MATCHINGS = ("auto", "greedy")                       # the device's names; the restatement's: handshake / greedy
DEFAULTS = dict(nu=2, passes=2, theta=0.25, overcorrection=1.8, cheb_ratio=4.0, coarse_max=128)


def oracle_matching(matching):
    return "greedy" if matching == "greedy" else "handshake"


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------------------------------------------------- matrices
def chain(n, sigma=0.5):
    if n == 0:
        return sp.csr_matrix((0, 0))
    A = sp.diags([-np.ones(max(n - 1, 0)), np.full(n, 2.0 + sigma), -np.ones(max(n - 1, 0))], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def bratu(ns):
    pb = R.Bratu2D(ns)
    A = pb.jac(np.random.default_rng(_seed("bratu", ns)).standard_normal(pb.n) * 0.2).tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def random3000sym():
    n = 3000
    B = sp.random(n, n, density=0.002, random_state=5, format="csr")
    B.data = -np.abs(B.data)
    Bs = (B + B.T).tocsr()
    A = (Bs + sp.diags(np.asarray(abs(Bs).sum(axis=1)).ravel() + 0.5)).tocsr()
    A.sort_indices()
    return A


def alternating_rows():
    A = bratu(20)
    return (sp.diags((-1.0) ** np.arange(A.shape[0])) @ A).tocsr()


def zeros_and_lone_rows(n=300):
    """a chain with some couplings stored as 0.0 and some rows that hold only their diagonal entry"""
    rp, ci, v = [0], [], []
    lone = {5, 100, 101, n - 1}
    for i in range(n):
        if i not in lone:
            if i > 0:
                ci.append(i - 1), v.append(-1.0)
            ci.append(i), v.append(2.5 + 0.001 * (i % 7))
            if i < n - 1:
                ci.append(i + 1), v.append(0.0 if 20 <= i < 40 else -1.0)
        else:
            ci.append(i), v.append(1.75)
        rp.append(len(ci))
    return sp.csr_matrix((np.array(v), np.array(ci), np.array(rp)), shape=(n, n))


def stall600(n=600):
    k = np.arange(n)
    off = np.where(k[:-1] % 2 == 0, -1.0, 0.5)
    return sp.diags([off, np.full(n, 3.0), off], [-1, 0, 1], format="csr")


GERSHGORIN_N = 262144 + 257


@functools.lru_cache(maxsize=None)
def gershgorin(p):
    n = GERSHGORIN_N
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [4.0 + 0.3 * np.cos(np.arange(n))]
    some = np.arange(1000, n - 1000, 1000)
    some = some[(np.abs(some - p) > 4)]
    rows += [some, some + 1]
    cols += [some + 1, some]
    vals += [np.full(len(some), -1.1), np.full(len(some), -0.9)]
    nb = {0: (1, 2), 255: (254, 256), 256: (255, 257), n - 1: (n - 3, n - 2)}[p]
    rows.append(np.array([p, p]))
    cols.append(np.array(nb))
    vals.append(np.array([-2.3, -1.7]))                  # (4.3 + 4) / 3.7 at the least: above every other row's 1 + 1.1 / 3.7
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


# ------------------------------------------------------------------------------------------------------------- cases
def _case(name, family, build, apply="ld", **params):
    return SimpleNamespace(name=name, family=family, build=build, params=params, apply=apply)


def _cases():
    out = []
    for n in (0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128):
        out.append(_case(f"chain{n}", "dense", functools.partial(chain, n)))
    out.append(_case("chain128s0", "dense", functools.partial(chain, 128, 0.0)))
    for n in (129, 130, 200, 257):
        out.append(_case(f"chain{n}", "coarsen", functools.partial(chain, n)))
    for n in (2047, 2048, 4095, 4096):
        out.append(_case(f"chain{n}", "scan", functools.partial(chain, n)))
    for n in (4094, 4096):
        out.append(_case(f"chain{n}p1", "scan", functools.partial(chain, n), passes=1))
    for cm in (1, 8, 64):
        out.append(_case(f"chain300cm{cm}", "coarse_max", functools.partial(chain, 300), coarse_max=cm))
        out.append(_case(f"bratu20cm{cm}", "coarse_max", functools.partial(bratu, 20), coarse_max=cm))
    sweeps = [("nu", (1, 3, 16)), ("passes", (1, 3, 4)), ("theta", (0.05, 0.9)), ("overcorrection", (1.0, 1.3)),
              ("cheb_ratio", (1.5, 30.0))]
    for mname, mk in (("bratu48", functools.partial(bratu, 48)), ("random3000sym", random3000sym)):
        for key, vals in sweeps:
            for val in vals:
                out.append(_case(f"{mname}-{key}{val}", "sweep", mk, **{key: val}))
    out.append(_case("negbratu48", "signs", lambda: (-bratu(48)).tocsr()))
    out.append(_case("altrows20", "signs", alternating_rows))
    out.append(_case("zeros300", "signs", zeros_and_lone_rows))
    out.append(_case("stall600", "stall", stall600, passes=1))
    for p in (0, 255, 256, GERSHGORIN_N - 1):
        out.append(_case(f"gershgorin{p}", "gershgorin", functools.partial(gershgorin, p)))
    return out


CASES = {c.name: c for c in _cases()}
CHAIN4 = SimpleNamespace(name="chain4_11", family="chain4", k=11, params={}, apply="f64")
# where both matchings give the same aggregates (asserted by the CPU test; the chains and the Bratu grids while their levels are
# even-sized): host and device set-ups bit for bit
SAME_AGGREGATES = tuple(n for n in CASES if n.startswith("chain") or n.startswith("bratu48") or
                        n in ("bratu20cm64", "negbratu48", "stall600"))


def params_of(case):
    p = dict(DEFAULTS)
    p.update(case.params)
    return p


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = CASES[name].build()
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def values(name, which=0):
    """the case's value array in stored order: which = 0 the first set, 1 the second (same pattern, every entry moved by a
    seeded factor in [1, 1.1))"""
    v = matrix(name).data.astype(np.float64)
    if which:
        v = v * (1.0 + 0.1 * np.random.default_rng(_seed("v2", name)).random(len(v)))
    return v


def rhs_set(n, name):
    out = [np.random.default_rng(_seed("b", name)).standard_normal(n)]
    for j in (0, n - 1):
        e = np.zeros(n)
        if n:
            e[j] = 1.0
        out.append(e)
    return out


# ------------------------------------------------------------------------------------------------------------- structure
class Structure:
    """pats[l] = (rowptr, col, n) of every level (coarsest last), aggs[l] / emaps[l] of every level but the coarsest;
    fixed_values[l] (closed forms only) replaces the Galerkin sums"""

    def __init__(self, pats, aggs, emaps, prm, fixed_values=None):
        self.pats, self.aggs, self.emaps, self.prm, self.fixed_values = pats, aggs, emaps, dict(prm), fixed_values
        self.dense = pats[-1][2] <= prm["coarse_max"]

    def sizes(self):
        return [p[2] for p in self.pats]


def structure_from_oracle(O, prm):
    pats = [(L["rp"], L["ci"], L["n"]) for L in O.levels] + [(O.coarse["rp"], O.coarse["ci"], O.coarse["n"])]
    return Structure(pats, [L["agg"] for L in O.levels], [L["emap"] for L in O.levels], prm)


@functools.lru_cache(maxsize=None)
def oracle_of(name, matching):
    """the float64 restatement on the case's first value set"""
    if CASES[name].family == "gershgorin":       # no level is coarsened under any matching (see the docstring): the vectorised rule
        matching = "auto"
    return R.AggregationAMG(sp.csr_matrix((values(name), matrix(name).indices, matrix(name).indptr), shape=matrix(name).shape),
                            matching=oracle_matching(matching), **params_of(CASES[name]))


@functools.lru_cache(maxsize=None)
def structure(name, matching):
    return structure_from_oracle(oracle_of(name, matching), params_of(CASES[name]))


def _tridiag_pattern(n):
    rp = np.zeros(n + 1, dtype=np.int64)
    cnt = np.full(n, 3, dtype=np.int64)
    cnt[0] -= 1
    cnt[-1] -= 1
    rp[1:] = np.cumsum(cnt)
    i = np.arange(n)
    ci = np.stack([i - 1, i, i + 1], axis=1).ravel()
    return rp, ci[1:-1].astype(np.int64)


def _tridiag_values(n, d):
    v = np.tile(np.array([-1.0, d, -1.0]), n)
    return v[1:-1]


@functools.lru_cache(maxsize=None)
def closed_chain4(k):
    """chain(4**k, 0.5) under the default parameters, in closed form (both matchings)"""
    pats, aggs, vals = [], [], []
    for l in range(k - 2):
        n = 4 ** (k - l)
        pats.append(_tridiag_pattern(n) + (n,))
        vals.append(_tridiag_values(n, 2.0 + 0.5 * 4.0 ** l))
        if l < k - 3:
            aggs.append(np.arange(n, dtype=np.int64) // 4)
    return Structure(pats, aggs, [None] * len(aggs), DEFAULTS, fixed_values=vals)


def numbers(S, v0, dtype=np.float64, defect=None):
    """per level: dict(n, rp, ci, rows, v, dinv, lmax) in `dtype`, sums sequential in stored / ascending fine order"""
    out = []
    v = np.asarray(v0, dtype=dtype)
    for l, (rp, ci, n) in enumerate(S.pats):
        if S.fixed_values is not None:
            v = np.asarray(S.fixed_values[l], dtype=dtype)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        on = ci == rows
        d, s = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
        np.add.at(d, rows[on], v[on])
        np.add.at(s, rows, np.abs(v))
        if np.any(d == 0) or not np.all(np.isfinite(d)):
            raise ArithmeticError("AMG: zero or non-finite diagonal entry")
        ratio = s / np.abs(d)
        if defect == "lmax_all_but_last" and n > 1:
            ratio = ratio[:-1]
        out.append(dict(n=n, rp=rp, ci=ci, rows=rows, v=v, dinv=1 / d, lmax=ratio.max() if n else dtype(1.0)))
        if l + 1 < len(S.pats) and S.fixed_values is None:
            em = S.emaps[l]
            nv = np.zeros(len(S.pats[l + 1][1]), dtype=dtype)
            if defect == "galerkin_miss" and l == 0:
                keep = np.ones(len(v), dtype=bool)
                keep[np.nonzero(em == em[len(em) // 2])[0][-1]] = False
                np.add.at(nv, em[keep], v[keep])
            elif defect == "galerkin_descending" and l == 0:
                np.add.at(nv, em, v)
                e = int(np.argmax(np.bincount(em)))              # the entry with the most addends, re-summed from the back
                acc = dtype(0.0)
                for t in np.nonzero(em == e)[0][::-1]:
                    acc = acc + v[t]
                nv[e] = acc
            else:
                np.add.at(nv, em, v)
            v = nv
    return out


def ge_solve(A, b, dtype):
    """A x = b by Gaussian elimination with partial pivoting in `dtype`"""
    M, x = np.array(A, dtype=dtype), np.array(b, dtype=dtype)
    n = len(x)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if M[p, k] == 0:
            raise ArithmeticError("AMG: the coarsest-level matrix is singular")
        if p != k:
            M[[k, p]] = M[[p, k]]
            x[[k, p]] = x[[p, k]]
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:, k:] -= np.outer(f, M[k, k:])
        x[k + 1:] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - M[k, k + 1:] @ x[k + 1:]) / M[k, k]
    return x


APPLY_DEFECTS = ("restrict_drop_last", "prolong_neighbour", "nu_off_by_one", "coarse_nu", "omega_twice", "omega_none",
                 "stale_residual", "lmax_wrong_level", "stale_dinv", "coarse_transposed", "border_leak")
SETUP_DEFECTS = ("lmax_all_but_last", "galerkin_miss", "galerkin_descending", "aggregates_by_largest_row")


class VCycle:
    """one V-cycle on the structure S with the values v, everything in `dtype`; `defect`: one of APPLY_DEFECTS"""

    def __init__(self, S, v, dtype=LD, defect=None):
        self.S, self.dtype, self.defect = S, dtype, defect
        self.nu, self.omega, self.ratio = int(S.prm["nu"]), dtype(S.prm["overcorrection"]), dtype(S.prm["cheb_ratio"])
        self.update(v)

    def update(self, v):
        old = getattr(self, "lv", None)
        self.lv = numbers(self.S, v, self.dtype)
        if self.defect == "stale_dinv" and old is not None:
            for a, b in zip(self.lv, old):
                a["dinv"] = b["dinv"]
        if self.defect == "lmax_wrong_level" and len(self.lv) > 1:
            self.lv[0]["lmax"] = self.lv[1]["lmax"]
        for L in self.lv:
            if self.dtype == np.float64:
                L["A"] = sp.csr_matrix((L["v"], L["ci"], L["rp"]), shape=(L["n"], L["n"]))
        C = self.lv[-1]
        if self.S.dense:
            D = np.zeros((C["n"], C["n"]), dtype=self.dtype)
            np.add.at(D, (C["rows"], C["ci"]), C["v"])
            if self.defect == "coarse_transposed":
                D = D.T.copy()
            if self.defect == "border_leak" and C["n"] % 8:
                D[-1, -1] += 1.0                                  # the border's one lands on row n − 1
            self.D = D
        return self

    def _mv(self, L, x):
        if self.dtype == np.float64:
            return L["A"] @ x
        y = np.zeros(L["n"], dtype=self.dtype)
        np.add.at(y, L["rows"], L["v"] * x[L["ci"]])
        return y

    def _cheb(self, L, b, x, nsteps):
        lmax = L["lmax"]
        lmin = lmax / self.ratio
        th, de = (lmax + lmin) / 2, (lmax - lmin) / 2
        s1 = th / de
        rho = 1 / s1
        if x is None:
            r = b.copy()
            d = L["dinv"] * r * (1 / th)
            x = d.copy()
        else:
            r = b - self._mv(L, x)
            d = L["dinv"] * r * (1 / th)
            x = x + d
        for _ in range(1, nsteps):
            rho_new = 1 / (2 * s1 - rho)
            r = r - self._mv(L, d)
            d = (rho_new * rho) * d + (2 * rho_new / de) * (L["dinv"] * r)
            x = x + d
            rho = rho_new
        return x, r, d

    def __call__(self, b, level=0):
        b = np.asarray(b, dtype=self.dtype)
        L = self.lv[level]
        if L["n"] == 0:
            return b.copy()
        if level == len(self.lv) - 1:
            if self.S.dense:
                return ge_solve(self.D, b, self.dtype)
            return self._cheb(L, b, None, (1 if self.defect == "coarse_nu" else 4) * self.nu)[0]
        agg, nc = self.S.aggs[level], self.S.pats[level + 1][2]
        x, r, d = self._cheb(L, b, None, self.nu + (1 if self.defect == "nu_off_by_one" else 0))
        if self.defect != "stale_residual":
            r = r - self._mv(L, d)
        bc = np.zeros(nc, dtype=self.dtype)
        if self.defect == "restrict_drop_last" and level == 0:
            keep = np.ones(L["n"], dtype=bool)
            keep[np.nonzero(agg == agg[L["n"] // 2])[0][-1]] = False
            np.add.at(bc, agg[keep], r[keep])
        else:
            np.add.at(bc, agg, r)
        xc = self(bc, level + 1)
        pick = agg
        if self.defect == "prolong_neighbour" and level == 0:
            pick = agg.copy()
            i = L["n"] // 2
            pick[i] = agg[i] + 1 if agg[i] + 1 < nc else agg[i] - 1
        om = self.omega
        if self.defect == "omega_twice":
            om = om * om
        if self.defect == "omega_none":
            om = self.dtype(1.0)
        x = x + om * xc[pick]
        return self._cheb(L, b, x, self.nu)[0]


@functools.lru_cache(maxsize=None)
def reference_applies(name, matching, which):
    """the long-double V-cycle on the case's right-hand sides (a tuple of arrays)"""
    S = structure(name, matching)
    V = VCycle(S, values(name, which), LD)
    return tuple(V(b) for b in rhs_set(S.sizes()[0], name))


# ------------------------------------------------------------------------------------------------------------- tolerances
def relmax(y, ref):
    ref = np.asarray(ref)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(y, dtype=ref.dtype) - ref)) / max(np.max(np.abs(ref)), np.finfo(float).tiny))


def pow2_up(x):
    return 0.0 if x == 0 else float(2.0 ** np.ceil(np.log2(x)))


class _Solve:
    def __init__(self, A):
        self.A = A

    def __matmul__(self, b):
        return np.linalg.solve(self.A, b) if len(b) else b


def oracle_with_values(name, matching, which, solve=False):
    O = _copy_oracle(oracle_of(name, matching))
    m = matrix(name)
    O.update(sp.csr_matrix((values(name, which), m.indices, m.indptr), shape=m.shape))
    if solve and O.coarse["dense"]:
        O.coarse["inv"] = _Solve(O.coarse["A"].toarray())
    return O


def _copy_oracle(O):
    import copy
    C = copy.copy(O)
    C.levels = [dict(L) for L in O.levels]
    C.coarse = dict(O.coarse)
    return C


def measure_row(name):
    """the restatement's deviation from the long-double V-cycle, rounded up to a power of two"""
    worst = 0.0
    for matching in MATCHINGS:
        for which in (0, 1):
            ref = reference_applies(name, matching, which)
            for solve in (False, True):
                O = oracle_with_values(name, matching, which, solve)
                for b, y in zip(rhs_set(matrix(name).shape[0], name), ref):
                    worst = max(worst, relmax(O(b), y))
    return pow2_up(worst)


def measure_chain4_row(k=CHAIN4.k):
    S = closed_chain4(k)
    n = S.sizes()[0]
    V64, VLD = VCycle(S, None, np.float64), VCycle(S, None, LD)
    return pow2_up(max(relmax(V64(b), VLD(b)) for b in rhs_set(n, CHAIN4.name)))


def bound(name):
    b = max(FACTOR * TABLE[name], FLOOR)
    assert b <= LIMIT, (name, b)
    return b


# ------------------------------------------------------------------------------------------------------------- checks
def probe(n, l):
    return 1.0 + np.random.default_rng(_seed("probe", n, l)).random(n)


def check_pattern_by_product(rp, ci, v, y, l):
    """y = (the level's own SpMV)(probe(n, l)) against the product on the reference pattern (see the module docstring)"""
    n = len(rp) - 1
    x = probe(n, l)
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    ref, mag = A @ x, abs(A) @ x
    gam = 2.0 * (np.diff(rp) + 1) * 2.0 ** -53
    bad = np.nonzero(np.abs(np.asarray(y) - ref) > gam * mag)[0]
    assert len(bad) == 0, f"level {l}: the product of the level matrix disagrees with the reference pattern in rows {bad[:5]}"


def check_structure(S, lv, got, what="", lmax_ulps=0):
    """S, lv = numbers(S, v, np.float64): the reference. got: dict(sizes, aggs (row → coarse row per level), lmax, levels =
    [dict(nnz, vals, and rp / ci or y = A_l·probe(n_l, l))]). lmax_ulps = 0 (the device: equality); the restatement sums a
    row's |a_ij| in SciPy's order, not the stored one: it gets the longest row's length in units of 2⁻⁵³"""
    assert list(got["sizes"]) == S.sizes(), f"{what}sizes {got['sizes']} vs {S.sizes()}"
    assert len(got["aggs"]) == len(S.aggs)
    for l, a in enumerate(S.aggs):
        assert np.array_equal(np.asarray(got["aggs"][l], dtype=np.int64), a), f"{what}aggregates of level {l}"
    for l, (L, g) in enumerate(zip(lv, got["levels"])):
        assert g["nnz"] == len(L["ci"]), f"{what}level {l}: {g['nnz']} entries vs {len(L['ci'])}"
        gv = np.asarray(g["vals"], dtype=np.float64)
        assert gv.shape == L["v"].shape and np.array_equal(gv.view(np.int64), L["v"].view(np.int64)), \
            f"{what}level {l}: values differ from the sequential ascending sums, first at {np.nonzero(gv != L['v'])[0][:5]}"
        if g.get("rp") is not None:
            assert np.array_equal(g["rp"], L["rp"]) and np.array_equal(g["ci"], L["ci"]), f"{what}level {l}: pattern"
        else:
            check_pattern_by_product(L["rp"], L["ci"], L["v"], g["y"], l)
    check_lmax(lv, got["lmax"], what, lmax_ulps)


def check_lmax(lv, lmax, what="", ulps=0):
    for l, L in enumerate(lv):
        assert abs(float(lmax[l]) - float(L["lmax"])) <= ulps * 2.0 ** -53 * float(L["lmax"]), f"{what}λmax of level {l}: {float(lmax[l])!r} vs the sequential {float(L['lmax'])!r}"


def check_apply(name, y, ref, what=""):
    dev = relmax(y, ref)
    assert dev <= bound(name), f"{what}{name}: deviation {dev:.3e} from the reference V-cycle, bound {bound(name):.3e}"
    return dev


def oracle_as_got(O):
    """the restatement's hierarchy in the form check_structure takes"""
    lv = O.levels + [O.coarse]
    return dict(sizes=O.sizes(), aggs=[L["agg"] for L in O.levels], lmax=[L["lmax"] for L in lv],
                levels=[dict(nnz=L["A"].nnz, vals=L["A"].data, rp=L["A"].indptr, ci=L["A"].indices) for L in lv])


# one row per apply case (python tests/amg_reference.py prints this dictionary)
TABLE = {
    "chain4_11": 4.440892098500626e-16,   # (the float64 V-cycle of this module; see the docstring)
    "chain0": 0.0,
    "chain1": 5.551115123125783e-17,
    "chain2": 2.220446049250313e-16,
    "chain7": 2.220446049250313e-16,
    "chain8": 4.440892098500626e-16,
    "chain9": 2.220446049250313e-16,
    "chain63": 4.440892098500626e-16,
    "chain64": 4.440892098500626e-16,
    "chain65": 4.440892098500626e-16,
    "chain127": 8.881784197001252e-16,
    "chain128": 4.440892098500626e-16,
    "chain128s0": 1.4210854715202004e-14,
    "chain129": 4.440892098500626e-16,
    "chain130": 8.881784197001252e-16,
    "chain200": 4.440892098500626e-16,
    "chain257": 4.440892098500626e-16,
    "chain2047": 4.440892098500626e-16,
    "chain2048": 4.440892098500626e-16,
    "chain4095": 4.440892098500626e-16,
    "chain4096": 4.440892098500626e-16,
    "chain4094p1": 4.440892098500626e-16,
    "chain4096p1": 4.440892098500626e-16,
    "chain300cm1": 4.440892098500626e-16,
    "bratu20cm1": 4.440892098500626e-16,
    "chain300cm8": 2.220446049250313e-16,
    "bratu20cm8": 8.881784197001252e-16,
    "chain300cm64": 4.440892098500626e-16,
    "bratu20cm64": 8.881784197001252e-16,
    "bratu48-nu1": 8.881784197001252e-16,
    "bratu48-nu3": 8.881784197001252e-16,
    "bratu48-nu16": 1.7763568394002505e-15,
    "bratu48-passes1": 1.7763568394002505e-15,
    "bratu48-passes3": 8.881784197001252e-16,
    "bratu48-passes4": 1.7763568394002505e-15,
    "bratu48-theta0.05": 8.881784197001252e-16,
    "bratu48-theta0.9": 1.7763568394002505e-15,
    "bratu48-overcorrection1.0": 4.440892098500626e-16,
    "bratu48-overcorrection1.3": 8.881784197001252e-16,
    "bratu48-cheb_ratio1.5": 8.881784197001252e-16,
    "bratu48-cheb_ratio30.0": 8.881784197001252e-16,
    "random3000sym-nu1": 4.440892098500626e-16,
    "random3000sym-nu3": 4.440892098500626e-16,
    "random3000sym-nu16": 4.440892098500626e-16,
    "random3000sym-passes1": 8.881784197001252e-16,
    "random3000sym-passes3": 8.881784197001252e-16,
    "random3000sym-passes4": 4.440892098500626e-16,
    "random3000sym-theta0.05": 4.440892098500626e-16,
    "random3000sym-theta0.9": 4.440892098500626e-16,
    "random3000sym-overcorrection1.0": 2.220446049250313e-16,
    "random3000sym-overcorrection1.3": 4.440892098500626e-16,
    "random3000sym-cheb_ratio1.5": 4.440892098500626e-16,
    "random3000sym-cheb_ratio30.0": 1.7763568394002505e-15,
    "negbratu48": 8.881784197001252e-16,
    "altrows20": 1.4210854715202004e-14,
    "zeros300": 4.440892098500626e-16,
    "stall600": 4.440892098500626e-16,
    "gershgorin0": 4.440892098500626e-16,
    "gershgorin255": 4.440892098500626e-16,
    "gershgorin256": 4.440892098500626e-16,
    "gershgorin262400": 4.440892098500626e-16,
}

if __name__ == "__main__":
    if sys.argv[1:] == ["chain4"]:
        print(f'"{CHAIN4.name}": {measure_chain4_row()!r},')
    else:
        print("TABLE = {")
        for nm in CASES:
            print(f'    "{nm}": {measure_row(nm)!r},')
        print("}")
