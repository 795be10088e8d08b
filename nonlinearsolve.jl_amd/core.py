"""Host-side mirror of the reference's interface for the first-order step path, above the C ABI.

The names, argument meaning and error behaviour follow NonlinearSolve.jl so that the parity tests read like
the reference's own tests:

    prob = NonlinearProblem(NonlinearFunction(f!; jvp = jvp!), u0, p)          # SciMLBase
    sol  = solve(prob, NewtonRaphson(; linsolve = KrylovJL_GMRES(), forcing = EisenstatWalkerForcing2());
                 abstol = 1e-8)                                                 # lib/NonlinearSolveFirstOrder
    cache = init(prob, TrustRegion(; linsolve = KrylovJL_GMRES())); step!(cache); solve!(cache); reinit!(cache, u0; p)
    J = StatefulJacobianOperator(JacobianOperator(prob, fu, u), u, p);  J * v;  J' * v   # lib/SciMLJacobianOperators

Everything numerical happens in libmi355x_nk.so (HIP kernels); this file only marshals pointers. Vectors may
be NumPy arrays (host; copied per call) or torch CUDA tensors (device; zero-copy). torch is used for device
memory and streams only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Callable, Optional, Sequence

import numpy as np

from . import _lib as L
from ._lib import NKError, check

try:  # torch is plumbing: device buffers + current stream
    import torch
except Exception:  # pragma: no cover
    torch = None


# ------------------------------------------------------------------------------------------- pointers
def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _ptr(x, n: Optional[int] = None):
    """(address, memspace, keepalive) of a float64 vector."""
    if _is_torch(x):
        if x.dtype != torch.float64:
            raise TypeError("device vectors must be float64")
        if not x.is_contiguous():
            raise ValueError("device vectors must be contiguous")
        if n is not None and x.numel() != n:
            raise ValueError(f"expected {n} elements, got {x.numel()}")
        return C.c_void_p(x.data_ptr()), (L.DEVICE if x.is_cuda else L.HOST), x
    a = np.ascontiguousarray(x, dtype=np.float64)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} elements, got {a.size}")
    return C.c_void_p(a.ctypes.data), L.HOST, a


def _like(x, n: int):
    if _is_torch(x):
        return torch.empty(n, dtype=torch.float64, device=x.device)
    return np.empty(n, dtype=np.float64)


class _DevView:
    """Zero-copy torch view of a raw device pointer handed to a callback (via __cuda_array_interface__)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


def _view(ptr, n):
    return torch.as_tensor(_DevView(ptr, n), device="cuda")


# ------------------------------------------------------------------------------------------- context
class Context:
    """nk_ctx: one HIP device + stream (+ communicator). One process per GPU."""

    def __init__(self, device: Optional[int] = None, stream: Optional[int] = None):
        lib = L.lib()
        if device is None:
            device = torch.cuda.current_device() if (torch is not None and torch.cuda.is_available()) else 0
        if stream is None and torch is not None and torch.cuda.is_available():
            stream = torch.cuda.current_stream(device).cuda_stream
        h = C.c_void_p()
        check(lib.nk_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h, self.device = h, int(device)
        self._keep = []

    def synchronize(self):
        check(L.lib().nk_ctx_synchronize(self._h))

    def set_deterministic(self, flag: bool = True):
        check(L.lib().nk_ctx_set_deterministic(self._h, int(bool(flag))))

    def set_halo_overlap(self, flag: bool = True):
        """Multi-rank CSR SpMV: halo exchange on a second stream, overlapped with the interior row blocks."""
        check(L.lib().nk_ctx_set_halo_overlap(self._h, int(bool(flag))))

    # -- per-kernel-family HIP-event timing (bench.py roofline evidence)
    def profile_enable(self, on: bool = True):
        check(L.lib().nk_ctx_profile_enable(self._h, int(bool(on))))

    def profile_report(self):
        out = {}
        for k in range(L.lib().nk_ctx_profile_kernel_count()):
            name, cnt, ms, by = C.c_char_p(), C.c_int64(), C.c_double(), C.c_double()
            check(L.lib().nk_ctx_profile_query(self._h, k, C.byref(name), C.byref(cnt), C.byref(ms), C.byref(by)))
            if cnt.value:
                out[name.value.decode()] = dict(launches=cnt.value, total_ms=ms.value, bytes=by.value,
                                                avg_us=1e3 * ms.value / cnt.value,
                                                gbps=by.value / (ms.value * 1e-3) / 1e9 if ms.value > 0 else 0.0)
        return out

    # -- communicator
    def comm_init_rccl(self, nranks: int, rank: int, unique_id: bytes):
        check(L.lib().nk_ctx_comm_init_rccl(self._h, nranks, rank, unique_id))

    def comm_init_callbacks(self, nranks: int, rank: int, allreduce: Callable, alltoallv: Callable):
        cb = L.CommCallbacks(L.ALLREDUCE_FN(allreduce), L.ALLTOALLV_FN(alltoallv), None)
        self._keep.append(cb)
        check(L.lib().nk_ctx_comm_init_callbacks(self._h, nranks, rank, C.byref(cb)))

    def comm_peer_handle(self, arena_bytes: int = 0) -> bytes:
        """Allocate this rank's uncached arena and return its 64-byte hipIpc handle (all-gather it, then comm_enable_peer)."""
        buf = C.create_string_buffer(64)
        check(L.lib().nk_ctx_comm_peer_handle(self._h, int(arena_bytes), buf))
        return buf.raw

    def comm_enable_peer(self, handles: bytes):
        check(L.lib().nk_ctx_comm_enable_peer(self._h, handles))

    def comm_peer_disable(self):
        check(L.lib().nk_ctx_comm_peer_disable(self._h))

    def comm_peer_selftest(self) -> bool:
        ok = C.c_int()
        check(L.lib().nk_ctx_comm_peer_selftest(self._h, C.byref(ok)))
        return bool(ok.value)

    def comm_peer_status(self):
        en, err = C.c_int(), C.c_int64()
        check(L.lib().nk_ctx_comm_peer_status(self._h, C.byref(en), C.byref(err)))
        return bool(en.value), int(err.value)

    def allreduce(self, x, op: str = "sum"):
        """in-place all-reduce of a float64 device tensor over the ranks, through the context's transport; returns x"""
        check(L.lib().nk_ctx_comm_allreduce(self._h, C.c_void_p(x.data_ptr()), int(x.numel()), {"sum": 0, "max": 1}[op]))
        return x

    def comm_info(self):
        k, n, r = C.c_int(), C.c_int(), C.c_int()
        check(L.lib().nk_ctx_comm_info(self._h, C.byref(k), C.byref(n), C.byref(r)))
        return k.value, n.value, r.value

    def comm_device_shared(self) -> bool:
        """several ranks of the communicator run on one device (processes time-slicing a GPU)"""
        s = C.c_int(0)
        check(L.lib().nk_ctx_comm_device_shared(self._h, C.byref(s)))
        return bool(s.value)

    def close(self):
        if self._h:
            L.lib().nk_ctx_destroy(self._h)
            self._h = None

    # -- BLAS-1 on device tensors
    def dot(self, x, y):
        r = C.c_double()
        check(L.lib().nk_dot(self._h, x.numel(), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.byref(r)))
        return r.value

    def nrm2(self, x):
        r = C.c_double()
        check(L.lib().nk_nrm2(self._h, x.numel(), C.c_void_p(x.data_ptr()), C.byref(r)))
        return r.value

    def norm_inf(self, x):
        r = C.c_double()
        check(L.lib().nk_norm_inf(self._h, x.numel(), C.c_void_p(x.data_ptr()), C.byref(r)))
        return r.value

    def axpy(self, a, x, y):
        check(L.lib().nk_axpy(self._h, x.numel(), float(a), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())))

    def multidot(self, V, w):
        """V: (nv, ldv) row-major torch tensor = column-major n×nv basis; returns h[j] = V[j]·w."""
        nv, ldv = V.shape
        h = (C.c_double * nv)()
        check(L.lib().nk_multidot(self._h, w.numel(), nv, C.c_void_p(V.data_ptr()), ldv, C.c_void_p(w.data_ptr()), h))
        return np.array(h[:])

    def multiaxpy(self, V, h, w, want_norm2=False):
        nv, ldv = V.shape
        hh = (C.c_double * nv)(*[float(t) for t in h])
        r = C.c_double()
        check(L.lib().nk_multiaxpy(self._h, w.numel(), nv, C.c_void_p(V.data_ptr()), ldv, hh,
                                   C.c_void_p(w.data_ptr()), C.byref(r) if want_norm2 else None))
        return r.value if want_norm2 else None


def _fused_axpy_dot(self, V, h, s, w):
    """w -= V (h∘s); returns (h2, ‖w_new‖²) with h2[j] = s_j V[j]·w_new — the fused CGS2 pass."""
    nv, ldv = V.shape
    hh = (C.c_double * nv)(*[float(t) for t in h])
    ss = (C.c_double * nv)(*[float(t) for t in s])
    out = (C.c_double * (nv + 1))()
    check(L.lib().nk_fused_axpy_dot(self._h, w.numel(), nv, C.c_void_p(V.data_ptr()), ldv, hh, ss,
                                    C.c_void_p(w.data_ptr()), out))
    arr = np.array(out[:])
    return arr[:nv], float(arr[nv])


Context.fused_axpy_dot = _fused_axpy_dot

_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def set_default_context(ctx: Optional[Context]):
    global _default_ctx
    _default_ctx = ctx


def partition_range(n_global: int, granule: int, nranks: int, rank: int):
    b, e = C.c_int64(), C.c_int64()
    check(L.lib().nk_partition_range(n_global, granule, nranks, rank, C.byref(b), C.byref(e)))
    return b.value, e.value


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(L.lib().nk_comm_unique_id(buf))
    return buf.raw


# ------------------------------------------------------------------------------------------- CSR
class CSRMatrix:
    """nk_csr: row-partitioned CSR with f64 values / i32 indices on the device (SparseMatrixCSC stand-in)."""

    def __init__(self, handle, ctx: Context, owned=True):
        self._h, self.ctx, self._owned = handle, ctx, owned

    @classmethod
    def from_arrays(cls, rowptr, colind, vals=None, n_global=None, row_begin=0, index_base=0, ctx=None):
        ctx = ctx or default_context()
        rowptr = np.ascontiguousarray(rowptr)
        colind = np.ascontiguousarray(colind)
        if rowptr.dtype not in (np.int32, np.int64):
            rowptr = rowptr.astype(np.int64)
        colind = colind.astype(rowptr.dtype, copy=False)
        bits = 32 if rowptr.dtype == np.int32 else 64
        nrows = rowptr.size - 1
        nnz = int(colind.size)
        if n_global is None:
            n_global = nrows
        v = None if vals is None else np.ascontiguousarray(vals, dtype=np.float64)
        h = C.c_void_p()
        check(L.lib().nk_csr_create(ctx._h, nrows, n_global, row_begin, nnz, bits, index_base,
                                    C.c_void_p(rowptr.ctypes.data), C.c_void_p(colind.ctypes.data),
                                    None if v is None else C.c_void_p(v.ctypes.data), L.HOST, C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_scipy(cls, A, ctx=None):
        A = A.tocsr()
        A.sort_indices()
        return cls.from_arrays(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, ctx=ctx)

    def set_values_csc(self, nzval):
        """New values in the CSC order of `from_csc` (Julia: `nonzeros(J)` after `f.jac(J, u, p)`): one gather on the device
        through the permutation remembered at creation — no new conversion, no new pattern upload."""
        if _is_torch(nzval) and nzval.is_cuda:
            check(L.lib().nk_csr_set_values_csc(self._h, C.c_void_p(nzval.data_ptr()), int(nzval.numel()), L.DEVICE))
        else:
            v = np.ascontiguousarray(nzval.cpu().numpy() if _is_torch(nzval) else nzval, dtype=np.float64)
            check(L.lib().nk_csr_set_values_csc(self._h, C.c_void_p(v.ctypes.data), int(v.size), L.HOST))
        return self

    @classmethod
    def from_csc(cls, colptr, rowval, nzval, index_base=1, ctx=None, row_range=None):
        """Julia's SparseMatrixCSC fields (1-based Int64 by default) of the whole matrix; on several ranks this rank keeps
        `row_range = (begin, end)` (default: the library's contiguous partition)."""
        ctx = ctx or default_context()
        colptr = np.ascontiguousarray(colptr, dtype=np.int64)
        rowval = np.ascontiguousarray(rowval, dtype=np.int64)
        nz = np.ascontiguousarray(nzval, dtype=np.float64)
        h = C.c_void_p()
        if row_range is None:
            check(L.lib().nk_csr_create_from_csc(ctx._h, colptr.size - 1, rowval.size, 64, index_base,
                                                 C.c_void_p(colptr.ctypes.data), C.c_void_p(rowval.ctypes.data),
                                                 C.c_void_p(nz.ctypes.data), C.byref(h)))
        else:
            check(L.lib().nk_csr_create_from_csc_rows(ctx._h, colptr.size - 1, rowval.size, 64, index_base,
                                                      C.c_void_p(colptr.ctypes.data), C.c_void_p(rowval.ctypes.data),
                                                      C.c_void_p(nz.ctypes.data), int(row_range[0]),
                                                      int(row_range[1] - row_range[0]), C.byref(h)))
        return cls(h, ctx)

    def info(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        check(L.lib().nk_csr_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(nrows_local=a.value, n_global=b.value, nnz=c.value, n_halo=d.value)

    @property
    def shape(self):
        i = self.info()
        return (i["nrows_local"], i["n_global"])

    def set_values(self, vals):
        p, ms, _k = _ptr(vals, self.info()["nnz"])
        check(L.lib().nk_csr_set_values(self._h, p, ms))

    def values(self):
        out = np.empty(self.info()["nnz"])
        check(L.lib().nk_csr_get_values(self._h, C.c_void_p(out.ctypes.data), L.HOST))
        return out

    def values_device(self):
        return _view(L.lib().nk_csr_values_device(self._h), self.info()["nnz"])

    def matvec(self, x, out=None):
        n = self.info()["nrows_local"]
        px, ms, _k = _ptr(x, n)
        y = _like(x, n) if out is None else out
        py, ms2, _k2 = _ptr(y, n)
        if ms != ms2:
            raise ValueError("x and out must live in the same memory space")
        check(L.lib().nk_spmv(self._h, px, py, ms))
        return y

    def powers(self, x, s, theta=None, scale=1.0):
        """Matrix powers Y[:, p] = scale·(A − θ_p I) Y[:, p−1], Y[:, −1] = x (theta None: plain powers) — the s operator
        applications of an s-step Arnoldi block. Returns (Y as an (s, n) array whose row p is power p, resident) where
        `resident` says whether the one-launch kernel that holds the matrix in registers ran (csrc/nk_powers.hip)."""
        n = self.info()["nrows_local"]
        px, ms, _k = _ptr(x, n)
        Y = _like(x, n * s)
        pY, _ms2, _k2 = _ptr(Y, n * s)
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        if th is not None and th.size != s:
            raise ValueError("theta must have s entries")
        res = C.c_int(0)
        check(L.lib().nk_csr_powers(self._h, px, pY, n, int(s), None if th is None else C.c_void_p(th.ctypes.data),
                                    float(scale), ms, C.byref(res)))
        return Y.reshape(s, n), bool(res.value)

    @staticmethod
    def powers_layout(A, num_cus: int = 256):
        """Which form of the resident matrix-powers kernel a SciPy CSR pattern fits on a device with `num_cus` compute units
        (host arithmetic only, nk_csr_powers_layout): dict(kind = 'none' | 'bands' | 'segments', slices, slots, bands, segments, ring)"""
        import numpy as _np
        A = A.tocsr()
        rp = _np.ascontiguousarray(A.indptr, dtype=_np.int32)
        ci = _np.ascontiguousarray(A.indices, dtype=_np.int32)
        out = (C.c_int * 6)()
        check(L.lib().nk_csr_powers_layout(int(A.shape[0]), C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data), int(num_cus), out))
        return {"kind": ("none", "bands", "segments")[out[0]], "slices": out[1], "slots": out[2], "bands": out[3],
                "segments": out[4], "ring": bool(out[5])}

    def rmatvec(self, x, out=None):
        n = self.info()["nrows_local"]
        px, ms, _k = _ptr(x, n)
        y = _like(x, n) if out is None else out
        py, _ms2, _k2 = _ptr(y, n)
        check(L.lib().nk_spmv_t(self._h, px, py, ms))
        return y

    def colsumsq(self, like=None):
        """diag(AᵀA): out_j = Σ_i A_ij² (LevenbergMarquardt's DᵀD source, levenberg_marquardt.jl:133-148)."""
        n = self.info()["nrows_local"]
        y = np.empty(n) if like is None else _like(like, n)
        py, ms, _k = _ptr(y, n)
        check(L.lib().nk_csr_colsumsq(self._h, py, ms))
        return y

    __matmul__ = matvec

    def close(self):
        if self._h and self._owned:
            L.lib().nk_csr_destroy(self._h)
        self._h = None


# ------------------------------------------------------------------------------------------- problems
class DeviceProblem:
    """nk_problem: residual / JVP / VJP / Jacobian provider living on the device."""

    def __init__(self, handle, ctx: Context, keep=()):
        self._h, self.ctx, self._keep = handle, ctx, list(keep)
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(L.lib().nk_problem_size(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_local, self.n_global, self.row_begin = a.value, b.value, c.value

    def residual(self, u):
        f = _like(u, self.n_local)
        pu, ms, _a = _ptr(u, self.n_local)
        pf, _m, _b = _ptr(f)
        check(L.lib().nk_residual(self._h, pu, pf, ms))
        return f

    def _jv(self, fn, u, v):
        out = _like(u, self.n_local)
        pu, ms, _a = _ptr(u, self.n_local)
        pv, ms2, _b = _ptr(v, self.n_local)
        po, _m, _c = _ptr(out)
        if ms != ms2:
            raise ValueError("u and v must live in the same memory space")
        check(fn(self._h, pu, pv, po, ms))
        return out

    def jvp(self, v, u):  # argument order of the reference: jvp(v, u, p)
        return self._jv(L.lib().nk_jvp, u, v)

    def vjp(self, v, u):
        return self._jv(L.lib().nk_vjp, u, v)

    def jac_csr(self) -> CSRMatrix:
        h = C.c_void_p()
        check(L.lib().nk_problem_jac_csr(self._h, C.byref(h)))
        return CSRMatrix(h, self.ctx)

    def jac_values(self, u, J: CSRMatrix, colored: bool = False):
        pu, ms, _a = _ptr(u, self.n_local)
        if colored:
            nc = C.c_int()
            check(L.lib().nk_jac_values_colored(self._h, pu, ms, J._h, C.byref(nc)))
            return nc.value
        check(L.lib().nk_jac_values(self._h, pu, ms, J._h))
        return None

    def initial_guess(self, device: bool = False):
        u0 = torch.empty(self.n_local, dtype=torch.float64, device=f"cuda:{self.ctx.device}") if device \
            else np.empty(self.n_local)
        p, ms, _a = _ptr(u0)
        check(L.lib().nk_problem_initial_guess(self._h, p, ms))
        return u0

    def set_params(self, params: Sequence[float]):
        arr = (C.c_double * len(params))(*[float(x) for x in params])
        check(L.lib().nk_problem_set_params(self._h, arr, len(params)))

    def close(self):
        if self._h:
            L.lib().nk_problem_destroy(self._h)
            self._h = None


def _builtin(kind, params, ctx):
    ctx = ctx or default_context()
    arr = (C.c_double * len(params))(*[float(x) for x in params])
    h = C.c_void_p()
    check(L.lib().nk_problem_create(ctx._h, kind, arr, len(params), C.byref(h)))
    return DeviceProblem(h, ctx)


def Quadratic(n: int, p: float = 2.0, ctx=None) -> DeviceProblem:
    """quadratic_f(u, p) = u .* u .- p   (common/common_rootfind_testing.jl:15-17)"""
    P = _builtin(L.PROBLEM_QUADRATIC, [n, p], ctx)
    P.params = [n, p]
    return P


def Bratu2D(n: int, lam: float = 6.0, scale: float = 0.0, ctx=None) -> DeviceProblem:
    """2-D Bratu, 5-point stencil; scale = 0 → h²-scaled residual."""
    P = _builtin(L.PROBLEM_BRATU2D, [n, lam, scale], ctx)
    P.params = [n, lam, scale]
    return P


def Brusselator2D(N: int, A=3.4, B=1.0, alpha=10.0, dx=None, ctx=None) -> DeviceProblem:
    """brusselator_2d_loop (lib/NonlinearSolveFirstOrder/test/sparsity_tests__item1.jl:13-36)"""
    dx = 1.0 / (N - 1) if dx is None else dx
    P = _builtin(L.PROBLEM_BRUSSELATOR2D, [N, A, B, alpha, dx], ctx)
    P.params = [N, A, B, alpha, dx]
    return P


# ------------------------------------------------------------------------------------------- compiled grid problems
def _grid_boundary(boundary, dim):
    """the library's boundary code of boundary=: one of the two old strings, a tuple of 2·dim kinds (x-lo, x-hi, y-lo, y-hi[,
    z-lo, z-hi]) or a dict {"x": kind | (lo, hi), ...} whose missing axes are "dirichlet" """
    if isinstance(boundary, str):
        if boundary not in L.GRID_BOUNDARIES:
            raise ValueError(f"boundary = {boundary!r}: expected one of {sorted(L.GRID_BOUNDARIES)}, a tuple of {2 * dim} kinds "
                             f"from {sorted(L.GRID_SIDE_KINDS)}, or a dict by axis")
        return L.GRID_BOUNDARIES[boundary]
    if isinstance(boundary, dict):
        axes = "xyz"[:dim]
        if any(a not in axes for a in boundary):
            raise ValueError(f"boundary = {boundary!r}: the axes of a {dim}-D grid are {list(axes)}")
        sides = []
        for a in axes:
            k = boundary.get(a, "dirichlet")
            sides += [k, k] if isinstance(k, str) else list(k)
    else:
        sides = list(boundary)
    if len(sides) != 2 * dim:
        raise ValueError(f"boundary = {boundary!r}: a {dim}-D grid has {2 * dim} sides (lo and hi of every axis)")
    for k in sides:
        if k not in L.GRID_SIDE_KINDS:
            raise ValueError(f"boundary side {k!r}: expected one of {sorted(L.GRID_SIDE_KINDS)}")
    return L.grid_sides(*[L.GRID_SIDE_KINDS[k] for k in sides])


def _grid_ids(stencil, boundary, dim=2):
    if stencil not in L.GRID_STENCILS:
        raise ValueError(f"stencil = {stencil!r}: expected one of {sorted(L.GRID_STENCILS)}")
    return L.GRID_STENCILS[stencil], _grid_boundary(boundary, dim)


def grid_pattern(nx: int, ny: int, dof: int = 1, stencil: str = "star", boundary="dirichlet", *, nz: Optional[int] = None):
    """(rowptr, colind), int32, of the Jacobian of a compiled grid problem: columns ascending within a row, every
    (stencil point in the domain) × (component) entry kept. Host only. With nz: the nx × ny × nz grid (7-point star or
    27-point box). stencil = "star2" / "diamond2": the radius-2 stencils of CompiledGridProblem (every side >= 5). boundary: as
    for CompiledGridProblem; at a mirror side the stencil points of a row that land on one node share one column."""
    st, bd = _grid_ids(stencil, boundary, 2 if nz is None else 3)
    nnz = C.c_int64()
    if nz is None:
        def pattern(rp, ci):
            return L.lib().nk_grid_pattern(nx, ny, dof, st, bd, rp, ci, C.byref(nnz))
    else:
        def pattern(rp, ci):
            return L.lib().nk_grid3_pattern(nx, ny, nz, dof, st, bd, rp, ci, C.byref(nnz))
    check(pattern(None, None))
    rowptr = np.empty(dof * nx * ny * (1 if nz is None else nz) + 1, dtype=np.int32)
    colind = np.empty(nnz.value, dtype=np.int32)
    check(pattern(C.c_void_p(rowptr.ctypes.data), C.c_void_p(colind.ctypes.data)))
    return rowptr, colind


def grid_mg_axis(n: int, lo: str = "dirichlet", hi: str = "dirichlet"):
    """(nc, idx, w): the folded prolongation table of one axis of n nodes with the side kinds lo, hi ("dirichlet", "periodic",
    "mirror_node", "mirror_face") onto the coarser axis of nc nodes that the multigrid `precs` of a compiled grid problem builds
    (MultigridPrecs): fine node i takes w[i, 0] of coarse node idx[i, 0] and w[i, 1] of idx[i, 1]; a dropped entry (outside a
    Dirichlet side, merged into the other one at a mirror, or of weight 0) has the index −1 and the weight 0. Host only."""
    for k in (lo, hi):
        if k not in L.GRID_SIDE_KINDS:
            raise ValueError(f"side kind {k!r}: expected one of {sorted(L.GRID_SIDE_KINDS)}")
    nc = C.c_int64()
    idx, w = np.empty((int(n), 2), dtype=np.int32), np.empty((int(n), 2), dtype=np.float64)
    check(L.lib().nk_grid_mg_axis(int(n), L.GRID_SIDE_KINDS[lo], L.GRID_SIDE_KINDS[hi], C.byref(nc), C.c_void_p(idx.ctypes.data),
                                  C.c_void_p(w.ctypes.data)))
    return nc.value, idx, w


def _slab_lines(n_outer: int, nranks: int):
    """the first line (plane) of every rank's slab and the end: nk_partition_range(n_outer, 1, R, r)"""
    return [partition_range(n_outer, 1, nranks, r)[0] for r in range(nranks)] + [n_outer]


def _slab_permutation(nx, ny, nz, dof, nranks):
    """perm[g] = the one-rank index c·nn + node of the unknown with the global (rank-contiguous) index g: slab after slab,
    component-major on each"""
    line, n_outer = (nx, ny) if nz is None else (nx * ny, nz)
    nn, begin = line * n_outer, _slab_lines(n_outer, nranks)
    return np.concatenate([c * nn + np.arange(begin[r] * line, begin[r + 1] * line, dtype=np.int64)
                           for r in range(nranks) for c in range(dof)])


def grid_slab_pattern(nx: int, ny: int, dof: int = 1, stencil: str = "star", boundary="dirichlet", *, nz: Optional[int] = None,
                      nranks: int, rank: int):
    """(lines, rowptr, colind): the slab of rank `rank` of `nranks` of a compiled grid problem — lines = (l0, l1) of the
    outermost axis (y; with nz: z), nk_partition_range's — and its rows of the Jacobian's pattern: rowptr int32 over the slab's
    dof·nn_loc rows in local order (c·nn_loc + slab node), colind int64 in the global, rank-contiguous numbering (row_begin of
    the owner + c·nn_loc of the owner + node within its slab), ascending within a row. Host only. A slab thinner than
    radius + 1 lines raises NKError (NK_E_INVALID). nranks = 1: grid_pattern's."""
    dim = 2 if nz is None else 3
    st, bd = _grid_ids(stencil, boundary, dim)
    nnz, l0, l1 = C.c_int64(), C.c_int64(), C.c_int64()

    def pattern(rp, ci):
        return L.lib().nk_grid_slab_pattern(dim, nx, ny, 1 if nz is None else nz, dof, st, bd, int(nranks), int(rank),
                                            C.byref(l0), C.byref(l1), rp, ci, C.byref(nnz))
    check(pattern(None, None))
    nn_loc = (l1.value - l0.value) * (nx if nz is None else nx * ny)
    rowptr = np.empty(dof * nn_loc + 1, dtype=np.int32)
    colind = np.empty(nnz.value, dtype=np.int64)
    check(pattern(C.c_void_p(rowptr.ctypes.data), C.c_void_p(colind.ctypes.data)))
    return (l0.value, l1.value), rowptr, colind


def grid_compile_check(source: str, dof: int = 1, stencil: str = "star", boundary="dirichlet", nparams: int = 0, *,
                       dim: int = 2, fields: int = 0, nranks: int = 1, rank: int = 0) -> int:
    """Compile the residual, JVP and Jacobian kernels of `source` for gfx950 (no device needed); the size of the code objects.
    A source that does not compile raises NKError with the contract and the compiler's log. dim = 3: the 3-D contract
    (nk_nbhd3, nk_site3). stencil = "star2" / "diamond2": the radius-2 neighbourhoods (offsets in −2 … 2). fields = 1..4: the
    contract with the field argument `const nk_flds &a` (3-D: nk_flds3) of CompiledGridProblem(..., fields=). nranks, rank:
    the programs of that rank of a grid split over several — its sides of the outermost axis that are cuts between two ranks
    read ghost lines; nranks = 1 are the programs of one rank."""
    if dim not in (2, 3):
        raise ValueError(f"dim = {dim!r}: expected 2 or 3")
    st, bd = _grid_ids(stencil, boundary, dim)
    nb = C.c_int64()
    if nranks != 1:
        check(L.lib().nk_grid_slab_compile_check(source.encode(), dim, dof, st, bd, nparams, int(fields), int(nranks), int(rank),
                                                 C.byref(nb)))
        return nb.value
    if fields:
        check(L.lib().nk_grid_fields_compile_check(source.encode(), dim, dof, st, bd, nparams, int(fields), C.byref(nb)))
        return nb.value
    fn = L.lib().nk_grid3_compile_check if dim == 3 else L.lib().nk_grid_compile_check
    check(fn(source.encode(), dof, st, bd, nparams, C.byref(nb)))
    return nb.value


def _params_array(params):
    """(the parameters as floats, a c_double array of them with at least one element)"""
    params = [float(x) for x in params]
    return params, (C.c_double * max(len(params), 1))(*params)


def _sized_call(fn, args, shapes):
    """a two-pass pattern function of the library, fn(*args, a, b, &count): once for the count, then into int32 arrays of
    shapes(count) = the two lengths"""
    cnt = C.c_int64()
    check(fn(*args, None, None, C.byref(cnt)))
    a, b = (np.empty(m, dtype=np.int32) for m in shapes(cnt.value))
    check(fn(*args, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.byref(cnt)))
    return a, b


class _CompiledDeviceProblem(DeviceProblem):
    """the nk_problem of a compiled grid, graph or element problem: the Jacobian pattern belongs to the problem, `p` is the
    source's whole p, and its read-only data arrays live in device buffers the problem owns"""

    def jac_csr(self) -> CSRMatrix:
        h = C.c_void_p()
        check(L.lib().nk_problem_jac_csr(self._h, C.byref(h)))
        return CSRMatrix(h, self.ctx, owned=False)   # freed with the problem

    def set_p(self, p):
        p = [float(p)] if isinstance(p, (int, float)) else [float(x) for x in p]
        if len(p) != len(self.p):
            raise ValueError(f"the source was compiled for {len(self.p)} parameters, got {len(p)}")
        self.set_params(p)
        self.p = p

    def _set_datum(self, setter, index, x, n, what):
        """x (n elements, a device tensor or a NumPy array) through setter(problem, *index, pointer, memspace)"""
        size = x.numel() if _is_torch(x) else np.size(x)
        if size != n:
            raise ValueError(f"{what}, got {size}")
        px, ms, _keep = _ptr(x, n) if n else (None, L.HOST, None)
        check(setter(self._h, *index, px, ms))

    def _get_datum(self, getter, index, n):
        """a device tensor of n elements filled by getter(problem, *index, pointer, memspace)"""
        out = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        check(getter(self._h, *index, C.c_void_p(out.data_ptr()), L.DEVICE))
        return out


class _GridDeviceProblem(_CompiledDeviceProblem):
    """the nk_problem of CompiledGridProblem"""

    nfields = 0   # CompiledGridProblem(..., fields=k)

    lines = (0, 0)   # the lines (3-D: planes) [l0, l1) of the outermost axis this rank owns; one rank: all of them

    @property
    def nn(self) -> int:
        """nodes of this rank's slab (one rank: of the grid): the length of a field"""
        return self.nx * (self.lines[1] - self.lines[0]) * (self.ny if hasattr(self, "nz") else 1)

    def _local_index(self):
        """the one-rank index c·nn + node of every local unknown, in local order"""
        line = self.nx * (self.ny if hasattr(self, "nz") else 1)
        nn = line * (self.nz if hasattr(self, "nz") else self.ny)
        return np.concatenate([c * nn + np.arange(self.lines[0] * line, self.lines[1] * line, dtype=np.int64)
                               for c in range(self.dof)])

    def local_of(self, full):
        """this rank's local vector (c·nn_loc + slab node) of an array in one-rank order (c·nn + node); a torch tensor stays one"""
        idx = self._local_index()
        return full[torch.as_tensor(idx, device=full.device)] if _is_torch(full) else np.asarray(full)[idx]

    def to_full(self, gathered):
        """the inverse on a gathered global vector (rank-contiguous: dist.gather_vector's): the array in one-rank order"""
        perm = _slab_permutation(self.nx, self.ny, getattr(self, "nz", None), self.dof, self.ctx.comm_info()[1])
        gathered = np.asarray(gathered)
        out = np.empty_like(gathered)
        out[perm] = gathered
        return out

    def set_field(self, k: int, x):
        """Replace field k (0 .. nfields − 1) by x: a torch tensor on the device or a NumPy array with one float64 per node of
        this rank's slab (one rank: per grid node), node (i, j[, k]) at (k·ny + j)·nx + i with the slab's own lines. The data
        is copied; a Jacobian cached for the same u is filled again. On several ranks the call is collective: the ghost lines
        of the field are exchanged here, once."""
        self._set_datum(L.lib().nk_problem_set_field, (int(k),), x, self.nn,
                        f"field {k}: expected {self.nn} elements (one per node of the rank's slab)")

    def field(self, k: int):
        """a copy of field k as a device tensor"""
        return self._get_datum(L.lib().nk_problem_get_field, (int(k),), self.nn)


def CompiledGridProblem(source: str, nx: int, ny: int, dof: int = 1, stencil: str = "star", boundary="dirichlet",
                        params: Sequence[float] = (), ctx=None, *, nz: Optional[int] = None, fields: int = 0) -> DeviceProblem:
    """A residual given pointwise on an nx × ny grid through a radius-1 or radius-2 stencil, as HIP source
        template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f);
    compiled (hiprtc, gfx950) into the residual kernel, the exact dual-number JVP kernel and the Jacobian fill on the stencil's
    CSR pattern (include/mi355x_nk.h, "compiled grid problems"). u0 defaults to zeros; NonlinearProblem(..., p) and
    reinit_(cache, p=...) replace the source's p[0..nparams). dof <= 4 (box: <= 2), Float64.
    Several ranks: on a context with a communicator of R > 1 ranks the grid is split into slabs along its outermost axis (y; with
    nz: z) and the call is collective. P.lines = (l0, l1) are this rank's lines (planes), nk_partition_range(n_outer, 1, R, r);
    every slab has at least radius + 1 of them (else NKError). Local vectors — u, f, v, what P.residual takes and returns — are
    component-major on the slab, element c·P.nn + slab node with P.nn the slab's nodes; the global numbering is P.row_begin +
    local, slab after slab. P.local_of(full) slices an array in one-rank order (c·nn + node) to the local vector,
    P.to_full(gathered) turns a gathered global vector back, dist.gather_grid(P, local) does both steps. The source still sees
    the site on the whole grid (s.j, s.ny; 3-D s.k, s.nz). Fields are split like u: set_field takes and field returns the slab.
    With nz the grid is nx × ny × nz and the source follows the 3-D contract
        template <typename T> __device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f);
    with u(di, dj, dk, c): the 7-point star (dof <= 4) or the 27-point box (dof = 1).
    Radius 2: stencil = "star2" — the points (0,±1) (0,±2) (±1,0) (±2,0) and the centre, in 3-D the 13-point star; dof <= 2 —
    and stencil = "diamond2" — the 13 points with |di| + |dj| <= 2, the support of the discrete biharmonic; 2-D only, dof = 1.
    Offsets then run over −2 … 2, a read outside the stencil's shape gives NaN, a Dirichlet neighbour up to two layers outside
    the grid reads 0, a periodic index wraps by ± n, and every side is >= 5.
    Fields: with fields = 1..4 the problem owns that many read-only arrays of one double per node (a previous time level, a
    coefficient, a source term) and the source takes one more argument after u,
        template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, nk_site s, T *f);
    (3-D: const nk_nbhd3<T> &u, const nk_flds3 &a, …, nk_site3 s) where a(di, dj, k = 0) — 3-D a(di, dj, dk, k = 0) — is field k
    at the neighbouring node: an nk_real, never a dual, so fields add no column and no partial. Offsets and the NaN rule are
    the stencil's own. At a periodic boundary the index wraps; outside a Dirichlet boundary a field reads as the field at the
    node itself (u reads 0 there), so a face coefficient 0.5·(a(0,0) + a(1,0)) becomes a(0,0) at the wall; a source that
    wants something else tests s. Fields are zero until P.set_field(k, x) — x a device tensor or a NumPy array of nx·ny[·nz]
    doubles, copied — and P.field(k) returns a device copy; P.nfields is their number. A field the source declares and does
    not read costs nothing. Implicit time stepping, F(u) = (u − u_old)/dt − L(u) with u_old = a(0, 0, 0):
        cache = init(NonlinearProblem(P, u0), alg)
        for step in range(nsteps):
            P.set_field(0, cache.u); reinit_(cache, u0=cache.u); solve_(cache)
    Boundaries: boundary = "dirichlet" or "periodic" for the whole grid, or a kind per side — a tuple of 2·dim strings (x-lo,
    x-hi, y-lo, y-hi[, z-lo, z-hi]) or a dict {"x": kind | (lo, hi), ...} whose missing axes are "dirichlet" — from
    "dirichlet" (a ghost reads 0, no column), "periodic" (both sides of the axis), "mirror_node" (the wall is the outermost
    node: −k ↦ k, NumPy's reflect) and "mirror_face" (the wall is half a cell outside: −k ↦ k−1, NumPy's symmetric — the
    zero-flux wall of a cell-centred grid). Axes are independent; a point that leaves through a Dirichlet side of any axis
    reads 0. A mirrored ghost is another unknown: J is the true dF/du, the partials of the stencil points of a row that land
    on one node are added into one entry, and u, v and the fields are read at the mirrored node. A channel:
    boundary={"x": "periodic", "y": "mirror_face"}. P.boundary keeps what was passed.
    Multigrid: on one rank KrylovJL_GMRES(precs=MultigridPrecs(nu, coarse_max)) and GMRES.set_multigrid_preconditioner take a
    compiled grid problem; the levels are this problem on smaller grids — the same source, the same code objects, p copied, u
    and the fields restricted. A source used that way takes its spacing from the site, h = 1/(s.nx + 1) and the like, not from p:
    s.nx, s.ny[, s.nz] are the sides of the level the kernel runs on (see MultigridPrecs)."""
    ctx = ctx or default_context()
    st, bd = _grid_ids(stencil, boundary, 2 if nz is None else 3)
    params, arr = _params_array(params)
    h = C.c_void_p()
    if fields:
        check(L.lib().nk_problem_create_grid_fields(ctx._h, source.encode(), nx, ny, 0 if nz is None else nz, dof, st, bd, arr,
                                                    len(params), int(fields), C.byref(h)))
    elif nz is None:
        check(L.lib().nk_problem_create_grid(ctx._h, source.encode(), nx, ny, dof, st, bd, arr, len(params), C.byref(h)))
    else:
        check(L.lib().nk_problem_create_grid3(ctx._h, source.encode(), nx, ny, nz, dof, st, bd, arr, len(params), C.byref(h)))
    P = _GridDeviceProblem(h, ctx)
    P.p, P.nx, P.ny, P.dof, P.stencil, P.boundary = params, nx, ny, dof, stencil, boundary
    if nz is not None:
        P.nz = nz
    P.nfields = int(fields)
    l0, l1 = C.c_int64(), C.c_int64()
    check(L.lib().nk_problem_grid_slab(h, C.byref(l0), C.byref(l1)))
    P.lines = (l0.value, l1.value)
    return P


# ------------------------------------------------------------------------------------------- compiled graph problems
def _graph_arrays(rowptr, colind):
    """the adjacency as contiguous int32 host arrays (nn from rowptr; colind may be empty)"""
    rp = np.ascontiguousarray(np.asarray(rowptr), dtype=np.int32).ravel()
    ci = np.ascontiguousarray(np.asarray(colind), dtype=np.int32).ravel()
    if rp.size < 2:
        raise ValueError(f"rowptr has {rp.size} entries: a graph of nn >= 1 nodes has nn + 1")
    if rp[-1] != ci.size:
        raise ValueError(f"rowptr[-1] = {int(rp[-1])} but colind has {ci.size} entries")
    return rp, ci, rp.size - 1


def graph_pattern(rowptr, colind, dof: int = 1):
    """(jrowptr, jcolind), int32, of the Jacobian of a compiled graph problem over the adjacency (rowptr, colind): row c·nn + i
    holds, for every component c2 in order, node i itself and its neighbours in ascending node order — dof·(deg_i + 1) ascending
    columns c2·nn + node. Host only. An adjacency that breaks a rule of CompiledGraphProblem raises NKError naming the first
    offending row."""
    rp, ci, nn = _graph_arrays(rowptr, colind)
    return _sized_call(L.lib().nk_graph_pattern, (nn, C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data), int(dof)),
                       lambda nnz: (dof * nn + 1, nnz))


def graph_compile_check(source: str, dof: int = 1, nparams: int = 0, edge_data: int = 0, node_data: int = 0) -> int:
    """Compile the residual, JVP and Jacobian kernels of a CompiledGraphProblem source for gfx950 (no device needed); the size of
    the code objects. A source that does not compile raises NKError with the contract and the compiler's log."""
    nb = C.c_int64()
    check(L.lib().nk_graph_compile_check(source.encode(), int(dof), int(nparams), int(edge_data), int(node_data), C.byref(nb)))
    return nb.value


class _GraphDeviceProblem(_CompiledDeviceProblem):
    """the nk_problem of CompiledGraphProblem: its data are one array per edge and per node"""

    def _set_data(self, on_edges, k, x):
        what, n = ("edge", self.ne) if on_edges else ("node", self.nn)
        self._set_datum(L.lib().nk_problem_set_graph_data, (on_edges, int(k)), x, n,
                        f"{what} datum {k}: expected {n} elements (one per {what})")

    def _get_data(self, on_edges, k):
        return self._get_datum(L.lib().nk_problem_get_graph_data, (on_edges, int(k)), self.ne if on_edges else self.nn)

    def set_edge_data(self, k: int, x):
        """Replace edge datum k (0 .. edge_data − 1) by x: a device tensor or a NumPy array of one float64 per edge, in the order
        of colind. The data is copied; a Jacobian cached for the same u is filled again."""
        self._set_data(1, k, x)

    def set_node_data(self, k: int, x):
        """Replace node datum k (0 .. node_data − 1) by x: one float64 per node. Copied, like set_edge_data."""
        self._set_data(0, k, x)

    def edge_data(self, k: int):
        """a copy of edge datum k as a device tensor"""
        return self._get_data(1, k)

    def node_data(self, k: int):
        """a copy of node datum k as a device tensor"""
        return self._get_data(0, k)


def CompiledGraphProblem(source: str, rowptr, colind, dof: int = 1, params: Sequence[float] = (), ctx=None, *, edge_data: int = 0,
                         node_data: int = 0) -> DeviceProblem:
    """A residual given node by node over any sparse adjacency — a network, an unstructured mesh — as HIP source
        template <typename T> __device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f);
    compiled (hiprtc, gfx950) into the residual kernel, the exact dual-number JVP kernel and the Jacobian fill on the graph's
    CSR pattern (include/mi355x_nk.h, "compiled graph problems"): what NonlinearFunction(f; jac_prototype = any sparse pattern)
    is in the reference. Every solver, linear solver and `precs` object takes it (the scalable one for a general graph is
    ObjectPrecs("amg"); MultigridPrecs needs a grid and is refused). u0 defaults to zeros; NonlinearProblem(..., p) and
    reinit_(cache, p=...) replace the source's p[0..nparams). One rank, Float64.
    The graph: (rowptr, colind) is a CSR adjacency of nn = len(rowptr) − 1 nodes, 0-based, columns strictly ascending within a
    row, no self-loops (the node itself is always an argument and always a column); it may be nonsymmetric (a directed network)
    and may have no edges. Anything else raises NKError naming the first offending row. dof = 1..4, up to 32 parameters,
    edge_data and node_data = 0..4 arrays of one double per edge and per node, dof²·(ne + nn) <= 2³¹ − 1.
    The source: u.self(c = 0) is the node's own unknown c, u.deg() its number of edges, u.nbr(e, c = 0) unknown c of the e-th
    neighbour (e a run-time loop counter in 0 .. deg() − 1), u.node(e) that neighbour's index, u.w(e, k = 0) datum k of that
    edge, u.a(k = 0) the node's own datum k and u.an(e, k = 0) the neighbour's; s = {i, nn, deg}; f receives the node's dof
    residuals, entries not written are zero; nk_real is double. Data are nk_real, never duals. A k outside the declared count
    (and an e or c out of range) reads NaN.
    Numbering is component-major: unknown c of node i is element c·nn + i; edge datum k is one double per edge in the order of
    colind, node datum k one per node. Data are zero until P.set_edge_data(k, x) / P.set_node_data(k, x) — a device tensor or a
    NumPy array, copied — and P.edge_data(k) / P.node_data(k) return device copies. P.nn, P.ne, P.dof describe the graph.
    The pattern (graph_pattern, P.jac_csr()): row c·nn + i holds, for c2 = 0 .. dof − 1, node i and its neighbours in ascending
    node order, dof·(deg_i + 1) entries, structural even where a derivative vanishes.
    Cost: per node 16·dof + 4 + deg·(4 + 8·r_e) + 8·r_n bytes with r_e, r_n the data arrays the source reads; neighbour values
    come from cache for a bandwidth-reducing numbering of the nodes and not for a random one — the graph is not reordered for
    you. The fill evaluates the source once per (node, column node) pair.
    AC power flow (dof 2 = θ, V; edge data g, b; node data P, Q), every bus a PQ bus:
        SRC = '''template <typename T>
        __device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
          const T th = u.self(0), V = u.self(1);
          T fp = T(0.0) - u.a(0), fq = T(0.0) - u.a(1);
          for (int e = 0; e < u.deg(); ++e) {
            const T d = th - u.nbr(e, 0), VV = V * u.nbr(e, 1);
            fp = fp + (u.w(e, 0) * V * V - VV * (u.w(e, 0) * cos(d) + u.w(e, 1) * sin(d)));
            fq = fq + (-u.w(e, 1) * V * V - VV * (u.w(e, 0) * sin(d) - u.w(e, 1) * cos(d)));
          }
          f[0] = fp; f[1] = fq;
        }'''
        P = CompiledGraphProblem(SRC, rowptr, colind, dof=2, edge_data=2, node_data=2)"""
    ctx = ctx or default_context()
    rp, ci, nn = _graph_arrays(rowptr, colind)
    params, arr = _params_array(params)
    h = C.c_void_p()
    check(L.lib().nk_problem_create_graph(ctx._h, source.encode(), nn, C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data),
                                          int(dof), arr, len(params), int(edge_data), int(node_data), C.byref(h)))
    P = _GraphDeviceProblem(h, ctx)
    P.p, P.nn, P.ne, P.dof, P.n_edge_data, P.n_node_data = params, nn, int(ci.size), int(dof), int(edge_data), int(node_data)
    return P


# ------------------------------------------------------------------------------------------- compiled element problems
def _elem_arrays(conn, nn):
    """the connectivity as a contiguous int32 host array [ne, npe]"""
    cn = np.ascontiguousarray(np.asarray(conn), dtype=np.int32)
    if cn.ndim != 2 or cn.shape[0] < 1:
        raise ValueError(f"conn has shape {cn.shape}: a mesh is [ne >= 1, npe] node indices, one row per element")
    return cn, int(nn), int(cn.shape[0]), int(cn.shape[1])


@dataclass
class ElementBlock:
    """a further element block of a CompiledElementProblem: its own source (its own nk_element), its own connectivity
    conn[ne, npe] (npe = 1..8; 1 is a point element) and its own count of element data arrays"""
    source: str
    conn: Any
    elem_data: int = 0


def _elem_block_arrays(conns, nn):
    """the parallel arrays of the block entry points for the connectivities `conns`: (arguments nn, nblocks, ne, npe, conn;
    what keeps them alive)"""
    cns = [_elem_arrays(c, nn)[0] for c in conns]
    k = len(cns)
    ne = (C.c_int64 * k)(*[c.shape[0] for c in cns])
    npe = (C.c_int * k)(*[c.shape[1] for c in cns])
    ptrs = (C.c_void_p * k)(*[c.ctypes.data for c in cns])
    return (int(nn), k, ne, npe, ptrs), cns


def elem_adjacency(conn, nn: int, blocks=None):
    """(rowptr, colind), int32: the node graph of the mesh conn[ne, npe] over nn nodes — two nodes are adjacent when they share
    an element; ascending columns, no self-loops. Host only. A mesh that breaks a rule of CompiledElementProblem raises NKError
    naming the first offending element. blocks=[conn_b, …]: the further connectivities of a mesh of several element blocks
    (the union graph; the message names the block too)."""
    if blocks is not None:
        args, _keep = _elem_block_arrays([conn, *blocks], nn)
        return _sized_call(L.lib().nk_elem_blocks_adjacency, args, lambda nedges: (args[0] + 1, nedges))
    cn, nn, ne, npe = _elem_arrays(conn, nn)
    return _sized_call(L.lib().nk_elem_adjacency, (nn, ne, npe, C.c_void_p(cn.ctypes.data)), lambda nedges: (nn + 1, nedges))


def elem_pattern(conn, nn: int, dof: int = 1, blocks=None):
    """(jrowptr, jcolind), int32, of the Jacobian of a compiled element problem on the mesh conn[ne, npe] over nn nodes:
    graph_pattern of elem_adjacency(conn, nn). Host only. blocks=[conn_b, …]: the further connectivities of a mesh of several
    element blocks."""
    if blocks is not None:
        args, _keep = _elem_block_arrays([conn, *blocks], nn)
        return _sized_call(L.lib().nk_elem_blocks_pattern, (*args, int(dof)), lambda nnz: (dof * args[0] + 1, nnz))
    cn, nn, ne, npe = _elem_arrays(conn, nn)
    return _sized_call(L.lib().nk_elem_pattern, (nn, ne, npe, C.c_void_p(cn.ctypes.data), int(dof)),
                       lambda nnz: (dof * nn + 1, nnz))


def elem_compile_check(source: str, npe: int, dof: int = 1, nparams: int = 0, node_data: int = 0, elem_data: int = 0) -> int:
    """Compile the residual, JVP and element-matrix kernels of a CompiledElementProblem source for gfx950 (no device needed); the
    size of the code objects. A source that does not compile raises NKError with the contract and the compiler's log."""
    nb = C.c_int64()
    check(L.lib().nk_elem_compile_check(source.encode(), int(npe), int(dof), int(nparams), int(node_data), int(elem_data), C.byref(nb)))
    return nb.value


class _ElemDeviceProblem(_CompiledDeviceProblem):
    """the nk_problem of CompiledElementProblem: its data are one array per node and per element, and it has fixed unknowns"""

    def _set_data(self, on_elements, k, x):
        what, n = ("element", self.ne) if on_elements else ("node", self.nn)
        self._set_datum(L.lib().nk_problem_set_elem_data, (on_elements, int(k)), x, n,
                        f"{what} datum {k}: expected {n} elements (one per {what})")

    def _get_data(self, on_elements, k):
        return self._get_datum(L.lib().nk_problem_get_elem_data, (on_elements, int(k)), self.ne if on_elements else self.nn)

    def set_node_data(self, k: int, x):
        """Replace node datum k (0 .. node_data − 1) by x: one float64 per node. Copied, like set_elem_data."""
        self._set_data(0, k, x)

    def node_data(self, k: int):
        """a copy of node datum k as a device tensor"""
        return self._get_data(0, k)

    def _block_ne(self, block):
        """the element count of a block; a block the problem does not have is the library's error"""
        return self.blocks[block][0] if 0 <= block < len(self.blocks) else 0

    def set_elem_data(self, k: int, x, block: int = 0):
        """Replace element datum k (0 .. elem_data − 1) of block `block` by x: a device tensor or a NumPy array of one float64
        per element of that block. The data is copied; a Jacobian cached for the same u is filled again."""
        if block == 0:
            return self._set_data(1, k, x)
        n = self._block_ne(int(block))
        size = x.numel() if _is_torch(x) else np.size(x)
        self._set_datum(L.lib().nk_problem_set_elem_block_data, (int(block), int(k)), x, n if n else size,
                        f"element datum {k} of block {block}: expected {n} elements (one per element)")

    def elem_data(self, k: int, block: int = 0):
        """a copy of element datum k of block `block` as a device tensor"""
        if block == 0:
            return self._get_data(1, k)
        return self._get_datum(L.lib().nk_problem_get_elem_block_data, (int(block), int(k)), self._block_ne(int(block)))

    def set_fixed(self, mask, values=None):
        """Fix the unknowns with mask != 0 (dof·nn entries, component-major) at `values` (dof·nn float64; None: zeros): their
        rows become F_r = u_r − g_r with the unit row in J. A mask of zeros frees everything again. Host arrays, copied."""
        n = self.dof * self.nn
        m = np.ascontiguousarray(np.asarray(mask).ravel() != 0, dtype=np.int32)
        if m.size != n:
            raise ValueError(f"mask: expected {n} entries (dof·nn, component-major), got {m.size}")
        g = None
        if values is not None:
            g = np.ascontiguousarray(values.detach().cpu().numpy() if _is_torch(values) else values, dtype=np.float64).ravel()
            if g.size != n:
                raise ValueError(f"values: expected {n} entries (dof·nn, component-major), got {g.size}")
        check(L.lib().nk_problem_set_elem_fixed(self._h, C.c_void_p(m.ctypes.data), None if g is None else C.c_void_p(g.ctypes.data),
                                                L.HOST))

    def fixed(self):
        """(mask int32, values float64) as NumPy arrays of dof·nn entries"""
        n = self.dof * self.nn
        m, g = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64)
        check(L.lib().nk_problem_get_elem_fixed(self._h, C.c_void_p(m.ctypes.data), C.c_void_p(g.ctypes.data), L.HOST))
        return m, g


def CompiledElementProblem(source: str, conn, nn: int, dof: int = 1, params: Sequence[float] = (), ctx=None, *, node_data: int = 0,
                           elem_data: int = 0, blocks: Sequence[ElementBlock] = ()) -> DeviceProblem:
    """A finite-element / finite-volume residual given element by element on any mesh, as HIP source
        template <typename T> __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f);
    compiled (hiprtc, gfx950) into the element-residual kernel, the exact dual-number JVP kernel and the element-matrix kernel;
    a gather kernel of the library sums an element's contributions into rows of F, of J·v and entries of J in ascending
    element order, without atomics (include/mi355x_nk.h, "compiled element problems"). In the reference this is the assembly
    loop inside `f` with jac_prototype = the mesh's sparsity. Every solver, linear solver and `precs` object takes it (the
    scalable one is ObjectPrecs("amg"); MultigridPrecs needs a grid and is refused). One rank, Float64.
    The mesh: conn[ne, npe] int32, the nodes of every element (all elements have one npe = 2..8), over nn nodes; dof = 1..4 with
    npe·dof <= 16; up to 32 parameters and node_data, elem_data = 0..4 arrays of one double per node and per element. A node
    index outside 0..nn−1 or a node twice in one element raises NKError naming the first offending element. A node in no
    element is allowed (its residual is 0 unless it is fixed).
    The source: u.at(a, c = 0) is unknown c at the element's a-th node (a = 0 .. NK_NPE − 1), u.node(a) that node's index,
    u.x(a, k = 0) node datum k at that node, u.w(k = 0) datum k of the element, s = {e, ne, nn}, and f[a·NK_DOF + c] receives
    the element's contribution to residual c of its a-th node (entries not written are zero). Data are nk_real, never duals; an
    a, c or k out of range reads NaN. Write loops over a with compile-time bounds (#pragma unroll).
    Numbering is component-major: unknown c of node i is element c·nn + i. Data are zero until P.set_node_data(k, x) /
    P.set_elem_data(k, x); P.node_data(k) / P.elem_data(k) return device copies. P.nn, P.ne, P.npe, P.dof describe the mesh.
    Fixed unknowns: P.set_fixed(mask, values=None) makes the rows with mask != 0 Dirichlet rows, F_r = u_r − g_r, unit row in J
    (columns of fixed unknowns stay in the free rows); P.fixed() returns (mask, values); P.initial_guess() is zeros with the
    fixed values written in. The pattern (elem_pattern, P.jac_csr()) is graph_pattern of elem_adjacency(conn, nn).
    P1 Bratu −Δu = λ·exp(u) on triangles (node data x, y; the exponential lumped at the nodes):
        SRC = '''template <typename T>
        __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
          const nk_real x1 = u.x(1, 0) - u.x(0, 0), y1 = u.x(1, 1) - u.x(0, 1), x2 = u.x(2, 0) - u.x(0, 0), y2 = u.x(2, 1) - u.x(0, 1);
          const nk_real det = x1 * y2 - x2 * y1, area = 0.5 * fabs(det);
          const nk_real bx[3] = {(y1 - y2) / det, y2 / det, -y1 / det}, by[3] = {(x2 - x1) / det, -x2 / det, x1 / det};
          const T gx = bx[0] * u.at(0) + bx[1] * u.at(1) + bx[2] * u.at(2), gy = by[0] * u.at(0) + by[1] * u.at(1) + by[2] * u.at(2);
        #pragma unroll
          for (int a = 0; a < 3; ++a) f[a] = area * (gx * bx[a] + gy * by[a]) - (p[0] * area / 3.0) * exp(u.at(a));
        }'''
        P = CompiledElementProblem(SRC, conn, nn, params=[1.0], node_data=2); P.set_fixed(boundary_mask)
    Several element blocks in one mesh: blocks=[ElementBlock(source, conn, elem_data=0), …] adds up to 7 further blocks, each
    with its own source, connectivity (npe = 1..8; 1 is a point element) and element data; the positional source, conn and
    elem_data are block 0, and nn, dof, params, the node data, the fixed unknowns and the pattern (the union of all blocks'
    node pairs) are shared. This is how boundary terms, mixed meshes (triangles beside quads), a truss on a continuum and
    nodal springs are written. A row sums block 0's elements ascending, then block 1's, …: no atomics, the same bits every
    run. The source of block k sees NK_NPE and NK_NELEM of its block, s.e and s.ne counting within it, u.w(k) its own data
    and NK_BLOCK = k; errors name the block. P.set_elem_data(k, x, block=0) and P.elem_data(k, block=0) address a block;
    P.blocks lists every block's (ne, npe, elem_data); P.ne and P.npe stay block 0's. A Robin (radiation) condition
    −∂u/∂n = p[1]·(u⁴ − w⁴) on the boundary edges of the Bratu triangulation above, the ambient value w an element datum of
    the bars (consistent 2 × 2 weights (2, 1; 1, 2)/6):
        ROBIN = '''template <typename T>
        __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
          const nk_real dx = u.x(1, 0) - u.x(0, 0), dy = u.x(1, 1) - u.x(0, 1), len = sqrt(dx * dx + dy * dy);
          const nk_real w4 = u.w(0) * u.w(0) * u.w(0) * u.w(0);
          const T q0 = u.at(0) * u.at(0) * u.at(0) * u.at(0) - w4, q1 = u.at(1) * u.at(1) * u.at(1) * u.at(1) - w4;
          f[0] = (p[1] * len / 6.0) * (2.0 * q0 + q1);
          f[1] = (p[1] * len / 6.0) * (q0 + 2.0 * q1);
        }'''
        P = CompiledElementProblem(SRC, conn, nn, params=[1.0, 0.5], node_data=2,
                                   blocks=[ElementBlock(ROBIN, boundary_edges, elem_data=1)])
        P.set_elem_data(0, ambient, block=1)"""
    ctx = ctx or default_context()
    cn, nn, ne, npe = _elem_arrays(conn, nn)
    params, arr = _params_array(params)
    h = C.c_void_p()
    if not blocks:
        check(L.lib().nk_problem_create_elements(ctx._h, source.encode(), nn, ne, npe, C.c_void_p(cn.ctypes.data), int(dof), arr,
                                                 len(params), int(node_data), int(elem_data), C.byref(h)))
        shapes = [(ne, npe, int(elem_data))]
    else:
        blocks = list(blocks)
        (_nn, k, nes, npes, ptrs), cns = _elem_block_arrays([cn] + [b.conn for b in blocks], nn)
        srcs = (C.c_char_p * k)(source.encode(), *[b.source.encode() for b in blocks])
        nel = (C.c_int * k)(int(elem_data), *[int(b.elem_data) for b in blocks])
        check(L.lib().nk_problem_create_element_blocks(ctx._h, nn, int(dof), k, srcs, nes, npes, ptrs, nel, arr, len(params),
                                                       int(node_data), C.byref(h)))
        shapes = [(int(c.shape[0]), int(c.shape[1]), int(m)) for c, m in zip(cns, nel)]
    P = _ElemDeviceProblem(h, ctx)
    P.p, P.nn, P.ne, P.npe, P.dof, P.n_node_data, P.n_elem_data = params, nn, ne, npe, int(dof), int(node_data), int(elem_data)
    P.blocks = shapes
    return P


@dataclass
class NonlinearFunction:
    """NonlinearFunction{true}(f!; jvp, vjp, jac, jac_prototype) with torch-tensor callbacks on the device:
    f(du, u, p), jvp(Jv, v, u, p), vjp(vJ, v, u, p), jac(nzval, u, p) (values of jac_prototype, a CSRMatrix)."""
    f: Callable
    jvp: Optional[Callable] = None
    vjp: Optional[Callable] = None
    jac: Optional[Callable] = None
    jac_prototype: Optional[CSRMatrix] = None
    mass_matrix: object = None   # picked up by PseudoTransient when the algorithm names none (number or diagonal vector)


class NonlinearProblem:
    """NonlinearProblem(f, u0, p). `f` is a built-in DeviceProblem or a NonlinearFunction of torch callbacks.
    (NonlinearLeastSquaresProblem below is the same container with `least_squares = True`.)"""
    least_squares = False

    def __init__(self, f, u0=None, p=None, ctx: Optional[Context] = None):
        self.p = p
        if isinstance(f, DeviceProblem):
            self.device_problem = f
            self.ctx = f.ctx
            self.u0 = f.initial_guess() if u0 is None else u0
            if p is not None:
                self.set_p(p)
            return
        if not isinstance(f, NonlinearFunction):
            f = NonlinearFunction(f)
        if u0 is None:
            raise ValueError("u0 is required for a NonlinearFunction problem")
        self.ctx = ctx or default_context()
        self.u0 = u0
        n = int(u0.numel() if _is_torch(u0) else np.asarray(u0).size)
        prob = self

        def wrap(fn, nargs):
            if fn is None:
                return None

            def cb(*a):
                try:
                    with torch.cuda.stream(torch.cuda.ExternalStream(a[-1])) if a[-1] else _nullctx():
                        tensors = [_view(q, n) for q in a[1:-1]]
                        if nargs == 2:      # residual(u, f) → f!(du, u, p)
                            fn(tensors[1], tensors[0], prob.p)
                        elif nargs == 3:    # (v, u, out) → jvp!(out, v, u, p)
                            fn(tensors[2], tensors[0], tensors[1], prob.p)
                    return 0
                except Exception as e:  # pragma: no cover - surfaced as NK_E_CALLBACK
                    import traceback
                    traceback.print_exc()
                    return 1
            return cb

        def jac_cb(user, u_ptr, vals_ptr, stream):
            try:
                nnz = f.jac_prototype.info()["nnz"]
                # the fill must be ordered against the library's SpMV / LU kernels: run it on the library's stream
                with torch.cuda.stream(torch.cuda.ExternalStream(stream)) if stream else _nullctx():
                    f.jac(_view(vals_ptr, nnz), _view(u_ptr, n), prob.p)
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1

        cbs = L.UserCallbacks(
            L.RESIDUAL_FN(wrap(f.f, 2)),
            L.JVP_FN(wrap(f.jvp, 3)) if f.jvp else L.JVP_FN(),
            L.JVP_FN(wrap(f.vjp, 3)) if f.vjp else L.JVP_FN(),
            L.JACVALS_FN(jac_cb) if (f.jac and f.jac_prototype is not None) else L.JACVALS_FN(),
        )
        h = C.c_void_p()
        check(L.lib().nk_problem_create_user(self.ctx._h, n, n, 0, C.byref(cbs), None,
                                             f.jac_prototype._h if f.jac_prototype is not None else None,
                                             C.byref(h)))
        self.device_problem = DeviceProblem(h, self.ctx, keep=[cbs, f])
        self.f = f

    def set_p(self, p):
        self.p = p
        dp = self.device_problem
        if isinstance(dp, (_GridDeviceProblem, _GraphDeviceProblem, _ElemDeviceProblem)):   # a compiled problem: p is the source's p[0..nparams)
            dp.set_p(p)
        elif hasattr(dp, "params"):
            params = list(dp.params)
            if isinstance(p, (int, float)):
                params[1] = float(p)           # quadratic p / Bratu λ
            else:
                params[1:1 + len(p)] = [float(x) for x in p]
            dp.params = params
            dp.set_params(params)


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ------------------------------------------------------------------------------------------- algorithms
@dataclass
class ChebyshevPrecs:
    """`precs` for KrylovJL_GMRES: right preconditioner M⁻¹ = p_d(A), d Chebyshev steps on [λmax/ratio, λmax]
    (λmax bounded/estimated by the library for every new Jacobian). Operator applications only."""
    degree: int = 16
    ratio: float = 100.0


@dataclass
class MultigridPrecs:
    """`precs` for KrylovJL_GMRES on Bratu2D and Brusselator2D problems and on compiled grid problems: one geometric multigrid
    V-cycle as the right preconditioner (nu Chebyshev smoothing steps, coarsest grid side ≤ coarse_max, banded LU there) — the
    device counterpart of an algebraic-multigrid `precs` (docs/src/tutorials/large_systems.md:244-316). Mesh-independent
    iteration counts.
    CompiledGridProblem (one rank; more ranks raise NKError): 2-D and 3-D, every stencil, dof <= 4, fields, every combination of
    side kinds. Level l is the same problem — same source, options and p, the fine problem's code objects — on smaller sides,
    its matrix that problem's Jacobian fill at the restricted u, its fields the restricted fields; every new Jacobian restricts
    u and the fields again, copies p, refills every level and refactors the coarsest, so set_field and set_p between solves are
    picked up. CONTRACT: the source takes its spacing from s.nx, s.ny, s.nz (the level it runs on), not from p. A source that
    does not gets a poor preconditioner, not a wrong answer; ObjectPrecs("amg") remains for it. Per axis (grid_mg_axis), in
    units of the fine spacing: a side's offset a is 1 (dirichlet), 0 (mirror_node), 1/2 (mirror_face), L = n − 1 + a_lo + a_hi,
    nc = floor(L/2 + 1.5 − a_lo − a_hi); periodic nc = floor(n/2 + 0.5); an axis is coarsened while n > coarse_max and nc >= 3
    (radius 2: 5). Transfers: tensor products of linear interpolation at the nodes' positions and its row-normalised transpose.
    Smoother: Chebyshev on D⁻¹A over [rho/4, rho], rho = max_i sum_j |a_ij|/|a_ii|. coarse_max < 3: the library's default for a
    compiled grid problem, 8; coarse_max = None selects the problem kind's default."""
    nu: int = 2
    coarse_max: Optional[int] = None   # None: the problem kind's default — 31 for Bratu2D and Brusselator2D, 8 for a compiled grid problem


@dataclass
class LinearSolveParameters:
    """lib/NonlinearSolveBase/src/linear_solve.jl:1-4: what `precs(A, p)` receives as p — the current iterate u (a device
    tensor) and the nonlinear problem's parameters p."""
    u: object
    p: object


class Preconditioner:
    """nk_precond: a preconditioner object built from a CSRMatrix on the device — what a `precs(A, p)` returns for a general
    sparse Jacobian (docs/src/tutorials/large_systems.md:252-316 fills the slot with IncompleteLU.ilu / an algebraic
    multigrid). Usable as Pl or Pr of the device GMRES and standalone (`apply`)."""

    def __init__(self, handle, A):
        self._h, self.A, self.n = handle, A, None

    def update(self):
        """refactorise for the matrix's current values (`precs` is re-evaluated for every new A)"""
        check(L.lib().nk_precond_update(self._h))
        return self

    def apply(self, x):
        """y = M⁻¹ x (device tensor in → device tensor out; NumPy in → NumPy out)"""
        if _is_torch(x):
            y = torch.empty_like(x)
            check(L.lib().nk_precond_apply(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                                           L.DEVICE if x.is_cuda else L.HOST))
            return y
        xa = np.ascontiguousarray(x, dtype=np.float64)
        ya = np.empty_like(xa)
        check(L.lib().nk_precond_apply(self._h, C.c_void_p(xa.ctypes.data), C.c_void_p(ya.ctypes.data), L.HOST))
        return ya

    __call__ = apply

    def info(self):
        k, ll, lu, nc = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(L.lib().nk_precond_info(self._h, C.byref(k), C.byref(ll), C.byref(lu), C.byref(nc)))
        return dict(kind={1: "jacobi", 2: "ilu0", 3: "amg", 4: "ilut"}[k.value], levels_lower=ll.value, levels_upper=lu.value, ncolors=nc.value)

    def close(self):
        if self._h:
            L.lib().nk_precond_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class JacobiPreconditioner(Preconditioner):
    """M = diag(A)"""

    def __init__(self, A: "CSRMatrix"):
        h = C.c_void_p()
        check(L.lib().nk_precond_create_jacobi(A._h, C.byref(h)))
        super().__init__(h, A)


class ILU0Preconditioner(Preconditioner):
    """A ≈ LU on the pattern of A (no fill, no pivoting) of the rank's local block, level-scheduled on the device.
    ordering = "natural": the classical preconditioner in the matrix's ordering (a lexicographic stencil is a dependency chain
    of 2n − 1 levels: milliseconds per application at n = 1024²); "multicolor": rows permuted by a greedy colouring (as many
    levels as colours — the GPU form)."""

    def __init__(self, A: "CSRMatrix", ordering: str = "multicolor"):
        h = C.c_void_p()
        check(L.lib().nk_precond_create_ilu0(A._h, {"natural": 0, "multicolor": 1}[ordering], C.byref(h)))
        super().__init__(h, A)
        self.ordering = ordering

    def factors(self):
        """(L, U, perm) as SciPy CSR matrices in the permuted ordering: perm[permuted row] = original row."""
        import scipy.sparse as sp
        nnz = C.c_int64(0)
        check(L.lib().nk_precond_ilu0_factors(self._h, C.byref(nnz), None, None, None, None))
        n = self.A.shape[0]
        rp, ci = np.zeros(n + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32)
        v, perm = np.zeros(nnz.value), np.zeros(n, dtype=np.int32)
        check(L.lib().nk_precond_ilu0_factors(self._h, None, C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data),
                                              C.c_void_p(v.ctypes.data), C.c_void_p(perm.ctypes.data)))
        M = sp.csr_matrix((v, ci, rp), shape=(n, n))
        return sp.tril(M, -1).tocsr() + sp.identity(n, format="csr"), sp.triu(M, 0).tocsr(), perm


class ILUTPreconditioner(ILU0Preconditioner):
    """Crout ILU with the drop tolerance `tau` — the tutorial's `incompletelu(W, p) = (ilu(W, τ = 50.0), I)`
    (docs/src/tutorials/large_systems.md:252-260): A ≈ (I + L) U with fill, an entry kept if its magnitude before the division by
    the pivot is ≥ tau. Factorised on the host for every `update()` (the pattern depends on the numbers; the reference's
    IncompleteLU.jl runs on the CPU as well), applied on the device by two level-scheduled triangular solves."""

    def __init__(self, A: "CSRMatrix", tau: float):
        h = C.c_void_p()
        check(L.lib().nk_precond_create_ilut(A._h, float(tau), C.byref(h)))
        Preconditioner.__init__(self, h, A)
        self.ordering, self.tau = "natural", float(tau)


class AMGPreconditioner(Preconditioner):
    """Aggregation algebraic multigrid built from the matrix alone (csrc/nk_amg.hip) — what the reference's tutorial returns from
    `precs(A, p)` as Pl for a large sparse Jacobian (`aspreconditioner(ruge_stuben(A))`, docs/src/tutorials/large_systems.md:276-316):
    pairwise aggregation (aggregates of ≤ 2^passes rows, formed on the device at creation), Galerkin coarse matrices refreshed on the device by
    `update()`, ν Chebyshev steps on D⁻¹A per side, over-corrected coarse correction, dense inverse on the ≤ 128 coarsest rows."""

    def __init__(self, A: "CSRMatrix", nu: int = 0, passes: int = 0, theta: float = 0.0, overcorrection: float = 0.0,
                 cheb_ratio: float = 0.0, coarse_max: int = 0, matching: str = "auto"):
        # matching: "auto" (the device set-up's handshaking on one rank, the host's sequential pass on a rank's local block),
        # "greedy" (host) or "handshake" (device)
        mt = {"auto": 0, "greedy": 1, "handshake": 2}[matching]
        prm = L.AMGParams(int(nu), int(passes), int(coarse_max), mt, float(theta), float(overcorrection), float(cheb_ratio))
        h = C.c_void_p()
        check(L.lib().nk_precond_create_amg(A._h, C.byref(prm), C.byref(h)))
        super().__init__(h, A)

    def hierarchy(self):
        """[(rows, non-zeros, Gershgorin bound of D⁻¹A)] per level, finest first, coarsest last"""
        nl = C.c_int(0)
        check(L.lib().nk_precond_amg_info(self._h, C.byref(nl), 0, None, None, None))
        n, z, lm = (C.c_int64 * nl.value)(), (C.c_int64 * nl.value)(), (C.c_double * nl.value)()
        check(L.lib().nk_precond_amg_info(self._h, C.byref(nl), nl.value, n, z, lm))
        return [(int(n[i]), int(z[i]), float(lm[i])) for i in range(nl.value)]

    @property
    def matching(self) -> str:
        """how the aggregates were formed: "greedy" (sequential pairwise pass, host set-up) or "handshake" (device set-up)"""
        m = C.c_int(0)
        check(L.lib().nk_precond_amg_matching(self._h, C.byref(m)))
        return {1: "greedy", 2: "handshake"}[m.value]

    def aggregates(self, level: int):
        """row → coarse row of `level` (NumPy int32)"""
        rows = self.hierarchy()[level][0]
        out = np.empty(rows, dtype=np.int32)
        check(L.lib().nk_precond_amg_aggregates(self._h, int(level), C.c_void_p(out.ctypes.data), rows))
        return out

    def level_matrix(self, level: int) -> "CSRMatrix":
        """A_l of the hierarchy: a non-owning view (it lives as long as this object; values as of the last `update()`). Level 0
        is the matrix the object was built from, or on several ranks the private copy of the rank's local square block."""
        h = C.c_void_p()
        check(L.lib().nk_precond_amg_level_matrix(self._h, int(level), C.byref(h)))
        A = CSRMatrix(h, self.A.ctx, owned=False)
        A._keep = self   # the view reads this object's arrays
        return A


@dataclass
class ObjectPrecs:
    """`precs` through nk_options: a built-in object (kind = "jacobi" | "ilu0" | "ilu0_natural" | "amg") on the concrete Jacobian,
    refactorised inside the solver for every new J — no callback into the host language. side = "left" as the reference's
    tutorial precs (`(Pl, I)`), or "right"."""
    kind: str = "ilu0"
    side: str = "left"


@dataclass
class KrylovJL_GMRES:
    """LinearSolve.KrylovJL_GMRES stand-in executed by the device GMRES (protocol: SURVEY.md §8d)."""
    gmres_restart: int = 30
    maxiters: int = 300
    ortho: str = "sstep"       # "mgs" (Krylov.jl's structure) | "cgs2" | "dcgs2" (= cgs2, delayed 2nd pass) | "cgs" | "sstep" (the library default)
    fixed_iters: int = 0
    sstep: int = 0             # ortho = "sstep": basis columns per block (1..16); 0 = automatic (15 Newton basis, 6 monomial)
    sstep_basis: str = "auto"  # "auto" (Newton where the spectrum can be bounded) | "monomial" | "newton"
    abstol: Optional[float] = None   # None → the nonlinear tolerances are forwarded (FirstOrder/src/solve.jl:203)
    reltol: Optional[float] = None
    # `precs`: a callable precs(A, p::LinearSolveParameters) -> (Pl, Pr) as in the reference (re-evaluated for every new A;
    # Pl / Pr: None (identity), a Preconditioner object, or a callable y = P⁻¹ x on device tensors), or one of the built-in
    # descriptors ChebyshevPrecs / MultigridPrecs (right) / ObjectPrecs (either side)
    precs: object = None


@dataclass
class EisenstatWalkerForcing2:  # eisenstat_walker.jl:18-29
    eta0: float = 0.5
    eta_max: float = 0.9
    gamma: float = 0.9
    alpha: float = 2.0
    safeguard: bool = True
    safeguard_threshold: float = 0.1


@dataclass
class BackTracking:
    """LineSearch.jl / LineSearches.jl BackTracking [EXT]: `NewtonRaphson(linesearch = BackTracking())`."""
    c_1: float = 1e-4
    rho_hi: float = 0.5
    rho_lo: float = 0.1
    order: int = 3
    maxiters: int = 1000


@dataclass
class LineSearchesJL:
    """LineSearch.jl's wrapper around LineSearches.jl [EXT]: `NewtonRaphson(linesearch = LineSearchesJL(; method = …))` with
    method "Static" | "BackTracking" | "StrongWolfe" | "MoreThuente" | "HagerZhang" (LineSearches.jl default parameters) — the methods of lib/NonlinearSolveFirstOrder/test/rootfind_tests__item2.jl:40-46."""
    method: str = "BackTracking"


class RadiusUpdateSchemes:  # trust_region.jl:59-147
    Simple, NLsolve, NocedalWright, Hei, Yuan, Bastin, Fan = range(7)


@dataclass
class NewtonRaphson:  # raphson.jl:30-43
    linsolve: Optional[KrylovJL_GMRES] = None
    forcing: Optional[EisenstatWalkerForcing2] = None
    concrete_jac: Optional[bool] = None
    linesearch: Optional[BackTracking] = None   # `missing` in the reference = no line search
    jac_colored: bool = False
    name: str = "NewtonRaphson"


@dataclass
class TrustRegion:  # trust_region.jl:25-43
    linsolve: Optional[KrylovJL_GMRES] = None
    radius_update_scheme: int = RadiusUpdateSchemes.Simple
    max_trust_radius: float = 0.0
    initial_trust_radius: float = 0.0
    step_threshold: float = 1.0 / 10000
    shrink_threshold: float = 1.0 / 4
    expand_threshold: float = 3.0 / 4
    shrink_factor: float = 1.0 / 4
    expand_factor: float = 2.0
    max_shrink_times: int = 32
    concrete_jac: Optional[bool] = None
    jac_colored: bool = False   # concrete J by colour-compressed assembly (sparse AD analogue) instead of closed-form values
    name: str = "TrustRegion"


@dataclass
class GaussNewton:  # gauss_newton.jl:11-23: NewtonDescent; on a least-squares problem with a Krylov linsolve: normal form
    linsolve: Optional[KrylovJL_GMRES] = None
    concrete_jac: Optional[bool] = None
    linesearch: Optional[BackTracking] = None
    forcing: Optional[EisenstatWalkerForcing2] = None
    name: str = "GaussNewton"


@dataclass
class LevenbergMarquardt:  # levenberg_marquardt.jl:37-64 (keyword names of the reference; α_geodesic spelt alpha_geodesic)
    linsolve: Optional[KrylovJL_GMRES] = None
    damping_initial: float = 1.0
    alpha_geodesic: float = 0.75
    disable_geodesic: bool = False
    damping_increase_factor: float = 2.0
    damping_decrease_factor: float = 3.0
    finite_diff_step_geodesic: float = 0.1
    b_uphill: float = 1.0
    min_damping_D: float = 1e-8
    concrete_jac: Optional[bool] = True   # concrete_jac = Val(true) in the reference's constructor
    jac_colored: bool = False
    name: str = "LevenbergMarquardt"


@dataclass
class PseudoTransient:  # pseudo_transient.jl:37-57
    """mass_matrix: None / 1.0 (identity), a number λ (λ·I), or a vector m of the local length of u (Diagonal(m)); the
    damping term is α⁻¹·M. A general (non-diagonal) M would change the sparsity pattern of the damped J — not on this path."""
    linsolve: Optional[KrylovJL_GMRES] = None
    alpha_initial: float = 1e-3
    mass_matrix: object = None
    concrete_jac: Optional[bool] = None
    linesearch: Optional[BackTracking] = None
    jac_colored: bool = False
    name: str = "PseudoTransient"


class LimitedMemoryBroyden:  # lib/NonlinearSolveQuasiNewton/src/lbroyden.jl:20-35
    """LimitedMemoryBroyden(; max_resets = 3, linesearch = nothing, threshold = 10, reset_tolerance = nothing, alpha = nothing):
    J⁻¹ = I/α + U Vᵀ with `threshold` columns (1..32, clamped to maxiters), good-Broyden updates, NoChangeInStateReset.
    Needs only the residual — a problem without jvp / jac is accepted. The line-search form is not built."""
    linsolve = None
    name = "LimitedMemoryBroyden"

    def __init__(self, max_resets: int = 3, linesearch=None, threshold: int = 10, reset_tolerance: Optional[float] = None,
                 alpha: Optional[float] = None):
        if linesearch is not None:
            raise NotImplementedError("LimitedMemoryBroyden(linesearch=…): only the form without a line search is built")
        self.max_resets, self.threshold = int(max_resets), int(threshold)
        self.reset_tolerance, self.alpha = reset_tolerance, alpha

    def __repr__(self):
        return (f"LimitedMemoryBroyden(max_resets={self.max_resets}, threshold={self.threshold}, "
                f"reset_tolerance={self.reset_tolerance}, alpha={self.alpha})")


class Broyden:  # lib/NonlinearSolveQuasiNewton/src/broyden.jl:34-49
    """Broyden(; max_resets = 100, linesearch = nothing, reset_tolerance = nothing, init_jacobian = Val(:identity), alpha = nothing,
    update_rule = Val(:good_broyden)): the inverse Jacobian itself, a dense n×n matrix on the device that starts as I/α
    (`update_rule` "good_broyden" or "bad_broyden"), or its diagonal ("diagonal"), with NoChangeInStateReset. Needs only the
    residual. The dense matrix is allocated by the first step and is limited to n ≤ 32768 (8 GiB); `init` raises above that.
    init_jacobian = "true_jacobian" and the line-search form are not built."""
    linsolve = None
    name = "Broyden"

    def __init__(self, max_resets: int = 100, linesearch=None, reset_tolerance: Optional[float] = None,
                 init_jacobian: str = "identity", alpha: Optional[float] = None, update_rule: str = "good_broyden"):
        if update_rule not in L.BROYDEN_RULES:
            raise ValueError(f"Unknown update rule `update_rule = {update_rule!r}`. Please choose a valid update rule.")
        if init_jacobian not in ("identity", "true_jacobian"):
            raise ValueError(f"Unknown `init_jacobian = {init_jacobian!r}`. Please choose a valid `init_jacobian`.")
        self.max_resets, self.linesearch, self.reset_tolerance = int(max_resets), linesearch, reset_tolerance
        self.init_jacobian, self.alpha, self.update_rule = init_jacobian, alpha, update_rule

    def __repr__(self):
        return (f"Broyden(max_resets={self.max_resets}, reset_tolerance={self.reset_tolerance}, "
                f"init_jacobian={self.init_jacobian!r}, alpha={self.alpha}, update_rule={self.update_rule!r})")


class Klement:  # lib/NonlinearSolveQuasiNewton/src/klement.jl:29-48
    """Klement(; max_resets = 100, linsolve = nothing, linesearch = nothing, alpha = nothing, init_jacobian = Val(:identity)): J is
    the vector α·1 (DiagonalStructure, not inverted), the step −fu ./ J, the reset test any(iszero, J). Needs only the residual;
    `linsolve` is not read (a diagonal J needs none). The true-Jacobian initialisations and the line-search form are not built."""
    name = "Klement"

    def __init__(self, max_resets: int = 100, linsolve=None, linesearch=None, alpha: Optional[float] = None,
                 init_jacobian: str = "identity"):
        if init_jacobian not in ("identity", "true_jacobian", "true_jacobian_diagonal"):
            raise ValueError(f"Unknown `init_jacobian = {init_jacobian!r}`. Please choose a valid `init_jacobian`.")
        self.max_resets, self.linsolve, self.linesearch = int(max_resets), linsolve, linesearch
        self.alpha, self.init_jacobian = alpha, init_jacobian

    def __repr__(self):
        return f"Klement(max_resets={self.max_resets}, alpha={self.alpha}, init_jacobian={self.init_jacobian!r})"


class DFSane:  # lib/NonlinearSolveSpectralMethods/src/dfsane.jl:21-35
    """DFSane(; sigma_min = 1e-10, sigma_max = 1e10, sigma_1 = nothing, M = 10, gamma = 1e-4, tau_min = 0.1, tau_max = 0.5,
    n_exp = 2, max_inner_iterations = 100): the spectral residual method, step −ασ f with σ = ⟨δu,δu⟩/⟨δu,δf⟩ and the
    RobustNonMonotone line search for α. Needs only the residual — a problem without jvp / jac is accepted. `sigma_1 = None`
    is what the reference's DFSane hands to GeneralizedDFSane (σ = ⟨u,u⟩/⟨u,f⟩ at the start); a number is taken as the first
    σ. M is 1..32, n_exp 1 or 2; `eta_strategy` is fixed at f₁/k²."""
    linsolve = None
    name = "DFSane"

    def __init__(self, sigma_min: float = 1e-10, sigma_max: float = 1e10, sigma_1: Optional[float] = None, M: int = 10,
                 gamma: float = 1e-4, tau_min: float = 0.1, tau_max: float = 0.5, n_exp: int = 2,
                 max_inner_iterations: int = 100, eta_strategy=None):
        if eta_strategy is not None:
            raise NotImplementedError("DFSane(eta_strategy=…): only the default f₁/k² is built")
        self.sigma_min, self.sigma_max, self.sigma_1 = float(sigma_min), float(sigma_max), sigma_1
        self.M, self.n_exp, self.max_inner_iterations = int(M), int(n_exp), int(max_inner_iterations)
        self.gamma, self.tau_min, self.tau_max = float(gamma), float(tau_min), float(tau_max)

    def __repr__(self):
        return (f"DFSane(sigma_min={self.sigma_min}, sigma_max={self.sigma_max}, sigma_1={self.sigma_1}, M={self.M}, "
                f"gamma={self.gamma}, tau_min={self.tau_min}, tau_max={self.tau_max}, n_exp={self.n_exp}, "
                f"max_inner_iterations={self.max_inner_iterations})")


@dataclass
class _TerminationMode:
    """SciMLBase termination modes (lib/NonlinearSolveBase/src/termination_conditions.jl); `internalnorm` is
    "inf" (Base.Fix1(maximum, abs), the reference default) or "l2"."""
    internalnorm: str = "inf"
    patience_steps: int = 100
    patience_objective_multiplier: float = 3.0
    min_max_factor: float = 1.3
    max_stalled_steps: Optional[int] = None
    protective_threshold: Optional[float] = None
    code = 0


class AbsNormSafeBestTerminationMode(_TerminationMode):
    code = 0


class NormTerminationMode(_TerminationMode):
    code = 1


class RelTerminationMode(_TerminationMode):
    code = 2


class RelNormTerminationMode(_TerminationMode):
    code = 3


class RelNormSafeTerminationMode(_TerminationMode):
    code = 4


class RelNormSafeBestTerminationMode(_TerminationMode):
    code = 5


class AbsTerminationMode(_TerminationMode):
    code = 6


class AbsNormTerminationMode(_TerminationMode):
    code = 7


class AbsNormSafeTerminationMode(_TerminationMode):
    code = 8


TERMINATION_CONDITIONS = [  # common/common_rootfind_testing.jl:3-13
    NormTerminationMode, RelTerminationMode, RelNormTerminationMode, RelNormSafeTerminationMode,
    RelNormSafeBestTerminationMode, AbsTerminationMode, AbsNormTerminationMode, AbsNormSafeTerminationMode,
    AbsNormSafeBestTerminationMode,
]

_SS_BASIS = {"auto": 0, "monomial": 1, "newton": 2}
_ORTHO = {"mgs": L.ORTHO_MGS, "cgs2": L.ORTHO_CGS2, "cgs": L.ORTHO_CGS, "dcgs2": L.ORTHO_DCGS2, "dcgs2_1r": L.ORTHO_DCGS2_1R,
          "sstep": L.ORTHO_SSTEP}


def _options(alg, abstol, reltol, maxiters, maxtime, store_trace, termination_kwargs,
             termination_condition=None, least_squares=False) -> L.Options:
    o = L.Options()
    check(L.lib().nk_options_default(C.byref(o)))
    ls = alg.linsolve
    o.algorithm = L.ALG_TRUST_REGION if isinstance(alg, TrustRegion) else L.ALG_NEWTON_RAPHSON
    if least_squares:
        o.termination_norm = 1  # default_termination_mode(::NonlinearLeastSquaresProblem): AbsNormSafeBest on the 2-norm
    if isinstance(alg, GaussNewton):   # (linsolve = None: a factorising solver takes J δ = f as it is — no normal form)
        o.algorithm = L.ALG_GAUSS_NEWTON
        o.termination_norm = 1  # (Gauss–Newton is defined on least-squares problems only)
    if isinstance(alg, PseudoTransient):
        o.algorithm = L.ALG_PSEUDO_TRANSIENT
        o.pt_alpha_initial = float(alg.alpha_initial)
    if isinstance(alg, LevenbergMarquardt):   # (linsolve = None: JᵀJ + λDᵀD is assembled and factorised on the device)
        o.algorithm = L.ALG_LEVENBERG_MARQUARDT
        o.lm_disable_geodesic = int(bool(alg.disable_geodesic))
        o.lm_damping_initial = float(alg.damping_initial)
        o.lm_damping_increase_factor = float(alg.damping_increase_factor)
        o.lm_damping_decrease_factor = float(alg.damping_decrease_factor)
        o.lm_min_damping_D = float(alg.min_damping_D)
        o.lm_alpha_geodesic = float(alg.alpha_geodesic)
        o.lm_finite_diff_step_geodesic = float(alg.finite_diff_step_geodesic)
        o.lm_b_uphill = float(alg.b_uphill)
    if isinstance(alg, LimitedMemoryBroyden):   # no Jacobian, no linear solve: `linsolve` and the Krylov fields are not read
        o.algorithm = L.ALG_LIMITED_MEMORY_BROYDEN
        if alg.threshold < 1 or alg.max_resets < 1:
            raise ValueError("LimitedMemoryBroyden: threshold and max_resets must be positive")
        o.lb_threshold, o.lb_max_resets = alg.threshold, alg.max_resets
        o.lb_reset_tolerance = 0.0 if alg.reset_tolerance is None else float(alg.reset_tolerance)
        o.lb_alpha = 0.0 if alg.alpha is None else float(alg.alpha)
        ls = KrylovJL_GMRES()
        o.linsolve = L.LINSOLVE_GMRES_MATFREE
    elif isinstance(alg, (Broyden, Klement)):   # likewise; a line search reaches the library, which refuses it (NK_E_INVALID)
        o.algorithm = L.ALG_BROYDEN if isinstance(alg, Broyden) else L.ALG_KLEMENT
        if alg.max_resets < 1:
            raise ValueError(f"{alg.name}: max_resets must be positive")
        o.broyden_update_rule = L.BROYDEN_RULES[getattr(alg, "update_rule", "good_broyden")]
        if alg.init_jacobian != "identity":
            o.broyden_update_rule += L.BROYDEN_TRUE_JACOBIAN
        o.qn_max_resets = alg.max_resets
        o.qn_reset_tolerance = 0.0 if getattr(alg, "reset_tolerance", None) is None else float(alg.reset_tolerance)
        o.qn_alpha = 0.0 if alg.alpha is None else float(alg.alpha)
        ls = KrylovJL_GMRES()
        o.linsolve = L.LINSOLVE_GMRES_MATFREE
    elif isinstance(alg, DFSane):   # likewise: the residual and nothing else
        o.algorithm = L.ALG_DFSANE
        if alg.M < 1 or alg.n_exp < 1 or alg.max_inner_iterations < 1:
            raise ValueError("DFSane: M, n_exp and max_inner_iterations must be positive")
        if not (alg.sigma_min > 0 and alg.sigma_max > 0 and alg.gamma > 0 and alg.tau_min > 0 and alg.tau_max > 0):
            raise ValueError("DFSane: sigma_min, sigma_max, gamma, tau_min and tau_max must be positive")
        if alg.sigma_1 is not None and not (float(alg.sigma_1) != 0.0):
            raise ValueError("DFSane: sigma_1 = 0 is no spectral coefficient (None selects ⟨u,u⟩/⟨u,f⟩)")
        o.sane_sigma_min, o.sane_sigma_max = alg.sigma_min, alg.sigma_max
        o.sane_sigma_1 = 0.0 if alg.sigma_1 is None else float(alg.sigma_1)
        o.sane_M, o.sane_n_exp, o.sane_max_inner_iterations = alg.M, alg.n_exp, alg.max_inner_iterations
        o.sane_gamma, o.sane_tau_min, o.sane_tau_max = alg.gamma, alg.tau_min, alg.tau_max
        ls = KrylovJL_GMRES()
        o.linsolve = L.LINSOLVE_GMRES_MATFREE
    elif ls is None:
        # linsolve = nothing: LinearSolve's default factorisation of the concrete sparse J → banded LU on device
        o.linsolve = L.LINSOLVE_BANDED_LU
        ls = KrylovJL_GMRES()  # unused Krylov fields keep their defaults
    else:
        o.linsolve = L.LINSOLVE_GMRES_CSR if (alg.concrete_jac or isinstance(alg, LevenbergMarquardt)) \
            else L.LINSOLVE_GMRES_MATFREE
    o.maxiters = int(maxiters)
    o.abstol = 0.0 if abstol is None else float(abstol)
    o.reltol = 0.0 if reltol is None else float(reltol)
    o.maxtime = 0.0 if maxtime is None else float(maxtime)
    o.gmres_restart, o.gmres_maxiters = int(ls.gmres_restart), int(ls.maxiters)
    o.gmres_ortho, o.gmres_fixed_iters = _ORTHO[ls.ortho], int(ls.fixed_iters)
    o.gmres_sstep = int(getattr(ls, "sstep", 0))
    o.gmres_sstep_basis = _SS_BASIS[getattr(ls, "sstep_basis", "auto")]
    o.lin_abstol = -1.0 if ls.abstol is None else float(ls.abstol)
    o.lin_reltol = -1.0 if ls.reltol is None else float(ls.reltol)
    lsr = getattr(alg, "linesearch", None)
    if isinstance(lsr, LineSearchesJL):
        o.linesearch = {"BackTracking": 1, "Static": 2, "StrongWolfe": 3, "MoreThuente": 4, "HagerZhang": 5}[lsr.method]
    elif lsr is not None:
        o.linesearch = 1
        o.ls_c1, o.ls_rho_hi, o.ls_rho_lo = float(lsr.c_1), float(lsr.rho_hi), float(lsr.rho_lo)
        o.ls_order, o.ls_maxiters = int(lsr.order), int(lsr.maxiters)
    precs = getattr(ls, "precs", None)
    if isinstance(precs, MultigridPrecs):
        o.mg_nu, o.mg_coarse = int(precs.nu), 31 if precs.coarse_max is None else int(precs.coarse_max)   # (grid problems: FirstOrderCache)
    elif isinstance(precs, ChebyshevPrecs):
        o.cheb_degree, o.cheb_ratio = int(precs.degree), float(precs.ratio)
    elif isinstance(precs, ObjectPrecs):
        o.precond_kind = {"jacobi": 1, "ilu0_natural": 2, "ilu0": 3, "ilu0_multicolor": 3, "amg": 4}[precs.kind]
        o.precond_side = {"right": 0, "left": 1}[precs.side]
    elif precs is not None and not callable(precs):
        raise TypeError("KrylovJL_GMRES(precs=…): a callable precs(A, p) -> (Pl, Pr) or a built-in descriptor")
    o.jac_colored = int(bool(getattr(alg, "jac_colored", False)))
    fo = getattr(alg, "forcing", None)
    if fo is not None:
        o.forcing = L.FORCING_EW2
        o.ew_eta0, o.ew_eta_max, o.ew_gamma, o.ew_alpha = fo.eta0, fo.eta_max, fo.gamma, fo.alpha
        o.ew_safeguard, o.ew_safeguard_threshold = int(fo.safeguard), fo.safeguard_threshold
    if isinstance(alg, TrustRegion):
        o.radius_update_scheme = int(alg.radius_update_scheme)
        o.max_shrink_times = int(alg.max_shrink_times)
        for k in ("max_trust_radius", "initial_trust_radius", "step_threshold", "shrink_threshold",
                  "expand_threshold", "shrink_factor", "expand_factor"):
            setattr(o, k, float(getattr(alg, k)))
    if termination_condition is not None:
        tc = termination_condition() if isinstance(termination_condition, type) else termination_condition
        o.termination_mode = tc.code
        o.termination_norm = {"inf": 0, "l2": 1}[tc.internalnorm]
        o.patience_steps = int(tc.patience_steps)
        o.patience_objective_multiplier = float(tc.patience_objective_multiplier)
        o.min_max_factor = float(tc.min_max_factor)
        # an explicitly constructed mode has max_stalled_steps = nothing unless given (the default *mode* of the
        # solver is built with max_stalled_steps = 32, termination_conditions.jl:385-389)
        o.max_stalled_steps = -1 if tc.max_stalled_steps is None else int(tc.max_stalled_steps)
        o.protective_threshold = 0.0 if tc.protective_threshold is None else float(tc.protective_threshold)
    for k, v in (termination_kwargs or {}).items():
        setattr(o, k, v)
    o.store_trace = int(bool(store_trace))
    return o


@dataclass
class NLStats:
    nf: int = 0
    njacs: int = 0
    nfactors: int = 0
    nsolve: int = 0
    nsteps: int = 0
    gmres_iters: int = 0
    op_applies: int = 0
    allreduces: int = 0
    halo_exchanges: int = 0


@dataclass
class NonlinearSolution:
    u: object
    resid: object
    retcode: str
    stats: NLStats
    trace: list = field(default_factory=list)
    alg: object = None

    @property
    def successful_retcode(self):  # SciMLBase.successful_retcode
        return self.retcode == "Success"


class FirstOrderCache:
    """GeneralizedFirstOrderAlgorithmCache behind nk_solver: init / step! / solve! / reinit!."""

    def __init__(self, prob: NonlinearProblem, alg, abstol=None, reltol=None, maxiters=1000, maxtime=None,
                 store_trace=False, termination_kwargs=None, termination_condition=None):
        self.prob, self.alg = prob, alg
        self._opts = _options(alg, abstol, reltol, maxiters, maxtime, store_trace, termination_kwargs,
                              termination_condition, least_squares=getattr(prob, "least_squares", False))
        precs = getattr(getattr(alg, "linsolve", None), "precs", None)
        if isinstance(precs, MultigridPrecs) and precs.coarse_max is None and isinstance(prob.device_problem, _GridDeviceProblem):
            self._opts.mg_coarse = 0   # the library's default for a compiled grid problem
        self._u0_is_torch = _is_torch(prob.u0)
        p, ms, _k = _ptr(prob.u0, prob.device_problem.n_local)
        h = C.c_void_p()
        check(L.lib().nk_solver_init(prob.device_problem._h, p, ms, C.byref(self._opts), C.byref(h)))
        self._h = h
        self.n = prob.device_problem.n_local
        self._install_precs_hook()
        M = getattr(alg, "mass_matrix", None)
        if M is None and isinstance(alg, PseudoTransient):   # resolve_ser_mass_matrix(::Nothing, prob): fall back to prob.f's
            M = getattr(getattr(prob, "f", None), "mass_matrix", None)
        if M is not None:
            if np.ndim(M) == 0:
                M = None if float(M) == 1.0 else np.full(self.n, float(M))       # resolve_ser_mass_matrix: I ≡ nothing
            elif np.ndim(M) != 1:
                raise NKError("PseudoTransient(mass_matrix=…): only the identity, λ·I and Diagonal(m) run on the device "
                              "(a general M changes the sparsity pattern of J + α⁻¹ M)")
            elif len(M) != self.n:  # DimensionMismatch in the reference (pseudo_transient.jl:110-118)
                raise NKError(f"mass matrix has {len(M)} diagonal entries but the problem has {self.n} local unknowns")
            if M is not None:
                pm, msm, self._mass_keep = _ptr(M, self.n)
                check(L.lib().nk_solver_set_mass_matrix_diagonal(self._h, pm, msm))

    def _out(self, fn):
        if self._u0_is_torch and self.prob.u0.is_cuda:
            out = torch.empty(self.n, dtype=torch.float64, device=self.prob.u0.device)
        else:
            out = np.empty(self.n)
        p, ms, _k = _ptr(out)
        check(fn(self._h, p, ms))
        return out

    @property
    def u(self):
        return self._out(L.lib().nk_solver_get_u)

    @property
    def fu(self):
        return self._out(L.lib().nk_solver_get_resid)

    @property
    def stats(self) -> NLStats:
        s = L.Stats()
        check(L.lib().nk_solver_get_stats(self._h, C.byref(s)))
        return NLStats(**s.as_dict())

    def _ret(self):
        r, n, f = C.c_int(), C.c_int(), C.c_int()
        check(L.lib().nk_solver_get_retcode(self._h, C.byref(r), C.byref(n), C.byref(f)))
        return r.value, n.value, bool(f.value)

    @property
    def retcode(self):
        return L.RET_NAMES[self._ret()[0]]

    @property
    def nsteps(self):
        return self._ret()[1]

    @property
    def force_stop(self):
        return self._ret()[2]

    @property
    def trust_region(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(L.lib().nk_solver_get_scalars(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return b.value

    @property
    def eta(self):
        """the Eisenstat–Walker forcing cache's η (`cache.forcing_cache.η`, eisenstat_walker.jl:32-39)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(L.lib().nk_solver_get_scalars(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return c.value

    @property
    def lbroyden_state(self) -> dict:
        """LimitedMemoryBroyden: resets counted, updates since the last reset (idx), the scaling a of a·I + U Vᵀ, the threshold
        in effect and the reset test's two counters"""
        r, i, t, d, f = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        a = C.c_double()
        check(L.lib().nk_solver_get_lbroyden_state(self._h, C.byref(r), C.byref(i), C.byref(a), C.byref(t), C.byref(d),
                                                   C.byref(f)))
        return dict(nresets=r.value, idx=i.value, a=a.value, threshold=t.value, since_du=d.value, since_dfu=f.value)

    @property
    def qn_state(self) -> dict:
        """Broyden / Klement: resets counted, the scaling of the last (re)initialisation (Broyden: a of J⁻¹ = a·I; Klement: α
        of J = α·1), the reset test's two counters and the steps since the last reset"""
        r, d, f, k = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        a = C.c_double()
        check(L.lib().nk_solver_get_qn_state(self._h, C.byref(r), C.byref(a), C.byref(d), C.byref(f), C.byref(k)))
        return dict(nresets=r.value, a=a.value, since_du=d.value, since_dfu=f.value, steps_since_reset=k.value)

    def broyden_inverse(self):
        """Broyden: J⁻¹ as it stands — an n×n tensor (array for a host u0), or the n diagonal entries for update_rule =
        "diagonal"; Klement: the n diagonal entries of J. It exists from the first step on."""
        dense = isinstance(self.alg, Broyden) and self.alg.update_rule != "diagonal"
        shape = (self.n, self.n) if dense else (self.n,)
        if self._u0_is_torch and self.prob.u0.is_cuda:
            out = torch.empty(shape, dtype=torch.float64, device=self.prob.u0.device)
            p, ms = C.c_void_p(out.data_ptr()), L.DEVICE
        else:
            out = np.empty(shape)
            p, ms = out.ctypes.data_as(C.c_void_p), L.HOST
        check(L.lib().nk_solver_get_broyden_inverse(self._h, p, self.n, ms))
        return out

    @property
    def dfsane_state(self) -> dict:
        """DFSane: the spectral coefficient σ the next step starts from, the last step's length with its sign (+α₊ or −α₋; NaN
        after a failed line search), the residual evaluations of the last line search and of all of them, M and the merit
        history (M values)"""
        s, a = C.c_double(), C.c_double()
        t, tt, m = C.c_int(), C.c_int(), C.c_int()
        h = (C.c_double * 32)()
        check(L.lib().nk_solver_get_dfsane_state(self._h, C.byref(s), C.byref(a), C.byref(t), C.byref(tt), C.byref(m), h))
        return dict(sigma=s.value, alpha=a.value, trials=t.value, total_trials=tt.value, M=m.value, history=list(h[:m.value]))

    @property
    def fnorm_inf(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(L.lib().nk_solver_get_scalars(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value

    @property
    def trace(self):
        n = C.c_int()
        check(L.lib().nk_solver_get_trace(self._h, None, 0, C.byref(n)))
        rows = (L.TraceEntry * max(n.value, 1))()
        check(L.lib().nk_solver_get_trace(self._h, rows, n.value, C.byref(n)))
        return [dict(iter=r.iter, gmres_iters=r.gmres_iters, accepted=bool(r.accepted), fnorm_inf=r.fnorm_inf,
                     step_norm2=r.step_norm2, eta=r.eta, trust_region=r.trust_region, rho=r.rho)
                for r in rows[: n.value]]

    def step(self, recompute_jacobian: Optional[bool] = None, evaluate_residual: bool = True):
        """step!(cache; recompute_jacobian = nothing, evaluate_residual = true)"""
        rj = -1 if recompute_jacobian is None else int(bool(recompute_jacobian))
        check(L.lib().nk_solver_step_ex(self._h, rj, int(bool(evaluate_residual))))
        return self

    def supports_deferred_residual(self) -> bool:
        y = C.c_int()
        check(L.lib().nk_solver_supports_deferred_residual(self._h, C.byref(y)))
        return bool(y.value)

    def refresh_residual(self):
        """refresh_residual!(cache): settle a residual evaluation deferred by step(evaluate_residual=False)."""
        check(L.lib().nk_solver_refresh_residual(self._h))
        return None

    def _install_precs_hook(self):
        """KrylovJL_GMRES(precs = callable): `precs(A, LinearSolveParameters(u, p)) -> (Pl, Pr)` is evaluated when the
        linear cache is built and again for every new Jacobian (never by reinit!) — the protocol test/Core/
        core_tests__item21.jl pins through its call counts. A = the concrete Jacobian (a CSRMatrix view of the solver's J),
        or the StatefulJacobianOperator of the matrix-free path."""
        ls = getattr(self.alg, "linsolve", None)
        precs = getattr(ls, "precs", None)
        if precs is None or isinstance(precs, (ChebyshevPrecs, MultigridPrecs, ObjectPrecs)) or not callable(precs):
            return
        n, prob = self.n, self.prob
        self._precs_keep = []

        def hook(user, gh, ah, uptr):
            try:
                u = _view(uptr, n)
                if ah:
                    A = CSRMatrix(C.c_void_p(ah), prob.ctx, owned=False)
                else:
                    A = StatefulJacobianOperator(JacobianOperator(prob), u)
                out = precs(A, LinearSolveParameters(u, prob.p))
                Pl, Pr = out if isinstance(out, tuple) else (out, None)
                keep = []
                _install_preconditioner(C.c_void_p(gh), "left", Pl, n, keep)
                _install_preconditioner(C.c_void_p(gh), "right", Pr, n, keep)
                self._precs_keep = keep      # (the previous pair may be released now: the GMRES object holds the new one)
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1
        self._precs_fn = L.PRECS_FN(hook)
        check(L.lib().nk_solver_set_precs(self._h, self._precs_fn, None))

    def solve(self) -> NonlinearSolution:
        r = C.c_int()
        check(L.lib().nk_solver_solve(self._h, C.byref(r)))
        return NonlinearSolution(self.u, self.fu, L.RET_NAMES[r.value], self.stats,
                                 self.trace if self._opts.store_trace else [], self.alg)

    def reinit(self, u0=None, p=None):
        params, npar = None, 0
        if p is not None:
            self.prob.set_p(p)  # built-ins push the new parameters to the device problem
        if u0 is not None:
            pu, ms, _k = _ptr(u0, self.n)
        else:
            pu, ms = None, L.HOST
        check(L.lib().nk_solver_reinit(self._h, pu, ms, params, npar))
        return self

    def close(self):
        if self._h:
            L.lib().nk_solver_destroy(self._h)
            self._h = None


class NonlinearLeastSquaresProblem(NonlinearProblem):
    """NonlinearLeastSquaresProblem(f, u0, p): residual count = unknown count on this path (row-partitioned square J). What the
    type changes is what the reference derives from it: the default termination mode measures the residual in the 2-norm
    (default_termination_mode(::NonlinearLeastSquaresProblem)) for EVERY algorithm, and a polyalgorithm's best-of fallback ranks
    its sub-solvers by the 2-norm (findmin_resids, NonlinearSolveBase/src/polyalg.jl)."""
    least_squares = True


def init(prob: NonlinearProblem, alg, **kw):
    from . import polyalg
    if isinstance(alg, polyalg.NonlinearSolvePolyAlgorithm):
        return polyalg.PolyAlgorithmCache(prob, alg, least_squares=getattr(prob, "least_squares", False), **kw)
    return FirstOrderCache(prob, alg, **kw)


def solve(prob: NonlinearProblem, alg, **kw) -> NonlinearSolution:
    from . import polyalg
    if isinstance(alg, polyalg.NonlinearSolvePolyAlgorithm):
        return polyalg.polysolve(prob, alg, least_squares=getattr(prob, "least_squares", False), **kw)
    cache = FirstOrderCache(prob, alg, **kw)
    try:
        return cache.solve()
    finally:
        cache.close()


def step_(cache: FirstOrderCache, **kw):   # step!(cache; recompute_jacobian, evaluate_residual)
    return cache.step(**kw)


def supports_deferred_residual(cache: FirstOrderCache) -> bool:
    return cache.supports_deferred_residual()


def refresh_residual(cache: FirstOrderCache):   # refresh_residual!(cache)
    return cache.refresh_residual()


def solve_(cache: FirstOrderCache):  # solve!(cache)
    return cache.solve()


def reinit_(cache, u0=None, p=None, **kw):  # reinit!(cache, u0; p[, retain_best])
    return cache.reinit(u0, p, **kw)


# ------------------------------------------------------------------------------------------- linear solve seam
def _install_preconditioner(gh, side: str, M, n: int, keep: list):
    """Pl or Pr on the nk_gmres `gh`: None / identity removes that side; a Preconditioner object goes in as it is (no host
    round trip per application); any other callable y = P⁻¹ x on device tensors becomes a device callback."""
    lib = L.lib()
    left = side == "left"
    if M is None or M is IDENTITY:
        check(lib.nk_gmres_set_preconditioner(gh, 1 if left else 0, None))
        return
    if isinstance(M, Preconditioner):
        keep.append(M)
        check(lib.nk_gmres_set_preconditioner(gh, 1 if left else 0, M._h))
        return
    if not callable(M):
        raise TypeError(f"a preconditioner must be None, a Preconditioner or a callable, not {type(M)}")

    def cb(user, x, y, stream):
        try:
            _view(y, n).copy_(M(_view(x, n)))
            return 0
        except Exception:  # pragma: no cover
            import traceback
            traceback.print_exc()
            return 1
    fn = L.MATVEC_FN(cb)
    keep.append(fn)
    check((lib.nk_gmres_set_left_preconditioner if left else lib.nk_gmres_set_right_preconditioner)(gh, fn, None))


class _Identity:
    """LinearAlgebra.I as a preconditioner (what the reference's DummyPreconditioners returns)"""

    def __call__(self, x):
        return x

    def __repr__(self):
        return "I"


IDENTITY = _Identity()


class GMRES:
    """nk_gmres: the LinearCache analogue NonlinearSolveBase drives (A, b, u, reltol; solve!)."""

    def __init__(self, n: int, restart: int = 30, ortho: str = "sstep", ctx: Optional[Context] = None, sstep: int = 0,
                 sstep_basis: str = "auto"):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(L.lib().nk_gmres_create(self.ctx._h, n, restart, _ORTHO[ortho], C.byref(h)))
        if ortho == "sstep":
            check(L.lib().nk_gmres_set_block_size(h, int(sstep)))
            check(L.lib().nk_gmres_set_sstep_basis(h, _SS_BASIS[sstep_basis]))
        self._h, self.n, self._keep = h, n, []
        self.abstol, self.reltol, self.maxiters = 0.0, 1e-8, 300

    def set_operator(self, A, u=None):
        """A: CSRMatrix (concrete J), StatefulJacobianOperator (matrix-free), or callable y = A(x) on tensors."""
        self._keep = [A]
        if isinstance(A, CSRMatrix):
            check(L.lib().nk_gmres_set_operator_csr(self._h, A._h))
        elif isinstance(A, StatefulJacobianOperator):
            if A.mode != "jvp":
                raise NotImplementedError("GMRES on a transposed operator")
            p, ms, k = _ptr(A.u, self.n)
            self._keep.append(k)
            check(L.lib().nk_gmres_set_operator_jvp(self._h, A.jac_op.prob.device_problem._h, p, ms))
        elif callable(A):
            n = self.n

            def cb(user, x, y, stream):
                try:
                    out = A(_view(x, n))
                    _view(y, n).copy_(out)
                    return 0
                except Exception:  # pragma: no cover
                    import traceback
                    traceback.print_exc()
                    return 1
            fn = L.MATVEC_FN(cb)
            self._keep.append(fn)
            check(L.lib().nk_gmres_set_operator_fn(self._h, fn, None))
        else:
            raise TypeError(f"unsupported operator {type(A)}")
        return self

    def set_right_preconditioner(self, M: Optional[Callable]):
        """precs hook (test/Core/core_tests__item21.jl): M(x) ≈ A⁻¹ x on device tensors."""
        if M is None:
            check(L.lib().nk_gmres_set_right_preconditioner(self._h, L.MATVEC_FN(), None))
            return self
        n = self.n

        def cb(user, x, y, stream):
            try:
                _view(y, n).copy_(M(_view(x, n)))
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1
        fn = L.MATVEC_FN(cb)
        self._keep.append(fn)
        check(L.lib().nk_gmres_set_right_preconditioner(self._h, fn, None))
        return self

    def set_left_preconditioner(self, M):
        """Pl of `precs(A, p) -> (Pl, Pr)`: GMRES runs on Pl⁻¹ A Pr⁻¹ and stops on the preconditioned residual. M: None, a
        Preconditioner object, or a callable y = Pl⁻¹ x on device tensors."""
        _install_preconditioner(self._h, "left", M, self.n, self._keep)
        return self

    def set_preconditioner(self, P, side: str = "left"):
        """a Preconditioner object (JacobiPreconditioner / ILU0Preconditioner) on either side"""
        _install_preconditioner(self._h, side, P, self.n, self._keep)
        return self

    def set_chebyshev_preconditioner(self, degree: int, lambda_min: float = 0.0, lambda_max: float = 0.0,
                                     ratio: float = 30.0):
        check(L.lib().nk_gmres_set_chebyshev_preconditioner(self._h, int(degree), float(lambda_min), float(lambda_max),
                                                            float(ratio)))
        return self

    def set_multigrid_preconditioner(self, problem, u, nu: int = 2, coarse_max: Optional[int] = None):
        """One V-cycle of the built-in geometric multigrid (Bratu2D, Brusselator2D, CompiledGridProblem on one rank: see
        MultigridPrecs) as the right preconditioner, linearised at u. Call it again after a new u, set_field or set_p.
        coarse_max = None: the problem kind's default (31 for the built-in problems, 8 for a compiled grid problem). The solver
        object holds one hierarchy; for a compiled grid problem it is built again when the problem, nu or coarse_max change."""
        dp = problem.device_problem if hasattr(problem, "device_problem") else problem
        if coarse_max is None:
            coarse_max = 0 if isinstance(dp, _GridDeviceProblem) else 31
        pu, ms, keep = _ptr(u, self.n)
        self._mg_u = (u, keep, dp)  # the hierarchy keeps reading the fine-level u and the problem's own arrays: keep both alive
        check(L.lib().nk_gmres_set_multigrid_preconditioner(self._h, dp._h, pu, ms, int(nu), int(coarse_max)))
        return self

    def multigrid_levels(self):
        """the hierarchy of the multigrid preconditioner of a compiled grid problem, finest first: per level a dict with
        sides (nx, ny[, nz]), n (unknowns), nnz (of A_l) and rho (the smoother's bound of D⁻¹A_l)"""
        nl = C.c_int(0)
        check(L.lib().nk_gmres_multigrid_levels(self._h, C.byref(nl), 0, None, None, None, None))
        sides, n, nnz = np.zeros((nl.value, 3), dtype=np.int64), np.zeros(nl.value, dtype=np.int64), np.zeros(nl.value, dtype=np.int64)
        rho = np.zeros(nl.value)
        check(L.lib().nk_gmres_multigrid_levels(self._h, C.byref(nl), nl.value, C.c_void_p(sides.ctypes.data),
                                                C.c_void_p(n.ctypes.data), C.c_void_p(nnz.ctypes.data), C.c_void_p(rho.ctypes.data)))
        dim = 3 if sides[0, 2] > 1 else 2
        return [dict(sides=tuple(int(x) for x in sides[l, :dim]), n=int(n[l]), nnz=int(nnz[l]), rho=float(rho[l]))
                for l in range(nl.value)]

    def multigrid_level_matrix(self, level: int) -> CSRMatrix:
        """A_l of that hierarchy: a non-owning view (it lives as long as this solver object)"""
        h = C.c_void_p()
        check(L.lib().nk_gmres_multigrid_level_matrix(self._h, int(level), C.byref(h)))
        A = CSRMatrix(h, self.ctx, owned=False)
        A._keep = self   # the view reads this object's arrays
        return A

    def multigrid_level_field(self, level: int, k: int):
        """a host copy of field k of level `level` of that hierarchy (one double per node of the level)"""
        lv = self.multigrid_levels()[level]
        out = np.empty(int(np.prod(lv["sides"])))
        check(L.lib().nk_gmres_multigrid_level_field(self._h, int(level), int(k), C.c_void_p(out.ctypes.data), L.HOST))
        return out

    def set_spectrum_interval(self, lo: float, hi: float):
        """Real bounds of the operator's spectrum for operators the library cannot bound itself (callbacks, matrix-free):
        they place the Newton-basis shifts of the s-step Arnoldi process. lo = hi = 0 forgets them."""
        check(L.lib().nk_gmres_set_spectrum_interval(self._h, float(lo), float(hi)))

    def sstep_state(self):
        """(block size in effect, Newton basis in the last solve, blocks that lost rank so far) of the s-step process"""
        bs, nb, bd = C.c_int(0), C.c_int(0), C.c_int(0)
        check(L.lib().nk_gmres_get_sstep_state(self._h, C.byref(bs), C.byref(nb), C.byref(bd)))
        return bs.value, bool(nb.value), bd.value

    def sstep_interval(self):
        """(lo, hi): the bounds of the spectrum the last solve placed its Newton-basis shifts on"""
        a, b = C.c_double(), C.c_double()
        check(L.lib().nk_gmres_get_sstep_interval(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def chebyshev_interval(self):
        a, b = C.c_double(), C.c_double()
        check(L.lib().nk_gmres_get_chebyshev_interval(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def update_tolerances(self, abstol=None, reltol=None):  # LinearSolve.update_tolerances!
        if abstol is not None:
            self.abstol = float(abstol)
        if reltol is not None:
            self.reltol = float(reltol)

    def solve(self, b, x0=None, abstol=None, reltol=None, maxiters=None, fixed_iters=0):
        x = _like(b, self.n)
        use_x0 = 0
        if x0 is not None:
            if _is_torch(x):
                x.copy_(x0)
            else:
                x[...] = x0
            use_x0 = 1
        pb, ms, _a = _ptr(b, self.n)
        px, _m, _b = _ptr(x)
        info = L.GmresInfo()
        check(L.lib().nk_gmres_solve(self._h, pb, px, ms, use_x0,
                                     self.abstol if abstol is None else abstol,
                                     self.reltol if reltol is None else reltol,
                                     self.maxiters if maxiters is None else maxiters, fixed_iters, C.byref(info)))
        return x, dict(iters=info.iters, restarts=info.restarts, converged=bool(info.converged),
                       failed=bool(info.failed), rnorm0=info.rnorm0, rnorm=info.rnorm)

    def close(self):
        if self._h:
            L.lib().nk_gmres_destroy(self._h)
            self._h = None


class BandedLU:
    """nk_lu: direct factorisation of a concrete sparse J (the LinearSolve factorisation cache analogue)."""

    def __init__(self, A: CSRMatrix):
        h = C.c_void_p()
        check(L.lib().nk_lu_create(A._h, C.byref(h)))
        self._h, self.A, self.n = h, A, A.info()["nrows_local"]
        self.factor()

    def factor(self, A: Optional[CSRMatrix] = None):
        ok = C.c_int()
        check(L.lib().nk_lu_factor(self._h, (A or self.A)._h, C.byref(ok)))
        if not ok.value:
            raise NKError("banded LU: zero or non-finite pivot")
        return self

    def solve(self, b):
        x = _like(b, self.n)
        pb, ms, _a = _ptr(b, self.n)
        px, _m, _b = _ptr(x)
        check(L.lib().nk_lu_solve(self._h, pb, px, ms))
        return x

    def info(self):
        kl, ku, by = C.c_int(), C.c_int(), C.c_int64()
        check(L.lib().nk_lu_info(self._h, C.byref(kl), C.byref(ku), C.byref(by)))
        e, blk, lev = C.c_int(), C.c_int(), C.c_int()
        check(L.lib().nk_lu_engine(self._h, C.byref(e), C.byref(blk), C.byref(lev)))
        return dict(kl=kl.value, ku=ku.value, band_bytes=by.value, engine=("band_lu", "block_cyclic_reduction")[e.value],
                    block=blk.value, levels=lev.value)

    def close(self):
        if self._h:
            L.lib().nk_lu_destroy(self._h)
            self._h = None


# ------------------------------------------------------------------------------------------- ensembles of small systems
@dataclass
class SimpleNewtonRaphson:
    """lib/SimpleNonlinearSolve/src/raphson.jl:23-25 — the algorithm the reference allows inside GPU kernels.
    `autodiff=None` = AutoForwardDiff (dual numbers in the kernel); `jac=True` uses the `nk_jac` of the source."""
    jac: bool = False
    name: str = "SimpleNewtonRaphson"


# lib/SimpleNonlinearSolve/src/raphson.jl:31 — `const SimpleGaussNewton = SimpleNewtonRaphson`: the name used on least-squares
# problems, the same algorithm object
SimpleGaussNewton = SimpleNewtonRaphson


@dataclass
class SimpleTrustRegion:
    """lib/SimpleNonlinearSolve/src/trust_region.jl:44-55 (default radius update rule); None = reference default.

    In `vectorized_solve` a square ensemble with 8 < n ≤ 64 runs one system per wavefront (`nk_batch_trust_region_wave`: lane j
    owns column j of the dual-number Jacobian; `jac=True` is not used there); n ≤ 8, `per_wavefront=False` and least-squares
    problems run one system per thread (`nk_batch_trust_region`, `nk_batch_trust_region_nlls`). The two forms differ at
    rounding level only; `EnsembleSolution.kernel` names the one that ran."""
    jac: bool = False
    step_threshold: float = 1e-4
    shrink_threshold: Optional[float] = None   # 0.25
    expand_threshold: Optional[float] = None   # 0.75
    shrink_factor: Optional[float] = None      # 0.25
    expand_factor: float = 2.0
    max_shrink_times: int = 32
    name: str = "SimpleTrustRegion"


@dataclass
class SimpleBroyden:
    """lib/SimpleNonlinearSolve/src/broyden.jl:15-24 with linesearch = nothing: Jacobian-free, one n×n inverse per system.
    `alpha=None` scales J⁻¹ from the norms of f(u0) and u0; otherwise J⁻¹ starts as I/alpha."""
    alpha: Optional[float] = None
    name: str = "SimpleBroyden"


@dataclass
class SimpleKlement:
    """lib/SimpleNonlinearSolve/src/klement.jl:7: Jacobian-free, a diagonal Jacobian estimate per system."""
    name: str = "SimpleKlement"


@dataclass
class SimpleDFSane:
    """lib/SimpleNonlinearSolve/src/dfsane.jl:53-64 (eta_strategy fixed at its default f₁/k²): spectral residual steps with a
    non-monotone line search over the last M merit values ‖f‖₂^n_exp. M in 1..32, n_exp 1 or 2."""
    sigma_min: float = 1e-10
    sigma_max: float = 1e10
    sigma_1: float = 1.0
    M: int = 10
    gamma: float = 1e-4
    tau_min: float = 0.1
    tau_max: float = 0.5
    n_exp: int = 2
    name: str = "SimpleDFSane"


class ImmutableNonlinearProblem:
    """SciMLBase.ImmutableNonlinearProblem{false}(f, u0, p) for the kernel-generation path
    (docs/src/tutorials/nonlinear_solve_gpus.md:120-140). `f_source` is HIP C++ defining
    `template <typename T> __device__ void nk_f(const T *u, const double *p, T *f)`; `u0` has n entries (shared by
    every system) or shape (nbatch, n); `p` has shape (nbatch, nparams) — one parameter set per system.

    `eltype=None` solves in Float64 whatever the inputs' dtype. `eltype=float32` (numpy, torch or "float32") solves in
    Float32, the tutorial's element type (nonlinear_solve_gpus.md:146-160): the kernels, constants and default abstol
    (eps(Float32)^(4/5)) are single precision, the source writes `const nk_real *p` (nk_real = float), and `u` / `resid`
    come back as float32."""

    def __init__(self, f_source: str, u0, p, ctx: Optional[Context] = None, eltype=None):
        self.f_source, self.ctx = f_source, ctx or default_context()
        self.u0, self.p = u0, p
        self.float32 = _is_float32(eltype)
        pshape = tuple(p.shape)
        if len(pshape) != 2:
            raise ValueError("p must have shape (nbatch, nparams)")
        self.nbatch, self.nparams = int(pshape[0]), int(pshape[1])
        ushape = tuple(u0.shape)
        self.n = int(ushape[-1])
        self.u0_per_system = len(ushape) == 2
        if self.u0_per_system and ushape[0] != self.nbatch:
            raise ValueError("u0 and p disagree on the number of systems")


class ImmutableNonlinearLeastSquaresProblem(ImmutableNonlinearProblem):
    """NonlinearLeastSquaresProblem{false}(f, u0, p) for the kernel-generation path: `resid_size` = m residuals for the n
    unknowns of `u0`, n ≤ m ≤ 64, one problem per GPU thread (a small model fitted to each of many data sets; each fit's data
    travels in its row of `p`). `f_source` defines `template <typename T> __device__ void nk_f(const T *u, const nk_real *p,
    T *f)` writing m values (and, for `jac=True`, `nk_jac` writing the row-major m×n Jacobian). Solved by
    `vectorized_solve` with SimpleGaussNewton (= SimpleNewtonRaphson) or SimpleTrustRegion; termination is ‖f‖₂ ≤ abstol, so a
    fit whose minimum residual is not zero ends in MaxIters or ShrinkThresholdExceeded, as in the reference. (The large-system
    class is NonlinearLeastSquaresProblem.)"""

    def __init__(self, f_source: str, u0, p, resid_size: int, ctx: Optional[Context] = None, eltype=None):
        super().__init__(f_source, u0, p, ctx, eltype)
        self.m = int(resid_size)
        if self.m < self.n:
            raise ValueError(f"resid_size = {self.m} < {self.n} unknowns: the minimum-norm solution of an underdetermined "
                             "problem is not offered")


@dataclass
class EnsembleSolution:
    u: object          # (nbatch, n)
    resid: object      # (nbatch, n), or (nbatch, m) for a least-squares problem: residual at the last evaluated iterate (reference: `fx` returned by check_termination)
    retcode: np.ndarray  # (nbatch,) strings
    iters: np.ndarray    # (nbatch,)
    retcode_raw: np.ndarray = None
    kernel: str = ""     # the kernel that solved the ensemble (nk_batch_last_kernel), e.g. "nk_batch_trust_region_wave"


def _is_float32(eltype) -> bool:
    if eltype is None or eltype in (np.float64, "float64") or (torch is not None and eltype is torch.float64):
        return False
    if eltype in (np.float32, "float32") or (torch is not None and eltype is torch.float32) or \
            (isinstance(eltype, np.dtype) and eltype == np.float32):
        return True
    if isinstance(eltype, np.dtype) and eltype == np.float64:
        return False
    raise ValueError(f"eltype {eltype!r}: the ensemble solvers work in float64 (None) or float32")


class _BatchKernel:
    _cache: dict = {}

    @classmethod
    def get(cls, ctx, source, n, nparams, flags, m=None):
        """m = None: a square ensemble (nk_batch_create); else a least-squares one with m residuals (nk_batch_create_nlls)"""
        key = (id(ctx), source, n, nparams, flags, m)
        if key not in cls._cache:
            h = C.c_void_p()
            if m is None:
                check(L.lib().nk_batch_create(ctx._h, source.encode(), n, nparams, flags, C.byref(h)))
            else:
                check(L.lib().nk_batch_create_nlls(ctx._h, source.encode(), n, m, nparams, flags, C.byref(h)))
            cls._cache[key] = h
        return cls._cache[key]


def vectorized_solve(prob: ImmutableNonlinearProblem, alg=None, abstol=None, maxiters=1000, per_wavefront=None):
    """`vectorized_solve(prob, alg; backend = ROCBackend())` of the tutorial (nonlinear_solve_gpus.md:106-114): solve
    every parameter set with SimpleNewtonRaphson, one system per GPU thread, in one kernel launch. The problem's eltype
    picks the precision (Float64 unless it was built with eltype=float32). `alg` may also be SimpleTrustRegion or one of the
    Jacobian-free SimpleBroyden, SimpleKlement, SimpleDFSane (their kernels are compiled on first use). On an
    ImmutableNonlinearLeastSquaresProblem `alg` is SimpleGaussNewton (= SimpleNewtonRaphson) or SimpleTrustRegion, and
    `resid` has shape (nbatch, m).

    `per_wavefront`: None picks the form per method and size (SimpleNewtonRaphson and SimpleTrustRegion run one system per
    wavefront for 8 < n ≤ 64); False runs every method one system per thread (NK_BATCH_PER_THREAD); True insists on a
    per-wavefront kernel: ValueError where there is none to ask for (n ≤ 8, n > 64, a least-squares problem, a Jacobian-free
    method), RuntimeError if it did not build. `EnsembleSolution.kernel` names the kernel that ran."""
    alg = alg or SimpleNewtonRaphson()
    nlls = isinstance(prob, ImmutableNonlinearLeastSquaresProblem)
    if per_wavefront and (nlls or not 8 < prob.n <= 64):
        raise ValueError("per_wavefront=True: the per-wavefront kernels solve square systems with 8 < n <= 64" +
                         (" (this is a least-squares problem)" if nlls else f" (n = {prob.n})"))
    if per_wavefront and not isinstance(alg, (SimpleNewtonRaphson, SimpleTrustRegion)):
        raise ValueError(f"per_wavefront=True: {getattr(alg, 'name', type(alg).__name__)} has no per-wavefront kernel")
    if nlls and not isinstance(alg, (SimpleNewtonRaphson, SimpleTrustRegion)):
        raise TypeError(f"{getattr(alg, 'name', type(alg).__name__)} is not defined on a least-squares problem (nor is it in "
                        "the reference): use SimpleGaussNewton or SimpleTrustRegion")
    if isinstance(alg, SimpleBroyden) and alg.alpha is not None and not alg.alpha > 0:
        raise ValueError(f"SimpleBroyden: alpha = {alg.alpha} must be positive (or None)")
    if isinstance(alg, SimpleDFSane) and not (1 <= int(alg.M) <= 32 and int(alg.n_exp) in (1, 2)):
        raise ValueError(f"SimpleDFSane: M = {alg.M} must lie in 1..32 and n_exp = {alg.n_exp} must be 1 or 2")
    f32 = prob.float32
    flags = (L.BATCH_ANALYTIC_JAC if getattr(alg, "jac", False) else 0) | (L.BATCH_FLOAT32 if f32 else 0) | \
        (L.BATCH_PER_THREAD if per_wavefront is False else 0)
    h = _BatchKernel.get(prob.ctx, prob.f_source, prob.n, prob.nparams, flags, prob.m if nlls else None)
    on_dev = _is_torch(prob.p) and prob.p.is_cuda
    nb, n = prob.nbatch, prob.n
    nr = prob.m if nlls else n
    if on_dev:
        tdt = torch.float32 if f32 else torch.float64
        u0 = prob.u0 if (_is_torch(prob.u0) and prob.u0.is_cuda) else torch.as_tensor(np.asarray(prob.u0), device=prob.p.device)
        u0 = u0.to(tdt).contiguous()
        pp = prob.p.to(tdt).contiguous()
        u = torch.empty((nb, n), dtype=tdt, device=pp.device)
        r = torch.empty((nb, nr), dtype=tdt, device=pp.device)
        rc = torch.empty(nb, dtype=torch.int32, device=pp.device)
        it = torch.empty(nb, dtype=torch.int32, device=pp.device)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        ms = L.DEVICE
    else:
        ndt = np.float32 if f32 else np.float64
        u0 = np.ascontiguousarray(np.asarray(prob.u0.cpu() if _is_torch(prob.u0) else prob.u0), dtype=ndt)
        pp = np.ascontiguousarray(np.asarray(prob.p.cpu() if _is_torch(prob.p) else prob.p), dtype=ndt)
        u, r = np.empty((nb, n), dtype=ndt), np.empty((nb, nr), dtype=ndt)
        rc, it = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32)
        ptr = lambda x: C.c_void_p(x.ctypes.data)
        ms = L.HOST
    if isinstance(alg, SimpleTrustRegion):
        d = lambda v: -1.0 if v is None else float(v)
        solve_tr = getattr(L.lib(), "nk_batch_solve_trust_region" + ("_nlls" if nlls else "") + ("_f32" if f32 else ""))
        check(solve_tr(h, nb, ptr(u0), 1 if prob.u0_per_system else 0, ptr(pp), ms,
                       0.0 if abstol is None else float(abstol), int(maxiters),
                       d(alg.step_threshold), d(alg.shrink_threshold), d(alg.expand_threshold),
                       d(alg.shrink_factor), d(alg.expand_factor), int(alg.max_shrink_times),
                       ptr(u), ptr(r), ptr(rc), ptr(it)))
    elif isinstance(alg, (SimpleBroyden, SimpleKlement, SimpleDFSane)):
        sfx = "_f32" if f32 else ""
        head = (h, nb, ptr(u0), 1 if prob.u0_per_system else 0, ptr(pp), ms, 0.0 if abstol is None else float(abstol),
                int(maxiters))
        outs = (ptr(u), ptr(r), ptr(rc), ptr(it))
        if isinstance(alg, SimpleBroyden):
            check(getattr(L.lib(), "nk_batch_solve_broyden" + sfx)(*head, -1.0 if alg.alpha is None else float(alg.alpha),
                                                                    *outs))
        elif isinstance(alg, SimpleKlement):
            check(getattr(L.lib(), "nk_batch_solve_klement" + sfx)(*head, *outs))
        else:
            check(getattr(L.lib(), "nk_batch_solve_dfsane" + sfx)(
                *head, float(alg.sigma_min), float(alg.sigma_max), float(alg.sigma_1), int(alg.M), float(alg.gamma),
                float(alg.tau_min), float(alg.tau_max), int(alg.n_exp), *outs))
    else:
        solve = getattr(L.lib(), ("nk_batch_solve_gauss_newton" if nlls else "nk_batch_solve") + ("_f32" if f32 else ""))
        check(solve(h, nb, ptr(u0), 1 if prob.u0_per_system else 0, ptr(pp), ms,
                    0.0 if abstol is None else float(abstol), int(maxiters), ptr(u), ptr(r), ptr(rc), ptr(it)))
    rch = rc.cpu().numpy() if on_dev else rc
    ith = it.cpu().numpy() if on_dev else it
    kernel = (L.lib().nk_batch_last_kernel(h) or b"").decode()
    if per_wavefront and not kernel.endswith("_wave"):
        raise RuntimeError(f"per_wavefront=True, but {kernel} ran: the per-wavefront kernel did not build")
    return EnsembleSolution(u, r, np.asarray(L.RET_NAMES)[rch], ith.copy(), rch.copy(), kernel)


# ------------------------------------------------------------------------------------------- Jacobian operators
class JacobianOperator:
    """JacobianOperator(prob, fu, u): JVP by default, `.T` flips to VJP
    (lib/SciMLJacobianOperators/src/SciMLJacobianOperators.jl:86-143)."""

    def __init__(self, prob: NonlinearProblem, fu=None, u=None, mode: str = "jvp"):
        self.prob, self.mode = prob, mode
        n = prob.device_problem.n_local
        self.size = (n, n)

    @property
    def T(self):
        return JacobianOperator(self.prob, mode="vjp" if self.mode == "jvp" else "jvp")

    adjoint = transpose = T

    def __call__(self, v, u, p=None):  # (op::JacobianOperator)(v, u, p)
        dp = self.prob.device_problem
        return dp.jvp(v, u) if self.mode == "jvp" else dp.vjp(v, u)


def JacVecOperator(prob, fu=None, u=None):
    return JacobianOperator(prob, fu, u, "jvp")


def VecJacOperator(prob, fu=None, u=None):
    return JacobianOperator(prob, fu, u, "vjp")


class StatefulJacobianOperator:
    """StatefulJacobianOperator(jac_op, u, p) with `*` / mul! (SciMLJacobianOperators.jl:210-243)."""

    def __init__(self, jac_op: JacobianOperator, u, p=None):
        self.jac_op, self.u, self.p, self.mode = jac_op, u, p, jac_op.mode

    @property
    def T(self):
        return StatefulJacobianOperator(self.jac_op.T, self.u, self.p)

    def __matmul__(self, v):
        if isinstance(v, StatefulJacobianOperator):
            return StatefulJacobianNormalFormOperator(self, v)
        return self.jac_op(v, self.u, self.p)

    __mul__ = __matmul__

    def mul_(self, out, v):  # mul!(Jv, J, v)
        r = self @ v
        if _is_torch(out):
            out.copy_(r)
        else:
            out[...] = r
        return out


class StatefulJacobianNormalFormOperator:
    """JᵀJ x via JVP then VJP (SciMLJacobianOperators.jl:252-291)."""

    def __init__(self, vjp_op, jvp_op):
        self.vjp_operator, self.jvp_operator = vjp_op, jvp_op

    def __matmul__(self, x):
        return self.vjp_operator @ (self.jvp_operator @ x)

    __mul__ = __matmul__
