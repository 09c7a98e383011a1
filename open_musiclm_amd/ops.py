"""Tensor-level wrappers over the C ABI (include/omlm.h).  No autograd, no fallbacks.

dtype code convention (include/omlm.h): 0 = fp32 ("bf16x3" split for GEMM/attention operands), 1 = bf16, 2 = fp16.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import NamedTuple, Optional, Sequence

import torch

from . import hip
from .ema import check_ema_settings
from .hip import call, ptr, stream_ptr

F32, BF16, F16 = 0, 1, 2
_CODES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
H16 = (torch.bfloat16, torch.float16)            # the 16-bit GEMM / attention operand types (precision "bf16" / "fp16")


def dcode(dtype: torch.dtype) -> int:
    try:
        return _CODES[dtype]
    except KeyError:
        raise TypeError(f"unsupported operand dtype {dtype}") from None


def tdtype(code: int) -> torch.dtype:
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[code]


def _chk(t: torch.Tensor, name: str):
    hip.require_gpu(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


# ---- bf16x3 through the bf16 tile kernels: fp32 operands are split once into bf16 hi / lo planes (omlm_split_planes) and the
# three products run as ONE GEMM with a 3x longer k-loop (omlm_gemm_planes).  The register-staged fp32 kernel measured 169
# TFLOP/s fp32-equivalent on the trunk shapes; the plane form runs at a third of the bf16 kernels' ~1 PFLOP/s.
# Planes are cached ONLY inside a plane scope (planes_begin .. planes_end: one forward + its backward, opened by the engine), so an
# activation feeding its forward, input-gradient and weight-gradient GEMMs is split once -- and nothing survives the scope: the
# kernels (and the fused optimizer) write tensors through raw pointers without bumping torch's version counter, so a cache that
# outlives the step would hand out planes of last step's weights (a captured HIP graph would additionally have lost the split
# launches: they ran during the eager warm-up).  Every scope starts empty, i.e. the split kernels of a captured micro-step are part
# of its graph and read the current weights on every replay.  Outside a scope (direct ops.gemm calls) nothing is cached.
# OMLM_X3_PLANES=0 keeps every fp32 GEMM on the register-staged kernel.
_X3_PLANES = os.environ.get("OMLM_X3_PLANES", "1") == "1"
_X3_MIN_MACS = 1 << 26
_PLANES = {}
_PLANE_SCOPE = [0]                 # > 0 while the engine sequences a forward / backward


def planes_begin():
    """Open a plane scope (engine.run_forward): the cache starts empty."""
    _PLANES.clear()
    _PLANE_SCOPE[0] = 1


def planes_end():
    """Close the scope (end of the backward, or of a forward that saves nothing): every cached plane is dropped."""
    _PLANES.clear()
    _PLANE_SCOPE[0] = 0


def operand_planes(t: torch.Tensor, rows: int, ld: int):
    """(planes buffer, byte distance hi -> lo) for the fp32 region rows x ld at t's data pointer."""
    n = int(rows) * int(ld)
    key = id(t)
    scoped = _PLANE_SCOPE[0] > 0
    if scoped:
        ent = _PLANES.get(key)
        if ent is not None and ent[0]() is t and ent[1] == t._version and ent[2] == (t.data_ptr(), n):
            return ent[3], ent[4]
    pe = (n + 7) // 8 * 8
    buf = torch.empty(2 * pe, dtype=torch.bfloat16, device=t.device)
    call("omlm_split_planes", ptr(t), ptr(buf), n, pe, stream_ptr())
    if scoped:
        try:
            ref = weakref.ref(t, lambda _r, k=key: _PLANES.pop(k, None))
            _PLANES[key] = (ref, t._version, (t.data_ptr(), n), buf, pe * 2)
        except TypeError:
            pass
    return buf, pe * 2


_TAIL_WS = {}                  # (device index, stream) -> workspace of the GEMM tails' deterministic split-K: a per-call argument of the library
_TAIL_WS_BYTES = int(os.environ.get("OMLM_GEMM_TAIL_WS_MB", "64")) << 20


def tail_workspace(device: torch.device):
    """(pointer, bytes) of the CURRENT stream's split-K scratch on `device` (include/omlm.h: the buffer belongs to the call, one per stream that
    launches GEMMs concurrently).  A stream that is capturing gets its own buffer from the graph's pool: it lives as long as the graph that
    replays its launches."""
    if _TAIL_WS_BYTES <= 0:
        return None, 0
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(device).cuda_stream)
    buf = _TAIL_WS.get(key)
    if buf is None:
        buf = _TAIL_WS[key] = torch.empty(_TAIL_WS_BYTES // 4, device=device)
    return ptr(buf), _TAIL_WS_BYTES


def gemm(A: torch.Tensor, B: torch.Tensor, C_: torch.Tensor, *, M: int, N: int, K: int,
         lda: Optional[int] = None, ldb: Optional[int] = None, ldc: Optional[int] = None,
         a_kmajor: bool = False, b_kmajor: bool = False, Cin: Optional[torch.Tensor] = None,
         ldcin: Optional[int] = None, a_map=None, b_map=None, c_map=None, alpha: float = 1.0,
         a_rows: Optional[int] = None, b_rows: Optional[int] = None, planes: bool = True):
    """C[m,n] = alpha * sum_k A(m,k) B(n,k) (+ Cin).  A, B share dtype (bf16 or fp32); C is fp32 or bf16.
    planes=False keeps fp32 operands on the register-staged kernel (no hi/lo plane buffers, no plane cache)."""
    hip.require_gpu(A, "A")
    assert A.dtype == B.dtype, (A.dtype, B.dtype)
    lda = lda if lda is not None else A.shape[-1]
    ldb = ldb if ldb is not None else B.shape[-1]
    ldc = ldc if ldc is not None else C_.shape[-1]
    if Cin is not None:
        assert Cin.dtype == torch.float32
        ldcin = ldcin if ldcin is not None else Cin.shape[-1]
    a_rows = a_rows if a_rows is not None else A.numel() // lda
    b_rows = b_rows if b_rows is not None else B.numel() // ldb
    ws, wsb = tail_workspace(A.device) if (A.dtype in H16 or A.dtype == torch.float32) else (None, 0)
    if (A.dtype == torch.float32 and planes and _X3_PLANES and M * N * K >= _X3_MIN_MACS and not (a_kmajor and a_map is not None)
            and not (b_kmajor and b_map is not None) and (a_kmajor and b_kmajor or K % 8 == 0)):
        pa, sa = operand_planes(A, a_rows, lda)
        pb, sb = operand_planes(B, b_rows, ldb)
        call("omlm_gemm_planes", ptr(pa), sa, ptr(pb), sb, ptr(C_), ptr(Cin), ptr(a_map), ptr(b_map), ptr(c_map),
             a_rows, b_rows, M, N, K, lda, ldb, ldc, ldcin or 0, int(a_kmajor), int(b_kmajor), dcode(C_.dtype), float(alpha),
             ws, wsb, stream_ptr())
        return
    call("omlm_gemm", ptr(A), ptr(B), ptr(C_), ptr(Cin), ptr(a_map), ptr(b_map), ptr(c_map),
         a_rows, b_rows, M, N, K, lda, ldb, ldc, ldcin or 0, int(a_kmajor), int(b_kmajor),
         dcode(A.dtype), dcode(C_.dtype), float(alpha), ws, wsb, stream_ptr())


def gemm_planes16(A, A_lo, B, B_lo, C_, C_lo=None, *, M: int, N: int, K: int, Cin: Optional[torch.Tensor] = None, a_map=None, c_map=None,
                  ldc: Optional[int] = None, a_rows: Optional[int] = None, b_rows: Optional[int] = None):
    """C = A B^T (+ Cin) with both operands as hi/lo planes of ONE 16-bit type (A [M, K], B [N, K] row-major; omlm_gemm_planes16): three
    products, fp32 accumulation.  C_lo None: C is fp32.  C_lo given: C / C_lo receive the result as planes of the operand type.
    a_map / c_map: row maps as in gemm (physical row of logical row m in A's planes / in C and Cin)."""
    hip.require_gpu(A, "A")
    assert A.dtype in H16 and A_lo.dtype == A.dtype and B.dtype == A.dtype and B_lo.dtype == A.dtype
    assert A_lo.shape == A.shape and B_lo.shape == B.shape
    if C_lo is None:
        assert C_.dtype == torch.float32 and (Cin is None or Cin.dtype == torch.float32)
    else:
        assert C_.dtype == A.dtype and C_lo.dtype == A.dtype and C_lo.shape == C_.shape and Cin is None
    lda, ldb = A.shape[-1], B.shape[-1]
    ldc = ldc if ldc is not None else C_.shape[-1]
    ws, wsb = tail_workspace(A.device)
    call("omlm_gemm_planes16", ptr(A), ptr(A_lo), ptr(B), ptr(B_lo), ptr(C_), ptr(C_lo), ptr(Cin), ptr(a_map), ptr(c_map),
         a_rows if a_rows is not None else A.numel() // lda, b_rows if b_rows is not None else B.numel() // ldb,
         M, N, K, lda, ldb, ldc, Cin.shape[-1] if Cin is not None else 0, dcode(A.dtype), ws, wsb, stream_ptr())


class Fp8Planes:
    """The fp8 companions of a half operand [rows, ld] for omlm_gemm_mx16: planes [2, rows padded to 256, 2 ld] bytes (hi8, lo8; element k of a row
    at byte k, zero up to the next multiple of 128) and one E8M0 scale byte per row.  Written by layernorm_fwd_mx / ffmid_fwd_mx (which also
    write their rows' zero tails: zero=False is enough for them) / QuantRowsGroup (weights: persistent, zero-filled once)."""
    __slots__ = ("planes", "scale", "rows", "ld")

    def __init__(self, rows: int, ld: int, device, zero: bool = True):
        self.rows, self.ld = int(rows), int(ld)
        rp = (self.rows + 255) // 256 * 256
        # bytes [K, ceil128(K)) of every real row must be zeros (an fp8 NaN byte there would poison the row's outputs); pad rows and their
        # scales only ever reach output rows >= M, which no epilogue stores
        self.planes = (torch.zeros if zero else torch.empty)(2, rp, 2 * self.ld, dtype=torch.uint8, device=device)
        self.scale = (torch.full((rp,), 127, dtype=torch.uint8, device=device) if zero else torch.empty(rp, dtype=torch.uint8, device=device))

    @property
    def stride(self) -> int:
        return self.planes.shape[1] * self.planes.shape[2]


def gemm_mx16(A, A8: Fp8Planes, B, B8: Fp8Planes, C_, C_lo=None, *, M: int, N: int, K: int, Cin: Optional[torch.Tensor] = None):
    """C = A B^T (+ Cin): the half product of the hi planes plus the two correction products on fp8 at twice the matrix rate (omlm_gemm_mx16).
    C_lo: plane output -- a half tensor, or a uint8 tensor of C's shape for the lo plane as bf8 (e5m2) bytes."""
    hip.require_gpu(A, "A")
    assert A.dtype == torch.float16 and B.dtype == torch.float16
    lda, ldb = A.shape[-1], B.shape[-1]
    assert A8.ld == lda and B8.ld == ldb and A8.rows >= M and B8.rows >= N
    if C_lo is None:
        assert C_.dtype == torch.float32 and (Cin is None or Cin.dtype == torch.float32)
    else:
        assert C_.dtype == A.dtype and C_lo.dtype in (A.dtype, torch.uint8) and C_lo.shape == C_.shape and Cin is None
    ws, wsb = tail_workspace(A.device)
    call("omlm_gemm_mx16", ptr(A), ptr(A8.planes), A8.stride, ptr(A8.scale), ptr(B), ptr(B8.planes), B8.stride, ptr(B8.scale),
         ptr(C_), ptr(C_lo), int(C_lo is not None and C_lo.dtype == torch.uint8), ptr(Cin), A.numel() // lda, B.numel() // ldb, M, N, K, lda, ldb, C_.shape[-1],
         Cin.shape[-1] if Cin is not None else 0, ws, wsb, stream_ptr())


class _DescGroup:
    """What the descriptor groups share.  add() appends an item: the fields of `desc` in order, tensors in the place of their pointers (they
    stay alive until the flush).  flush() issues all items as ONE call of `entry` (descriptor array, count, args, dtype code where the group
    has one operand / output type, stream) and empties the group."""
    desc = entry = dtype = None

    def __init__(self):
        self.items = []

    def _fields(self, item):
        return [ptr(v) if v is None or isinstance(v, torch.Tensor) else v for v in item]

    def flush(self, *args):
        if not self.items:
            return
        arr = (self.desc * len(self.items))(*[self.desc(*self._fields(it)) for it in self.items])
        call(self.entry, C.cast(arr, C.c_void_p), len(arr), *args, *([] if self.dtype is None else [dcode(self.dtype)]), stream_ptr())
        self.items = []


class _WgradDesc(C.Structure):
    """omlm_gemm_wgrad_desc (include/omlm.h)"""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("c_map", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int)]


class WgradGroup(_DescGroup):
    """Collects the weight-gradient contractions dW[M,N] += dY[K,M]^T X[K,N] of a backward pass (16-bit operands of ONE type, rows =
    tokens) and issues them as ONE grouped launch (omlm_gemm_wgrad_group).  The operands are kept alive until :meth:`flush`."""
    desc, entry = _WgradDesc, "omlm_gemm_wgrad_group"

    def add(self, dY: torch.Tensor, X: torch.Tensor, dW: torch.Tensor, *, M: int, N: int, K: int, c_map=None):
        hip.require_gpu(dY, "dY")
        assert dY.dtype in H16 and X.dtype == dY.dtype and dW.dtype == torch.float32
        assert self.dtype in (None, dY.dtype), "one operand type per group"
        self.dtype = dY.dtype
        self.items.append((dY, X, dW, c_map, M, N, K, dY.shape[-1], X.shape[-1], dW.shape[-1]))

    def flush(self, splits: int = 0):
        super().flush(int(splits))


class _CastDesc(C.Structure):
    """omlm_cast_pad_desc (include/omlm.h)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("R", C.c_int), ("C", C.c_int), ("ld_src", C.c_int), ("ld_dst", C.c_int),
                ("transpose", C.c_int), ("lo", C.c_int)]


class CastPadGroup(_DescGroup):
    """Collects weight re-packs (cast_pad problems, plain or transposed, with ONE output type) and issues them as one launch."""
    desc, entry = _CastDesc, "omlm_cast_pad_group"

    def add(self, src, dst, R, C_, ld_src, ld_dst, transpose=False, lo=False):
        """lo: dst receives the lo plane rne16(v - rne16(v)) of the cast (the hi/lo weight planes of precision "fp16ff")."""
        hip.require_gpu(src, "src")
        assert src.dtype == torch.float32 and self.dtype in (None, dst.dtype), "fp32 sources, one output type per group"
        self.dtype = dst.dtype
        self.items.append((src, dst, int(R), int(C_), int(ld_src), int(ld_dst), int(bool(transpose)), int(bool(lo))))


def _seg_rows(x, y, seg, xc):
    """A row segment (n_full, p0, n_live) of x [B * n_full, D] (include/omlm.h, "Row segments"): the compact row count, checked against the outputs."""
    n_full, p0, n_live = seg
    assert x.shape[0] % n_full == 0 and p0 + n_live == n_full and p0 > 0
    M = x.shape[0] // n_full * n_live
    assert y.shape[0] == M and (xc is None or (xc.shape == (M, x.shape[1]) and xc.dtype == torch.float32))
    return M


def layernorm_fwd(x, gamma, y, xcast, mean, rstd, eps=1e-5, seg=None, xc=None):
    """seg (n_full, p0, n_live): x is read at the segment's rows and y, mean, rstd leave compact ([B * n_live, ..]); xc (optional) receives the
    fp32 source rows compact in the same pass."""
    M, D = x.shape
    if seg is not None:
        assert xcast is None and mean.numel() == rstd.numel() == y.shape[0]
        call("omlm_layernorm_fwd_seg", ptr(x), ptr(gamma), ptr(y), None, ptr(mean), ptr(rstd), ptr(xc),
             _seg_rows(x, y, seg, xc), D, y.shape[-1], float(eps), dcode(y.dtype), *seg, stream_ptr())
        return
    call("omlm_layernorm_fwd", ptr(x), ptr(gamma), ptr(y), ptr(xcast), ptr(mean), ptr(rstd),
         M, D, y.shape[-1], float(eps), dcode(y.dtype), stream_ptr())


def layernorm_fwd_planes(x, gamma, y, y_lo, mean, rstd, eps=1e-5, seg=None, xc=None):
    """layernorm_fwd with the result as hi/lo planes of y's 16-bit type: y = rne16(v), y_lo = rne16(v - y) (omlm_layernorm_fwd_planes)."""
    M, D = x.shape
    assert y.dtype in H16 and y_lo.dtype == y.dtype and y_lo.shape == y.shape
    if seg is not None:
        assert mean.numel() == rstd.numel() == y.shape[0]
        call("omlm_layernorm_fwd_planes_seg", ptr(x), ptr(gamma), ptr(y), ptr(y_lo), ptr(mean), ptr(rstd), ptr(xc),
             _seg_rows(x, y, seg, xc), D, y.shape[-1], float(eps), dcode(y.dtype), *seg, stream_ptr())
        return
    call("omlm_layernorm_fwd_planes", ptr(x), ptr(gamma), ptr(y), ptr(y_lo), ptr(mean), ptr(rstd),
         M, D, y.shape[-1], float(eps), dcode(y.dtype), stream_ptr())


def layernorm_fwd_mx(x, gamma, y, P: "Fp8Planes", mean, rstd, eps=1e-5, seg=None, xc=None):
    """layernorm_fwd with y as omlm_gemm_mx16's A operand: the half hi plane y (bit for bit layernorm_fwd's) + its fp8 planes and row scales in P."""
    M, D = x.shape
    if seg is not None:
        M = _seg_rows(x, y, seg, xc)
        assert y.dtype == torch.float16 and P.ld == y.shape[-1] and P.rows >= M and mean.numel() == rstd.numel() == M
        call("omlm_layernorm_fwd_mx_seg", ptr(x), ptr(gamma), ptr(y), ptr(P.planes), P.stride, ptr(P.scale), ptr(mean), ptr(rstd), ptr(xc),
             M, D, y.shape[-1], float(eps), *seg, stream_ptr())
        return
    assert y.dtype == torch.float16 and P.ld == y.shape[-1] and P.rows >= M
    call("omlm_layernorm_fwd_mx", ptr(x), ptr(gamma), ptr(y), ptr(P.planes), P.stride, ptr(P.scale), ptr(mean), ptr(rstd),
         M, D, y.shape[-1], float(eps), stream_ptr())


class _QuantDesc(C.Structure):
    """omlm_quant_rows_desc (include/omlm.h)"""
    _fields_ = [("src", C.c_void_p), ("dst8", C.c_void_p), ("lo_stride", C.c_longlong), ("scale8", C.c_void_p),
                ("R", C.c_int), ("C", C.c_int), ("ld_src", C.c_int), ("ld8", C.c_int)]


class QuantRowsGroup(_DescGroup):
    """Collects the fp8 re-packs of fp32 weights (rows [row0, row0 + R) of an Fp8Planes from src [R, C]) and issues them as one launch."""
    desc, entry = _QuantDesc, "omlm_quant_rows_mx"

    def add(self, src, P: "Fp8Planes", row0: int, R: int, C_: int, ld_src: int):
        hip.require_gpu(src, "src")
        assert src.dtype == torch.float32 and row0 + R <= P.rows and C_ <= 2 * P.ld
        self.items.append((src, P, int(row0), int(R), int(C_), int(ld_src)))

    def _fields(self, item):
        src, P, row0, R, C_, ld_src = item
        pitch = 2 * P.ld
        return ptr(src), P.planes.data_ptr() + row0 * pitch, P.stride, P.scale.data_ptr() + row0, R, C_, ld_src, pitch


_LN_WS = {}
LN_BWD_PARTIAL_ROWS = 2048      # a two-level LayerNorm backward leaves min(M, this) partial d(gamma) rows, one per workgroup (csrc/norm_plan.h: LN_GRID)


def _ln_workspace(D: int, device) -> torch.Tensor:
    key = (D, str(device))
    if key not in _LN_WS:
        _LN_WS[key] = torch.empty(int(hip.lib().omlm_layernorm_bwd_workspace_bytes(D)) // 4, device=device)
    return _LN_WS[key]


class _ColsumDesc(C.Structure):
    """omlm_colsum_desc (include/omlm.h)"""
    _fields_ = [("part", C.c_void_p), ("out", C.c_void_p), ("P", C.c_int), ("C", C.c_int), ("ldp", C.c_int)]


class ColsumGroup(_DescGroup):
    """Collects column sums out[c] += sum_p part[p, c] (the d(gamma) partial rows of the LayerNorm backwards of one backward pass) and issues
    them as ONE launch (omlm_colsum_group).  The partial buffers are kept alive until :meth:`flush`."""
    desc, entry = _ColsumDesc, "omlm_colsum_group"

    def add(self, part: torch.Tensor, out: torch.Tensor, P: int, C_: int, ldp: int):
        self.items.append((part, out, int(P), int(C_), int(ldp)))


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dx, dxcast, dgamma, dx_scale=1.0, dres2=None, defer: Optional["ColsumGroup"] = None, seg=None):
    """dres2 (optional): a second residual-gradient term in the cast type (dxcast's dtype; with dxcast None its own dtype names it).
    defer: the d(gamma) partial rows stay in a workspace of this call's own and their column sum joins the group's one launch.
    seg (n_full, p0, n_live): dy, x, the statistics and dres are compact ([B * n_live, ..]); dx / dxcast are full-size ([B * n_full, D]): the
    segment's rows are written, the rows in front of it as zeros by the same launch (no dres2)."""
    M, D = x.shape
    if seg is not None:
        n_full, p0, n_live = seg
        assert dres2 is None and M % n_live == 0 and p0 + n_live == n_full and dy.shape[0] == M
        assert dx.shape[0] == M // n_live * n_full and (dxcast is None or dxcast.shape[0] == dx.shape[0]) and (dres is None or dres.shape[0] == M)
    code = dcode(dxcast.dtype) if dxcast is not None else (dcode(dres2.dtype) if dres2 is not None else F32)
    assert dres2 is None or dcode(dres2.dtype) == code, "dres2 must have the cast type"
    deferred = dgamma is not None and defer is not None
    rows = min(M, LN_BWD_PARTIAL_ROWS)
    if deferred:
        ws = torch.empty(rows * D, device=x.device)     # private, alive until the group's flush: one partial row per workgroup (min(M, 2048) of them)
    else:
        ws = _ln_workspace(D, x.device) if dgamma is not None else None       # stream-ordered reuse: one backward at a time
    if seg is not None:
        call("omlm_layernorm_bwd2_seg", ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), None, ptr(dx),
             ptr(dxcast), ptr(None if deferred else dgamma), ptr(ws), M, D, float(dx_scale), dcode(dy.dtype) if dxcast is None else code,
             dcode(dy.dtype), *seg, stream_ptr())
    else:
        call("omlm_layernorm_bwd2", ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dres2), ptr(dx),
             ptr(dxcast), ptr(None if deferred else dgamma), ptr(ws), M, D, float(dx_scale), code, dcode(dy.dtype), stream_ptr())
    if deferred:
        defer.add(ws, dgamma, rows, D, D)


def qk_norm_fwd(q_raw, kv_raw, q_scale, k_scale, q, k, v, H):
    call("omlm_qk_norm_fwd", ptr(q_raw), ptr(kv_raw), ptr(q_scale), ptr(k_scale), ptr(q), ptr(k), ptr(v),
         q_raw.shape[0], H, dcode(q.dtype), stream_ptr())


def qk_norm_bwd(dq, dk, dv, q_raw, kv_raw, q_scale, k_scale, dq_raw, dkv_raw, dq_scale, dk_scale, H):
    call("omlm_qk_norm_bwd", ptr(dq), ptr(dk), ptr(dv), ptr(q_raw), ptr(kv_raw), ptr(q_scale), ptr(k_scale),
         ptr(dq_raw), ptr(dkv_raw), ptr(dq_scale), ptr(dk_scale), q_raw.shape[0], H, dcode(dq_raw.dtype), stream_ptr())


_DBIAS_WS = {}
_DBIAS_RETIRED = []            # outgrown workspaces stay alive (captured graphs may still point at them)


def gemm_qknorm(A, B, C_, scale, norm_out, groups, *, M, N, K, C2=None, c2_col0=0):
    """C = per-head l2-normalised, scaled A B^T in the 16-bit operand type (omlm_gemm_qknorm); norm_out [M, >= groups] fp32."""
    hip.require_gpu(A, "A")
    assert A.dtype in H16 and B.dtype == A.dtype and C_.dtype == A.dtype and norm_out.dtype == torch.float32 and scale.dtype == torch.float32
    assert C2 is None or C2.dtype == A.dtype
    call("omlm_gemm_qknorm", ptr(A), ptr(B), ptr(C_), ptr(C2), int(c2_col0), C2.shape[-1] if C2 is not None else 0, ptr(scale), ptr(norm_out),
         norm_out.shape[-1] if norm_out.dim() > 1 else 1, int(groups), A.numel() // A.shape[-1], B.numel() // B.shape[-1], M, N, K,
         A.shape[-1], B.shape[-1], C_.shape[-1], dcode(A.dtype), stream_ptr())


def qk_norm_bwd2(dq, dk, dv, q, k, qn, kn, q_scale, k_scale, dq_raw, dkv_raw, dq_scale, dk_scale, H):
    call("omlm_qk_norm_bwd2", ptr(dq), ptr(dk), ptr(dv), ptr(q), ptr(k), ptr(qn), ptr(kn), ptr(q_scale), ptr(k_scale),
         ptr(dq_raw), ptr(dkv_raw), ptr(dq_scale), ptr(dk_scale), q.shape[0], H, dcode(dq_raw.dtype), stream_ptr())


class AttnBias:
    """Rel-pos bias table of one attention layer in the two layouts the kernels read: `table` [N + min(P, N) - 1, ld] fp32 (row =
    i - j + min(P, N) - 1, column = head; include/omlm.h) and `tableT`, its transposed / zero-padded / log2(e)-scaled form
    (omlm_attn_bias_prepare).  P: the non-causal prefix the layout is for (0: causal); attn_fwd / attn_bwd take it only with the same P.

    q_scale / k_scale (the layer's learned per-dim scales) or qk_bound (an explicit bound on |q . k|, e.g. 1.0 for unit vectors)
    let the 16-bit forward take its exponentials against a fixed reference point instead of a running maximum; without either the
    online softmax runs.  half=True (fp16 attention operands): the reference point sits 15 octaves lower, so the probability numerators
    span half's normal range instead of sitting at its bottom (the kernels fall back to the online softmax if the scales grow too wide)."""

    def __init__(self, table: Optional[torch.Tensor], N: int, H: int, device=None, q_scale=None, k_scale=None,
                 qk_bound: float = 0.0, scale: float = 8.0, half: bool = False, _tableT: Optional[torch.Tensor] = None, _P: int = 0):
        self.table, self.N, self.H, self.P = table, N, H, _P
        dev = table.device if table is not None else device
        if _tableT is not None:                         # (AttnBias.group: the table was written by the grouped launch)
            self.tableT = _tableT
            return
        self.tableT = torch.empty(int(hip.lib().omlm_attn_bias_table_floats(N, H, 0)), device=dev)
        call("omlm_attn_bias_prepare", ptr(table), ptr(self.tableT), N, H, table.shape[-1] if table is not None else 0,
             ptr(q_scale), ptr(k_scale), float(qk_bound), float(scale), 15 if half else 0, stream_ptr())

    @staticmethod
    def group(table: Optional[torch.Tensor], N: int, H: int, device, q_scales, k_scales, scale: float = 8.0, half: bool = False, P: int = 0):
        """One AttnBias per layer (q_scales[l], k_scales[l]) over the same rel-pos table, written by ONE launch
        (omlm_attn_bias_prepare_group) instead of one small launch per layer.  P >= 1: the non-causal prefix's layout."""
        L = len(q_scales)
        dev = table.device if table is not None else device
        buf = torch.empty(L, int(hip.lib().omlm_attn_bias_table_floats(N, H, P)), device=dev)
        outs = (C.c_void_p * L)(*[buf[l].data_ptr() for l in range(L)])
        qs = (C.c_void_p * L)(*[t.data_ptr() for t in q_scales])
        ks = (C.c_void_p * L)(*[t.data_ptr() for t in k_scales])
        for t in list(q_scales) + list(k_scales):
            hip.require_gpu(t, "scale")
        call("omlm_attn_bias_prepare_group", ptr(table), C.cast(outs, C.c_void_p), L, N, H, table.shape[-1] if table is not None else 0,
             C.cast(qs, C.c_void_p), C.cast(ks, C.c_void_p), 0.0, float(scale), 15 if half else 0, int(P), stream_ptr())
        return [AttnBias(table, N, H, dev, _tableT=buf[l], _P=P) for l in range(L)]


def _attn_tables(bias, N, H, P, device):
    """(table, tableT) for the C entries from attn_fwd's / attn_bwd's bias argument.  A raw table (or None) is prepared here for P = 0 --
    one prepare launch, after which 16-bit operands run the second-generation kernels with the online softmax -- but handed over as it is
    for P >= 1, which runs the first-generation kernels.  That asymmetry is a route of its own; keep it unless the routes are meant to change."""
    if isinstance(bias, AttnBias):
        if bias.P != P:
            raise ValueError(f"attention with P = {P} handed an AttnBias prepared for P = {bias.P}")
        return bias.table, bias.tableT
    return bias, (AttnBias(bias, N, H, device).tableT if P == 0 else None)


def _dbias_workspace(B: int, N: int, H: int, device) -> torch.Tensor:
    """Scratch for the backward's d(bias) partial rows (omlm_mqa_attn_bwd_workspace_bytes): ONE buffer per device, shared by every
    layer and every step (the reduction kernel of a layer consumes it before the next layer's dQ kernel writes it: stream order;
    like _ln_workspace it assumes one backward at a time per device).  It is quadratic in N (B H ceil(N/32)^2 128 bytes: 40 MB at
    B = 32, N = 1116), so one copy per layer was 24 x 53 MB for the musiclm_large leg.  Past N = 4096 it also holds the dK / dV kernel's
    slots (include/omlm.h)."""
    n = int(hip.lib().omlm_mqa_attn_bwd_workspace_bytes(B, N, H)) // 4
    key = str(device)
    ws = _DBIAS_WS.get(key)
    if ws is None or ws.numel() < n:
        if ws is not None:
            # a captured HIP graph (graph.py) holds the OLD buffer's address in its kernel nodes: a regrown workspace must not free
            # it, or later replays would write d(bias) partials into memory the allocator has handed to someone else
            _DBIAS_RETIRED.append(ws)
        ws = _DBIAS_WS[key] = torch.empty(n, device=device, dtype=torch.float32)
    return ws


def attn_max_positions(dtype, P: int = 0) -> int:
    """Most positions per sample attn_fwd + attn_bwd take for operands of `dtype` with a prefix of P rows (omlm_attn_max_positions)."""
    return int(hip.lib().omlm_attn_max_positions(dcode(dtype), int(P)))


def _check_positions(what, N, dtype, P):
    """16-bit causal attention past its ceiling is refused here, before the bias table is prepared (the library refuses every other case
    itself, with the limit of the route the call would take)."""
    if P == 0 and dtype in H16 and N > attn_max_positions(dtype, 0):
        raise RuntimeError(f"{what}: N = {N} positions per sample is past the limit of {attn_max_positions(dtype, 0)} "
                           f"(omlm_attn_max_positions) of causal attention with {dtype} operands")


def attn_fwd(q, k, v, bias, keymask, out, lse, B, N, H, scale, P=0, p=0.0, seed=0, seed_dev=None):
    """Attention with a non-causal prefix of P rows (omlm_mqa_attn_fwd; 0: causal): score (i, j) is live iff j <= i or i, j < P.
    bias: an AttnBias of the layout for P (built once per forward by the engine: AttnBias.group(..., P=P)), a raw [N + min(P, N) - 1, ld]
    fp32 rel-pos table (row i - j + min(P, N) - 1, relpos_forward with P), or None.
    p > 0: dropout on the probabilities with the keep-mask of include/omlm.h (seed, optional device salt seed_dev: int64 [1])."""
    _check_positions("attn_fwd", N, q.dtype, P)
    table, tableT = _attn_tables(bias, N, H, P, q.device)
    call("omlm_mqa_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(table), ptr(tableT), ptr(keymask), ptr(out), ptr(lse), B, N, H, float(scale),
         table.shape[-1] if table is not None else 0, dcode(q.dtype), int(P), float(p), int(seed), ptr(seed_dev), stream_ptr())


def attn_bwd(q, k, v, bias, keymask, out, dout, lse, delta, dq, dk, dv, dbias, B, N, H, scale, P=0, workspace=True, p=0.0, seed=0,
             seed_dev=None):
    """Backward of attn_fwd.  bias: the forward's (an AttnBias: its tableT carries the reference point lse is relative to).  dbias: the raw
    table's layout (accumulated, +=), or None.  workspace=False: d(bias) by device-scope atomics straight into the table (the C ABI's
    null-workspace form; slower).  P, p, seed, seed_dev: those of the forward (the kernels regenerate its keep-mask)."""
    _check_positions("attn_bwd", N, q.dtype, P)
    table, tableT = _attn_tables(bias, N, H, P, q.device)
    ws = _dbias_workspace(B, N, H, q.device) if dbias is not None and workspace else None
    ld = table.shape[-1] if table is not None else (dbias.shape[-1] if dbias is not None else 0)
    call("omlm_mqa_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(table), ptr(tableT), ptr(keymask), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dq),
         ptr(dk), ptr(dv), ptr(dbias), ptr(ws), B, N, H, float(scale), ld, dcode(q.dtype), int(P), float(p), int(seed), ptr(seed_dev),
         stream_ptr())


def attn_dropout_keep(B, N, H, p, seed, seed_dev=None, device=None) -> torch.Tensor:
    """The keep-mask [B, H, N, N] uint8 the attention kernels apply (omlm_attn_dropout_keep; small shapes)."""
    keep = torch.empty(B, H, N, N, dtype=torch.uint8, device=device if device is not None else seed_dev.device)
    call("omlm_attn_dropout_keep", ptr(keep), B, N, H, float(p), int(seed), ptr(seed_dev), stream_ptr())
    return keep


def dropout_residual_fwd(x, y, x1, p, seed, seed_dev=None):
    """x1 = x + keep o y / (1 - p) (to_out dropout), fp32 [M, D]."""
    call("omlm_dropout_residual_fwd", ptr(x), ptr(y), ptr(x1), x.shape[0], x.shape[1], float(p), int(seed), ptr(seed_dev), stream_ptr())


def dropout_residual_bwd(dx1, dy, p, seed, seed_dev=None):
    """dy = keep o dx1 / (1 - p) in dy's dtype; dx1 fp32 [M, D]."""
    call("omlm_dropout_residual_bwd", ptr(dx1), ptr(dy), dx1.shape[0], dx1.shape[1], float(p), int(seed), ptr(seed_dev), dcode(dy.dtype),
         stream_ptr())


def pack_conv_taps(convw: torch.Tensor, F: int, Fp: int) -> torch.Tensor:
    """Reference ds_conv.weight viewed [2F, 3] -> tap-major, padded [3, 2*Fp] in h1's column layout (tiny re-pack)."""
    out = torch.zeros(3, 2 * Fp, device=convw.device, dtype=torch.float32)
    out[:, :F] = convw[:F].t()
    out[:, Fp:Fp + F] = convw[F:].t()
    return out


def pad_vector(v: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, device=v.device, dtype=torch.float32)
    out[: v.numel()] = v
    return out


def _ff_seg(seg, nseq):
    """(n_full, p0) of a row segment for the ConvFeedForward forwards (nseq is its n_live), or (0, 0): none."""
    if seg is None:
        return 0, 0
    assert seg[2] == nseq and seg[1] + seg[2] == seg[0]
    return int(seg[0]), int(seg[1])


def ffmid_fwd(h1, convw, gamma, h2, mean, rstd, nseq, F, Fp, p, seed, eps=1e-5, seed_dev=None, drop_bits=None, gh=None, seg=None):
    """convw: packed taps [3, 2*Fp] (pack_conv_taps); gamma: padded [Fp] (pad_vector).
    seg (n_full, p0, n_live = nseq): the buffers hold rows [p0, n_full) of every sample compact; the keep bits drawn are those of a launch
    over the full rows (include/omlm.h: omlm_ffmid_fwd_seg)."""
    assert convw.shape == (3, 2 * Fp) and gamma.numel() == Fp
    assert convw.dtype == h1.dtype and gamma.dtype == h1.dtype, "taps / gamma travel in the operand dtype of h1"
    call("omlm_ffmid_fwd_seg", ptr(h1), ptr(convw), ptr(gamma), ptr(h2), ptr(mean), ptr(rstd),
         h1.shape[0], nseq, F, Fp, float(eps), float(p), int(seed), ptr(seed_dev), ptr(drop_bits), ptr(gh), dcode(h1.dtype),
         *_ff_seg(seg, nseq), stream_ptr())


def ffmid_fwd_planes(h1, h1_lo, convw, convw_lo, gamma, gamma_lo, h2, h2_lo, mean, rstd, nseq, F, Fp, p, seed, eps=1e-5, seed_dev=None,
                     drop_bits=None, gh=None, seg=None):
    """ffmid_fwd on hi/lo planes (precision "fp16ff"): h1, taps and gamma are read as hi + lo, h2 leaves as planes (omlm_ffmid_fwd_planes)."""
    assert convw.shape == (3, 2 * Fp) and gamma.numel() == Fp and h1.dtype in H16
    for t in (h1_lo, convw, convw_lo, gamma, gamma_lo, h2, h2_lo):
        assert t.dtype == h1.dtype, "every plane travels in the operand dtype of h1"
    assert h1_lo.shape == h1.shape and h2_lo.shape == h2.shape and convw_lo.shape == convw.shape
    call("omlm_ffmid_fwd_planes_seg", ptr(h1), ptr(h1_lo), ptr(convw), ptr(convw_lo), ptr(gamma), ptr(gamma_lo), ptr(h2), ptr(h2_lo), ptr(mean),
         ptr(rstd), h1.shape[0], nseq, F, Fp, float(eps), float(p), int(seed), ptr(seed_dev), ptr(drop_bits), ptr(gh), dcode(h1.dtype),
         *_ff_seg(seg, nseq), stream_ptr())


def ffmid_fwd_mx(h1, h1_lo, convw, convw_lo, gamma, gamma_lo, h2, P: "Fp8Planes", mean, rstd, nseq, F, Fp, p, seed, eps=1e-5, seed_dev=None,
                 drop_bits=None, gh=None, seg=None):
    """ffmid_fwd_planes with h2 leaving as omlm_gemm_mx16's A operand: the half hi plane h2 + its fp8 planes and row scales in P.
    h1_lo: the lo plane of h1 as bf8 bytes (uint8, h1's shape: gemm_mx16's plane output)."""
    assert convw.shape == (3, 2 * Fp) and gamma.numel() == Fp and h1.dtype == torch.float16 and h1_lo.dtype == torch.uint8
    for t in (convw, convw_lo, gamma, gamma_lo, h2):
        assert t.dtype == h1.dtype, "every plane travels in the operand dtype of h1"
    assert h1_lo.shape == h1.shape and convw_lo.shape == convw.shape and P.ld == Fp and P.rows >= h1.shape[0]
    call("omlm_ffmid_fwd_mx_seg", ptr(h1), ptr(h1_lo), ptr(convw), ptr(convw_lo), ptr(gamma), ptr(gamma_lo), ptr(h2), ptr(P.planes), P.stride,
         ptr(P.scale), ptr(mean), ptr(rstd), h1.shape[0], nseq, F, Fp, float(eps), float(p), int(seed), ptr(seed_dev), ptr(drop_bits), ptr(gh),
         *_ff_seg(seg, nseq), stream_ptr())


def ffmid_set_impl(impl: int):
    """0: wave-per-row kernels; 1 (default): column-strip kernels (csrc/ffmid2.hip) wherever their preconditions hold."""
    call("omlm_ffmid_set_impl", int(impl))


def ffmid_bwd_workspace_floats(F, Fp) -> int:
    return int(hip.lib().omlm_ffmid_bwd_workspace_bytes(F, Fp)) // 4


def ffmid_bwd(dh2, h1, convw, gamma, mean, rstd, du_tmp, dh1, dgamma, dconv, workspace, nseq, F, Fp, p, seed, seed_dev=None,
              drop_bits=None, gh=None):
    assert convw.shape == (3, 2 * Fp) and gamma.numel() == Fp
    assert convw.dtype == h1.dtype and gamma.dtype == h1.dtype, "taps / gamma travel in the operand dtype of h1"
    call("omlm_ffmid_bwd", ptr(dh2), ptr(h1), ptr(convw), ptr(gamma), ptr(mean), ptr(rstd), ptr(du_tmp), ptr(dh1),
         ptr(dgamma), ptr(dconv), ptr(workspace), h1.shape[0], nseq, F, Fp, float(p), int(seed), ptr(seed_dev), ptr(drop_bits),
         ptr(gh), dcode(h1.dtype), stream_ptr())


def _ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t) if t is not None else None
    return arr


_INDEX_ERR = {}


def index_error_flag(device) -> torch.Tensor:
    """Per-device int32 flag the gather / cross-entropy kernels OR into when they meet an index past its table (they skip the
    row instead of reading out of bounds).  Reading it synchronises: see :func:`raise_on_index_error`."""
    key = str(device)
    if key not in _INDEX_ERR:
        _INDEX_ERR[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _INDEX_ERR[key]


def raise_on_index_error(device):
    """Raise IndexError if any kernel since the last call met an out-of-range token id / position / label (torch's embedding and
    cross entropy raise a device assert in the same situation).  Synchronises the device: call it where the host already waits
    (the trainer does after every step's loss read-back)."""
    flag = _INDEX_ERR.get(str(device))
    if flag is None:
        return
    v = int(flag.item())
    if v:
        flag.zero_()
        what = [n for b, n in ((1, "token id >= embedding rows"), (2, "position >= absolute position rows"), (4, "label >= vocabulary")) if v & b]
        raise IndexError("open_musiclm_amd: " + ", ".join(what) + " (rows were skipped; check codebook sizes / the token store)")


def _rows_array(tensors):
    if tensors is None:
        return None
    return (C.c_longlong * len(tensors))(*[int(t.shape[0]) if t is not None else 0 for t in tensors])


def embed_fwd(ids, seg, posidx, tables, starts, pos_tables, out):
    B, N = ids.shape
    D = out.shape[-1]
    pos_arr = _ptr_array(pos_tables) if pos_tables is not None else None
    call("omlm_embed_gather_fwd", ptr(ids), ptr(seg), ptr(posidx), _ptr_array(tables), _ptr_array(starts),
         pos_arr, len(tables), ptr(out), B, N, D, _rows_array(tables), _rows_array(pos_tables), ptr(index_error_flag(out.device)),
         stream_ptr())


def embed_bwd(ids, seg, posidx, dtables, dstarts, dpos_tables, dx, alpha):
    B, N = ids.shape
    D = dx.shape[-1]
    pos_arr = _ptr_array(dpos_tables) if dpos_tables is not None else None
    call("omlm_embed_gather_bwd", ptr(ids), ptr(seg), ptr(posidx), _ptr_array(dtables), _ptr_array(dstarts),
         pos_arr, len(dtables), ptr(dx), B, N, D, float(alpha), _rows_array(dtables), _rows_array(dpos_tables),
         ptr(index_error_flag(dx.device)), stream_ptr())


def check_null_cond_prob(p, name="null_cond_prob"):
    """The condition-drop probability as a float: a number in [0, 1), or exactly 1 (every sample; tests).  Anything else raises a
    ValueError that names the argument.  Pure Python: runs before any device work."""
    try:
        v = float("nan") if isinstance(p, (str, bytes, bool)) else float(p)
    except (TypeError, ValueError):
        v = float("nan")
    if not (0.0 <= v <= 1.0):
        raise ValueError(f"{name} must be a number in [0, 1], not {p!r}")
    return v


FP32_MAX = 3.4028234663852886e38            # the largest finite fp32: a scale past it would reach the kernel as inf


def check_cond_scale(cond_scale, name="cond_scale"):
    """The guidance scale as generate / score take it: None -> None (off), 1 -> None (off: g = l), any other finite number >= 0 -> float.
    Anything else (negative, NaN, inf, not a number) raises a ValueError that names the argument.  Pure Python: before any device work."""
    if cond_scale is None:
        return None
    try:
        s = float("nan") if isinstance(cond_scale, (str, bytes, bool)) else float(cond_scale)
    except (TypeError, ValueError):
        s = float("nan")
    if not (0.0 <= s <= FP32_MAX):
        raise ValueError(f"{name} must be None or a finite number >= 0 (as fp32), not {cond_scale!r}")
    return None if s == 1.0 else s


def guide_logits(cond, null, out, V, scale):
    """omlm_guide_logits (include/omlm.h): out[r, c] = null[r, c] + scale * (cond[r, c] - null[r, c]) for c < V, three fp32 roundings.
    cond / null / out: fp32 [rows, ld] of one leading dimension (row-contiguous views such as the halves of a [2P, ld] block); out may be
    cond.  Columns V .. ld - 1 of out are not written.
    scale: a number, or a contiguous fp32 [rows] device tensor -- one scale per row, omlm_guide_logits_rows (its values are the caller's
    to check: per_row_cond_scale)."""
    by_row = isinstance(scale, torch.Tensor) and scale.dim() == 1
    s = None if by_row else check_cond_scale(scale, "scale")
    rows, ld = cond.shape
    if by_row:
        hip.require_gpu(scale, "scale")
        if scale.dtype != torch.float32 or scale.shape != (rows,) or not scale.is_contiguous():
            raise ValueError(f"guide_logits: a per-row scale must be a contiguous fp32 tensor [{rows}]; got {scale.dtype} {tuple(scale.shape)}")
    for t, name in ((cond, "cond"), (null, "null"), (out, "out")):
        hip.require_gpu(t, name)
        if t.dtype != torch.float32 or t.shape != (rows, ld) or t.stride() != (ld, 1):
            raise ValueError(f"guide_logits: {name} must be fp32 [{rows}, {ld}] with contiguous rows; got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if not 0 < int(V) <= ld:
        raise ValueError(f"guide_logits: V must lie in [1, {ld}], not {V}")
    name, args = guide_call(ptr(cond), ptr(null), ptr(out), rows, int(V), ld, scale if by_row else 1.0 if s is None else s)
    call(name, *args, stream_ptr())


def guide_call(cond, null, out, rows, V, ld, scale):
    """The guidance entry for a scale, as (name, arguments in front of the stream): omlm_guide_logits for a number, omlm_guide_logits_rows
    for a [rows] device tensor.  cond / null / out: device addresses.  Nothing is checked or launched here."""
    if isinstance(scale, torch.Tensor):
        return "omlm_guide_logits_rows", (cond, null, out, rows, V, ld, ptr(scale))
    return "omlm_guide_logits", (cond, null, out, rows, V, ld, scale)


def decode_twin(ids=None, ids_twin=None, x=None, x_twin=None):
    """omlm_decode_twin (include/omlm.h): ids_twin[:] = ids (int64 [rows]) and x_twin[:] = x (fp32 [rows, D]) in one launch; either pair may
    be left out."""
    if (ids is None) != (ids_twin is None) or (x is None) != (x_twin is None):
        raise ValueError("decode_twin: give ids with ids_twin and x with x_twin")
    if ids is None and x is None:
        return
    rows = ids.shape[0] if ids is not None else x.shape[0]
    if ids is not None:
        for t in (ids, ids_twin):
            hip.require_gpu(t, "ids")
            assert t.dtype == torch.int64 and t.shape == (rows,) and t.is_contiguous()
    D = 0
    if x is not None:
        D = x.shape[1]
        for t in (x, x_twin):
            hip.require_gpu(t, "x")
            assert t.dtype == torch.float32 and t.shape == (rows, D) and t.is_contiguous()
    call("omlm_decode_twin", ptr(ids), ptr(ids_twin), ptr(x), ptr(x_twin), rows, D, stream_ptr())


def prepare_train_batch(raw_ids, eos_ids, quantizers, codebooks, pad_id, scores, n_drop, want_labels, *, null_u=None, null_p=0.):
    """One launch for the wrapper's id / label / key-mask construction (omlm_prepare_train_batch).  raw_ids: list of int64 [B, len_s]
    contiguous; returns (ids32 [B, N], keymask uint8 [B, N], labels: list of int32 [B, len_s + 1] or None, lens: the per-sequence token
    counts the engine's layout wants -- len_s + 1 for conditioning sequences, len_last for the predicted one).
    null_u (fp32 [B]) with null_p: the condition drop of include/omlm.h -- sample b with null_u[b] < null_p gets the null condition."""
    n = len(raw_ids)
    B, dev = raw_ids[0].shape[0], raw_ids[0].device
    if null_u is not None:
        null_p = check_null_cond_prob(null_p, "null_p")
        if n < 2:
            raise ValueError("prepare_train_batch: the condition drop needs a conditioning sequence (at least two token sequences)")
        hip.require_gpu(null_u, "null_u")
        assert null_u.dtype == torch.float32 and null_u.shape == (B,) and null_u.is_contiguous()
    for t in raw_ids:
        hip.require_gpu(t, "token ids")
        assert t.dtype == torch.int64 and t.dim() == 2 and t.is_contiguous() and t.shape[0] == B
    lens = [int(t.shape[1]) for t in raw_ids]
    N = sum(l + 1 for l in lens) + (n - 1)
    ids32 = torch.empty(B, N, dtype=torch.int32, device=dev)
    keymask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    labels = [torch.empty(B, l + 1, dtype=torch.int32, device=dev) if w else None for l, w in zip(lens, want_labels)]
    arr_i = lambda v: (C.c_int * n)(*[int(x) for x in v])
    call("omlm_prepare_train_batch", _ptr_array(raw_ids), _ptr_array(labels), arr_i(lens), arr_i(eos_ids), arr_i(quantizers), arr_i(codebooks),
         n, B, int(pad_id), ptr(scores), int(n_drop), ptr(ids32), ptr(keymask), N, ptr(null_u), float(null_p) if null_u is not None else 0.,
         stream_ptr())
    return ids32, keymask, labels, [l + 1 for l in lens[:-1]] + [lens[-1]]


def _check_number(x):
    try:
        return float("nan") if isinstance(x, (str, bytes, bool)) else float(x)
    except (TypeError, ValueError):
        return float("nan")


def check_label_smoothing(eps, name="label_smoothing"):
    """The label-smoothing weight as a float: a number in [0, 1) (include/omlm.h; 0: off).  Anything else (negative, 1 and above, NaN,
    inf, not a number) raises a ValueError that names the argument.  Pure Python: runs before any device work."""
    v = _check_number(eps)
    if not (0.0 <= v < 1.0):
        raise ValueError(f"{name} must be a number in [0, 1), not {eps!r}")
    return v


def check_z_loss(zeta, name="z_loss"):
    """The z-loss weight as a float: a finite number >= 0 as fp32 (include/omlm.h; 0: off).  Anything else (negative, NaN, inf, not a
    number) raises a ValueError that names the argument.  Pure Python: runs before any device work."""
    v = _check_number(zeta)
    if not (0.0 <= v <= FP32_MAX):
        raise ValueError(f"{name} must be a finite number >= 0 (as fp32), not {zeta!r}")
    return v


def ce_fwd(logits, labels, row_lse, nll_sum, V, *, label_smoothing=0., z_loss=0.):
    """omlm_cross_entropy_fwd: row_lse written, nll_sum[0] accumulated onto.  With label_smoothing or z_loss set (include/omlm.h) the call
    is omlm_cross_entropy_fwd_reg and `nll_sum` is the 3 floats {nll, smooth, z}; with both 0 it is the call it always was."""
    eps, zeta = check_label_smoothing(label_smoothing), check_z_loss(z_loss)
    R, ld = logits.shape
    if eps == 0.0 and zeta == 0.0:
        call("omlm_cross_entropy_fwd", ptr(logits), ptr(labels), ptr(row_lse), ptr(nll_sum), R, V, ld,
             ptr(index_error_flag(logits.device)), stream_ptr())
        return
    if nll_sum.dtype != torch.float32 or nll_sum.numel() != 3 or not nll_sum.is_contiguous():
        raise ValueError(f"ce_fwd: with label_smoothing / z_loss the sums are 3 contiguous fp32 {{nll, smooth, z}}; got {nll_sum.dtype} {tuple(nll_sum.shape)}")
    call("omlm_cross_entropy_fwd_reg", ptr(logits), ptr(labels), ptr(row_lse), ptr(nll_sum), R, V, ld,
         ptr(index_error_flag(logits.device)), stream_ptr())


def ce_bwd(logits, labels, row_lse, gscale, coef, dlogits, V, *, label_smoothing=0., z_loss=0.):
    """omlm_cross_entropy_bwd; with label_smoothing or z_loss set, omlm_cross_entropy_bwd_reg (the gradient rule of include/omlm.h)."""
    eps, zeta = check_label_smoothing(label_smoothing), check_z_loss(z_loss)
    R, ld = logits.shape
    if eps == 0.0 and zeta == 0.0:
        call("omlm_cross_entropy_bwd", ptr(logits), ptr(labels), ptr(row_lse), ptr(gscale), float(coef), ptr(dlogits),
             R, V, ld, dlogits.shape[-1], dcode(dlogits.dtype), stream_ptr())
        return
    call("omlm_cross_entropy_bwd_reg", ptr(logits), ptr(labels), ptr(row_lse), ptr(gscale), float(coef), ptr(dlogits),
         R, V, ld, dlogits.shape[-1], dcode(dlogits.dtype), eps, zeta, stream_ptr())


METRICS_FILTER_THRES = 0.9                    # generate()'s default filter_thres: what default_metrics_top_k keeps


def default_metrics_top_k(V):
    """The k the sampler keeps of V entries at the default filter_thres = 0.9 -- the expression of utils.top_k (102 at V = 1025)."""
    return max(int((1 - METRICS_FILTER_THRES) * V), 1)


def check_metrics_top_k(k, V, name="metrics_top_k"):
    """The k of the top-k hit counter of the quantizer metrics (include/omlm.h: rank < k) as an int: None -> default_metrics_top_k(V);
    otherwise an integer in [1, V].  Anything else raises a ValueError that names the argument.  Pure Python: before any device work."""
    if k is None:
        return default_metrics_top_k(V)
    if isinstance(k, bool) or not isinstance(k, int) or not (1 <= k <= V):
        raise ValueError(f"{name} must be an integer in [1, {V}] (the entries of a row, eos included) or None, not {k!r}")
    return int(k)


def ce_metrics(logits, labels, V, *, row_nll=None, row_rank=None, row_entropy=None):
    """omlm_ce_metrics over fp32 logits [R, ld] and int32 labels [R]: per live row nll (fp32), the exact rank of the label (int32) and the
    predictive entropy (fp32) into whichever of the three [R] outputs is given (include/omlm.h; ignored rows: 0 / -1 / 0).  Read-only on
    the logits; a label >= V raises the device flag of index_error_flag like the loss."""
    R, ld = logits.shape
    call("omlm_ce_metrics", ptr(logits), ptr(labels), ptr(row_nll), ptr(row_rank), ptr(row_entropy), R, V, ld,
         ptr(index_error_flag(logits.device)), stream_ptr())


def ce_metrics_bins(row_nll, row_rank, row_entropy, labels, n, Q, V, k_top, bins):
    """omlm_ce_metrics_bins: the rows of ce_metrics ([B, n] order) ACCUMULATED onto bins, fp64 [Q + 1, 5] {count, nll, entropy, top1, topk},
    bin t mod Q and bin Q for eos labels, in a fixed order (include/omlm.h)."""
    if bins.dtype != torch.float64 or tuple(bins.shape) != (Q + 1, 5) or not bins.is_contiguous():
        raise ValueError(f"ce_metrics_bins: bins must be contiguous fp64 [{Q + 1}, 5]; got {bins.dtype} {tuple(bins.shape)}")
    call("omlm_ce_metrics_bins", ptr(row_nll), ptr(row_rank), ptr(row_entropy), ptr(labels), labels.numel(), int(n), int(Q), int(V),
         int(k_top), ptr(bins), stream_ptr())


def sumsq_accumulate(g, out, partials=None):
    """out[0] += sum g^2; with `partials` (>= 2048 floats) the reduction order is fixed (bit-reproducible)."""
    call("omlm_sumsq_accumulate", ptr(g), g.numel(), ptr(out), ptr(partials), stream_ptr())


def adamw_clip_step(p, g, m, v, p16, *, lr, beta1, beta2, eps, wd, step, gscale, gnorm_sq, max_norm,
                    decoupled, zero_grad, ls_state=None, ema=None, ema_decay=None, ema_update_after_step=0, ema_warmup=True):
    """p16: optional 16-bit shadow of p (bf16 or fp16: the operand type of the model's precision), written by the same kernel.
    ls_state: the device-side loss-scale block of precision "fp16" (engine.loss_scale_state).
    ema: optional flat fp32 buffer like p that the same launch moves by the EMA rule of include/omlm.h (ema.ema_decay_at); None is the
    call this function always made."""
    args = (ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), p.numel(), float(lr), float(beta1),
            float(beta2), float(eps), float(wd), int(step), float(gscale), ptr(gnorm_sq), float(max_norm or 0.0),
            int(decoupled), int(zero_grad), dcode(p16.dtype) if p16 is not None else BF16, ptr(ls_state))
    if ema is None:
        call("omlm_adamw_clip_step", *args, stream_ptr())
        return
    decay, after, warmup = check_ema_settings(ema_decay, ema_update_after_step, ema_warmup)       # refusals by name, before any device work
    assert ema.dtype == torch.float32 and ema.numel() == p.numel() and ema.device == p.device
    call("omlm_adamw_clip_step_ema", *args, ptr(ema), decay, after, int(warmup), stream_ptr())


def loss_scale_update(ls_state, gnorm_sq, *, growth=2.0, backoff=0.5, interval=2000, scale_min=1.0, scale_max=65536.0):
    call("omlm_loss_scale_update", ptr(ls_state), ptr(gnorm_sq), float(growth), float(backoff), int(interval), float(scale_min),
         float(scale_max), stream_ptr())


def cast_pad(src, dst, R, C_, ld_src, ld_dst):
    call("omlm_cast_pad", ptr(src), ptr(dst), R, C_, ld_src, ld_dst, dcode(dst.dtype), stream_ptr())


def colsum_accumulate(part, out, P, C_, ldp):
    call("omlm_colsum_accumulate", ptr(part), ptr(out), P, C_, ldp, stream_ptr())


def relpos_first_fwd(w0, b0, pre, z, n, Hd, x0=0):
    """Rows are the distances x0 .. x0 + n - 1."""
    call("omlm_relpos_first_fwd", ptr(w0), ptr(b0), ptr(pre), ptr(z), n, Hd, int(x0), stream_ptr())


def relpos_first_bwd(ds, dw0, n, Hd, x0=0):
    call("omlm_relpos_first_bwd", ptr(ds), ptr(dw0), n, Hd, int(x0), stream_ptr())


def bias_silu_fwd(a, b, pre, z, R, C_):
    call("omlm_bias_silu_fwd", ptr(a), ptr(b), ptr(pre), ptr(z), R, C_, stream_ptr())


def silu_bwd(dz, pre, ds, total):
    call("omlm_silu_bwd", ptr(dz), ptr(pre), ptr(ds), total, stream_ptr())


def bias_add(a, b, out, R, C_, ld):
    call("omlm_bias_add", ptr(a), ptr(b), ptr(out), R, C_, ld, stream_ptr())


def relpos_mlp_fwd(w0, b0, W1, b1, W2, b2, W3, b3, saves, table, n, Hd, H, ldb, x0=0):
    """The whole rel-pos MLP as one launch (omlm_relpos_mlp_fwd).  saves: None or [pre0, z0, pre1, z1, pre2, z2] ([n, Hd] fp32 each).
    x0: the distance of row 0 (negative for a non-causal prefix)."""
    sv = saves if saves is not None else [None] * 6
    call("omlm_relpos_mlp_fwd", ptr(w0), ptr(b0), ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(W3), ptr(b3), *[ptr(t) for t in sv], ptr(table),
         int(n), int(Hd), int(H), int(ldb), int(x0), stream_ptr())


def relpos_mlp_bwd(dtable, W1, W2, W3, saves, scratch, grads, n, Hd, H, ldb, x0=0):
    """Backward of the fused MLP: saves = [pre0, z0, pre1, z1, pre2, z2]; grads = [gw0, gb0, gW1, gb1, gW2, gb2, gW3, gb3] (accumulated into)."""
    call("omlm_relpos_mlp_bwd", ptr(dtable), ptr(W1), ptr(W2), ptr(W3), *[ptr(t) for t in saves], ptr(scratch), *[ptr(g) for g in grads],
         int(n), int(Hd), int(H), int(ldb), int(x0), stream_ptr())


def rvq_encode(x, codebooks_T, indices, residual_out, n, D, C_, nstage, idx_stride=None):
    """Residual-VQ chain in the library's distance form (-cdist, first maximum; csrc/optim_misc.hip FORM_CDIST).
    indices: int32 [n, nstage] (or, with nstage == 1, any int32 view whose rows are idx_stride elements apart)."""
    call("omlm_rvq_encode", ptr(x), ptr(codebooks_T), ptr(indices), ptr(residual_out), n, D, C_, nstage, int(idx_stride or 0), stream_ptr())


def nearest_centroid(x, centroids_T, indices, n, D, C_):
    """k-means assign (sklearn MiniBatchKMeans.predict, hf_hubert_kmeans.py:87): squared-difference form; indices int32 [n]."""
    hip.require_gpu(x, "x")                 # a CPU tensor's address would reach the kernel
    call("omlm_nearest_centroid", ptr(x), ptr(centroids_T), ptr(indices), n, D, C_, stream_ptr())


def vq_accumulate(x, indices, idx_stride, counts, sums, n, D, K):
    call("omlm_vq_accumulate", ptr(x), ptr(indices), int(idx_stride), ptr(counts), ptr(sums), n, D, K, stream_ptr())


def vq_kmeans_update(means, means_T, counts, sums, K, D):
    call("omlm_vq_kmeans_update", ptr(means), ptr(means_T), ptr(counts), ptr(sums), K, D, stream_ptr())


def vq_ema_update(cluster_size, embed_avg, embed, embed_T, counts, sums, total_scratch, K, D, decay, eps):
    call("omlm_vq_ema_update", ptr(cluster_size), ptr(embed_avg), ptr(embed), ptr(embed_T), ptr(counts), ptr(sums),
         ptr(total_scratch), K, D, float(decay), float(eps), stream_ptr())


def kmeans_pp_workspace_bytes(m, trials):
    nbytes = int(hip.lib().omlm_kmeans_pp_workspace_bytes(int(m), int(trials)))
    if nbytes < 0:
        raise RuntimeError(f"omlm_kmeans_pp_workspace_bytes: bad sizes m={m}, trials={trials}")
    return nbytes


def _kmeans_pp(name, rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, K, trials):
    m, D = rows.shape
    for t, what in ((rows, "rows"), (closest, "closest"), (uniforms, "uniforms"), (pick_counter, "pick_counter"), (centres, "centres"),
                    (centres_T, "centres_T"), (chosen, "chosen"), (pots, "pots"), (workspace, "workspace")):
        hip.require_gpu(t, what)
    assert rows.dtype == closest.dtype == uniforms.dtype == centres.dtype == centres_T.dtype == torch.float32
    assert pick_counter.dtype == chosen.dtype == torch.int32 and pots.dtype == torch.float64
    assert rows.is_contiguous() and closest.numel() >= m and uniforms.numel() >= K * trials and centres.numel() >= K * D
    assert centres_T.numel() >= K * D and chosen.numel() >= K and pots.numel() >= K
    call(name, ptr(rows), ptr(closest), ptr(uniforms), ptr(pick_counter), ptr(centres), ptr(centres_T), ptr(chosen), ptr(pots),
         ptr(workspace), workspace.numel() * workspace.element_size(), int(m), int(D), int(K), int(trials), stream_ptr())


def kmeans_pp_pick(rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, K, trials):
    """One greedy k-means++ pick (number `pick_counter[0]` on the device, advanced by the call); include/omlm.h states the rule."""
    _kmeans_pp("omlm_kmeans_pp_pick", rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, K, trials)


def kmeans_pp_seed(rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, K, trials):
    """A whole seeding: K picks queued from one call, nothing returns to the host."""
    _kmeans_pp("omlm_kmeans_pp_seed", rows, closest, uniforms, pick_counter, centres, centres_T, chosen, pots, workspace, K, trials)


def kmeans_minibatch_step(x, idx, centres, centres_T, counts, bcounts, sums, rowmin, move_partial, state, alpha, tol_abs,
                          max_no_improvement):
    """One MiniBatchKMeans step on rows x[idx] (idx int32 [B]); state: 8 fp64 on the device (include/omlm.h)."""
    n, D = x.shape
    K = centres.shape[0]
    B = idx.numel()
    for t, what in ((x, "x"), (idx, "idx"), (centres, "centres"), (state, "state")):
        hip.require_gpu(t, what)
    assert x.dtype == torch.float32 and x.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous()
    assert state.dtype == move_partial.dtype == torch.float64 and state.numel() >= 8 and move_partial.numel() >= K
    assert counts.numel() >= K and bcounts.numel() >= K and sums.numel() >= K * D and rowmin.numel() >= B
    call("omlm_kmeans_minibatch_step", ptr(x), ptr(idx), ptr(centres), ptr(centres_T), ptr(counts), ptr(bcounts), ptr(sums), ptr(rowmin),
         ptr(move_partial), ptr(state), int(n), int(B), int(D), int(K), float(alpha), float(tol_abs), int(max_no_improvement),
         stream_ptr())


def kmeans_inertia(x, centres_T, out, labels=None):
    """out[0] (fp64, device) += sum over the rows of x of the min squared distance; labels int32 [n] optional."""
    n, D = x.shape
    K = centres_T.shape[1]
    hip.require_gpu(x, "x")
    hip.require_gpu(centres_T, "centres_T")
    assert x.dtype == torch.float32 and x.is_contiguous() and centres_T.is_contiguous() and out.dtype == torch.float64
    assert labels is None or (labels.dtype == torch.int32 and labels.numel() >= n)
    call("omlm_kmeans_inertia", ptr(x), ptr(centres_T), ptr(out), ptr(labels), int(n), int(D), int(K), stream_ptr())


SAMPLER_MAX_V = 65536             # csrc/sampler.hip: widest row the sampler takes (V = codebook_size + 1); the uint16 token stores end there too


def check_sampler_width(V):
    """ValueError before any launch when a row of V logits (a predicted codebook of V - 1 entries) is past the sampler's limit."""
    if V > SAMPLER_MAX_V:
        raise ValueError(f"sampler: a predicted codebook of {V - 1} entries needs rows of V = {V} logits, past the limit of "
                         f"{SAMPLER_MAX_V} (codebooks of up to {SAMPLER_MAX_V - 1} entries sample)")


def sample_topk_gumbel(logits, uniform, out, V, k, temperature, forbid_last):
    check_sampler_width(V)
    B, ld = logits.shape
    call("omlm_sample_topk_gumbel", ptr(logits), ptr(uniform), ptr(out), B, V, ld, int(k), float(temperature),
         int(forbid_last), stream_ptr())


def split_seed(seed):
    """(seed_lo, seed_hi): the uint32 halves of a 64-bit sampler seed (any Python int; taken modulo 2^64)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def sample_topk_gumbel_rng(logits, seed, step, row0, out, V, k, temperature, forbid_last):
    """sample_topk_gumbel on the counter stream of include/omlm.h: row b draws u(step, row0 + b, c) from `seed`; no uniform buffer."""
    check_sampler_width(V)
    B, ld = logits.shape
    lo, hi = split_seed(seed)
    call("omlm_sample_topk_gumbel_rng", ptr(logits), lo, hi, int(step), int(row0), ptr(out), B, V, ld, int(k), float(temperature),
         int(forbid_last), stream_ptr())


class SampleArgs(C.Structure):
    """Mirror of ``omlm_sample_args`` (include/omlm.h)."""
    _fields_ = [("logits", C.c_void_p), ("B", C.c_int), ("V", C.c_int), ("ld", C.c_int),
                ("uniform", C.c_void_p), ("seed_lo", C.c_uint), ("seed_hi", C.c_uint), ("step", C.c_int), ("row0", C.c_int),
                ("step_dev", C.c_void_p), ("out", C.c_void_p), ("hist", C.c_void_p),
                ("k", C.c_int), ("temperature", C.c_float), ("top_p", C.c_float), ("forbid_last", C.c_int),
                ("emb_table", C.c_void_p), ("emb_row_offset", C.c_longlong), ("emb_rows", C.c_longlong), ("x", C.c_void_p), ("D", C.c_int)]


def check_top_p(top_p, name="top_p"):
    """The nucleus mass as the kernels take it: None -> 1.0 (no nucleus), a number in (0, 1] -> float; anything else (<= 0, > 1, NaN,
    not a number) raises a ValueError that names the argument.  Pure Python: runs before any device work."""
    if top_p is None:
        return 1.0
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or a number in (0, 1], not {top_p!r}") from None
    if not (0.0 < p <= 1.0):
        raise ValueError(f"{name} must be None or a number in (0, 1], not {top_p!r}")
    return p


class SampleRowParams(C.Structure):
    """Mirror of ``omlm_sample_row_params`` (include/omlm.h): [B] device arrays, each or None."""
    _fields_ = [("k", C.c_void_p), ("temperature", C.c_void_p), ("top_p", C.c_void_p), ("seed", C.c_void_p), ("sample", C.c_void_p)]


# member of omlm_sample_row_params -> element type of its [B] array (a seed is 64 bits: uint64 held as int64)
_ROW_DTYPES = {"k": torch.int32, "temperature": torch.float32, "top_p": torch.float32, "seed": torch.int64, "sample": torch.int32}


def sample_row_params(B, **rows):
    """SampleRowParams over the given [B] tensors (``k`` int32, ``temperature`` / ``top_p`` fp32, ``seed`` int64 holding the uint64,
    ``sample`` int32; each contiguous on the device, or None), or None when none is given.  A wrong tensor raises a ValueError that
    names it.  The VALUES are the caller's to check (the per_row_* functions below): the library sees pointers."""
    if all(t is None for t in rows.values()):
        return None
    for name, t in rows.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != _ROW_DTYPES[name] or t.shape != (B,) or not t.is_contiguous():
            got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else repr(t)
            raise ValueError(f"sample: row_{name} must be a contiguous {_ROW_DTYPES[name]} tensor [{B}]; got {got}")
        hip.require_gpu(t, f"row_{name}")
    return SampleRowParams(*(ptr(rows[n]) for n, _ in SampleRowParams._fields_))


def sample(logits, out, V, k, temperature, forbid_last, *, top_p=None, uniform=None, seed=None, step=0, row0=0, step_dev=None,
           hist=None, emb_table=None, emb_row_offset=0, x=None, lp_model=None, lp_sampled=None,
           row_k=None, row_temperature=None, row_top_p=None, row_seed=None, row_sample=None):
    """omlm_sample: the sampler with an optional nucleus, one call over every form.  ``uniform`` ([B, V], or [steps, B, V] with
    ``step_dev``) or ``seed`` (the counter stream: row b draws u(step or *step_dev, row0 + b, c)) -- exactly one of the two;
    ``step_dev`` (int32 [1], device) selects the graph-replayable form, where ``hist`` is [steps, B]; ``emb_table`` [rows, D] with ``x``
    [B, D] adds the embedding gather.  top_p None or 1: the launch of sample_topk_gumbel*.
    ``lp_model`` / ``lp_sampled`` (fp32 [B], or [steps, B] with ``step_dev``; either or both): the log-probabilities of the sampled id
    (include/omlm.h), written by the same launch -- the call is then omlm_sample_lp; the ids are those of the call without them.
    ``row_k`` / ``row_temperature`` / ``row_top_p`` / ``row_seed`` / ``row_sample`` ([B] device tensors: int32 / fp32 / fp32 / the uint64
    seeds as int64 / int32; any subset): per-row values in place of ``k`` / ``temperature`` / ``top_p`` / ``seed`` / ``row0 + b`` -- the
    call is then omlm_sample_rows, and a scalar whose tensor is given is not read (pass None).  ``row_seed`` and ``row_sample`` belong
    to the counter stream: ``row_seed`` stands for ``seed``, and either of them with ``uniform`` is refused.  Which of the three entries
    the call takes: sampler_call."""
    check_sampler_width(V)
    B, ld = logits.shape
    rows = sample_row_params(B, k=row_k, temperature=row_temperature, top_p=row_top_p, seed=row_seed, sample=row_sample)
    p = 1.0 if row_top_p is not None else check_top_p(top_p)
    if uniform is not None and (row_seed is not None or row_sample is not None):
        raise ValueError("sample: row_seed / row_sample belong to the counter stream and cannot be combined with uniform=")
    if (uniform is None) == (seed is None and row_seed is None):
        raise ValueError("sample: give either uniform= or seed=, not both and not neither")
    lo, hi = split_seed(seed) if seed is not None else (0, 0)
    a = SampleArgs(ptr(logits), B, int(V), ld, ptr(uniform), lo, hi, int(step), int(row0), ptr(step_dev), ptr(out), ptr(hist),
                   1 if row_k is not None else int(k), 1.0 if row_temperature is not None else float(temperature), p, int(forbid_last),
                   ptr(emb_table), int(emb_row_offset), 0 if emb_table is None else emb_table.shape[0], ptr(x),
                   0 if emb_table is None else emb_table.shape[1])
    for t, name in ((lp_model, "lp_model"), (lp_sampled, "lp_sampled")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape[-1] != B):
            raise ValueError(f"sample: {name} must be a contiguous fp32 tensor [B] ([steps, B] with step_dev), B = {B}; got "
                             f"{t.dtype} {tuple(t.shape)}")
    name, args = sampler_call(a, rows, lp_model, lp_sampled)
    call(name, *args, stream_ptr())


def sampler_call(args: SampleArgs, rows: Optional[SampleRowParams], lp_model=None, lp_sampled=None):
    """The sampler entry for a filled block, as (name, arguments in front of the stream): omlm_sample_rows with a row block,
    omlm_sample_lp with a log-probability tensor and no row block, omlm_sample with neither.  The caller keeps `args`, `rows` and the
    tensors alive for as long as it uses the result.  Nothing is checked or launched here."""
    if rows is not None:
        return "omlm_sample_rows", (C.addressof(args), C.addressof(rows), ptr(lp_model), ptr(lp_sampled))
    if lp_model is not None or lp_sampled is not None:
        return "omlm_sample_lp", (C.addressof(args), ptr(lp_model), ptr(lp_sampled))
    return "omlm_sample", (C.addressof(args),)


# ---- per-row sampling arguments: one pure-Python normaliser per argument of generate() / SamplingLoop -----------------------------
# A plain number (or None) comes back as the scalar the call has always used; a list, tuple or 1-D tensor / array of length `batch`
# comes back as a LIST of checked numbers, one per row.  Everything runs before any device work; a ValueError names the argument and,
# for a bad entry, its index.

def _row_sequence(x, batch, name):
    """None for a scalar; the entries of a per-row sequence as a list of Python objects (length checked against `batch`)."""
    if isinstance(x, (torch.Tensor,)) or type(x).__module__ == "numpy":
        if getattr(x, "ndim", 0) == 0:
            return None
        if x.ndim != 1:
            raise ValueError(f"{name}: a per-row value is a number or a 1-D sequence of length {batch}, not an array of shape {tuple(x.shape)}")
        x = x.tolist()
    if not isinstance(x, (list, tuple)):
        return None
    if len(x) != int(batch):
        raise ValueError(f"{name}: a per-row sequence holds one value per row: its length is {len(x)}, the batch is {int(batch)}")
    return list(x)


def per_row_checked(x, batch, name, scalar, entry, what):
    """The normaliser behind every per_row_* function: `scalar(x)` for a number; for a sequence of length `batch` the list of
    `entry(v)`, where `entry` returns None for a value it refuses (`what` says what it accepts)."""
    seq = _row_sequence(x, batch, name)
    if seq is None:
        return scalar(x)
    out = []
    for i, v in enumerate(seq):
        r = None if v is None else entry(v)
        if r is None:
            raise ValueError(f"{name}[{i}] must be {what}, not {v!r}")
        out.append(r)
    return out


def _as_fp32(v):
    return C.c_float(v).value


def per_row_temperature(temperature, batch, name="temperature"):
    """A number: returned as it is (the sampler refuses what is not > 0).  A sequence: a list of floats, each finite and > 0 as fp32."""
    def entry(v):
        f = _check_number(v)
        return f if 0.0 < f <= FP32_MAX and _as_fp32(f) > 0.0 else None
    return per_row_checked(temperature, batch, name, lambda s: s, entry, "a finite number > 0")


def per_row_filter_thres(filter_thres, batch, name="filter_thres"):
    """A number: returned as it is.  A sequence: a list of floats, each in [0, 1] (row r keeps k_r = max(int((1 - thres_r) * V), 1))."""
    def entry(v):
        f = _check_number(v)
        return f if 0.0 <= f <= 1.0 else None
    return per_row_checked(filter_thres, batch, name, lambda s: s, entry, "a number in [0, 1]")


def per_row_top_p(top_p, batch, name="top_p"):
    """A number or None: check_top_p's float (1.0: no nucleus).  A sequence: a list of floats, each in (0, 1] (1: no nucleus for the row)."""
    def entry(v):
        f = _check_number(v)
        return f if 0.0 < f <= 1.0 and _as_fp32(f) > 0.0 else None
    return per_row_checked(top_p, batch, name, lambda s: check_top_p(s, name), entry, "a number in (0, 1]")


def per_row_cond_scale(cond_scale, batch, name="cond_scale"):
    """A number or None: check_cond_scale's value (None: off).  A sequence: a list of floats, each finite and >= 0 -- guidance is then on
    for every row, the rows of scale 1 included."""
    def entry(v):
        f = _check_number(v)
        return f if 0.0 <= f <= FP32_MAX else None
    return per_row_checked(cond_scale, batch, name, lambda s: check_cond_scale(s, name), entry, "a finite number >= 0 (as fp32)")


def per_row_seed(seed, batch, name="sampler_seed"):
    """A number or None: returned as it is.  A sequence: a list of ints in [0, 2^64) (any Python int, taken modulo 2^64)."""
    def entry(v):
        if isinstance(v, bool) or not isinstance(v, int):
            return None
        return v & 0xFFFFFFFFFFFFFFFF
    return per_row_checked(seed, batch, name, lambda s: s, entry, "an integer (taken modulo 2^64)")


def topk_count(filter_thres, V1):
    """k of a row of V1 logits: max(int((1 - thres) * V1), 1); a list for a list."""
    if isinstance(filter_thres, list):
        return [max(int((1 - t) * V1), 1) for t in filter_thres]
    return max(int((1 - filter_thres) * V1), 1)


def row_tensor(values, member, device):
    """The [B] device tensor of a list of checked per-row values, in the element type of `member` of omlm_sample_row_params (a seed's
    uint64 as the int64 of the same bits) or, for "scale", of omlm_guide_logits_rows' scale (fp32); None for None."""
    if values is None:
        return None
    if member == "seed":
        values = [v - (1 << 64) if v >= (1 << 63) else v for v in values]
    return torch.tensor(values, dtype=torch.float32 if member == "scale" else _ROW_DTYPES[member]).to(device)


class SamplerUpload(NamedTuple):
    """SamplerSettings.upload: what the launches of `rows` prompts take.  ``tensors``: member of omlm_sample_row_params -> its [rows]
    device tensor or None; ``k`` / ``temperature`` / ``top_p``: the scalars of omlm_sample_args, a valid placeholder (1, 1.0, 1.0; not
    read) where a tensor stands in; ``seed``: the one seed, None with a seed per row (or none at all); ``guidance``: the scale as a number,
    a [rows] fp32 tensor, or None."""
    rows: int
    tensors: dict
    k: object
    temperature: object
    top_p: object
    seed: object
    guidance: object

    def block(self) -> Optional[SampleRowParams]:
        """The row block over ``tensors`` (sample_row_params: None when there is none)."""
        return sample_row_params(self.rows, **self.tensors)


class SamplerSettings(NamedTuple):
    """The checked sampling arguments of a call over `rows` prompts, host side: each of ``k`` (the top-k counts), ``temperature``,
    ``top_p`` (1.0: no nucleus), ``guidance`` (None: off) and ``seed`` is a number or a list of `rows` numbers, as the per_row_*
    functions return them."""
    rows: int
    k: object
    temperature: object
    top_p: object
    guidance: object
    seed: object
    logprobs: bool = False

    @classmethod
    def checked(cls, rows, V1, *, temperature, filter_thres, top_p, cond_scale, sampler_seed, logprobs=False, after_guidance=None):
        """From generate()'s raw arguments, for rows of V1 logits, in the order generate() has always checked them: the first thing wrong
        raises its ValueError, which names the argument.  ``after_guidance(guidance)`` runs between the guidance check and the rest (what
        the caller must refuse once it knows whether guidance is on).  Pure Python: before any device work."""
        guidance = per_row_cond_scale(cond_scale, rows)
        if after_guidance is not None:
            after_guidance(guidance)
        top_p = per_row_top_p(top_p, rows)
        temperature = per_row_temperature(temperature, rows)
        filter_thres = per_row_filter_thres(filter_thres, rows)
        seed = per_row_seed(sampler_seed, rows)
        return cls(rows, topk_count(filter_thres, V1), temperature, top_p, guidance, seed, bool(logprobs))

    def cut(self, b0: int, b1: int) -> "SamplerSettings":
        """The settings of rows [b0, b1): lists sliced, numbers kept."""
        return self._replace(rows=b1 - b0, **{f: v[b0:b1] for f, v in self._asdict().items() if isinstance(v, list)})

    def upload(self, device) -> SamplerUpload:
        """The per-row lists as [rows] device tensors (row_tensor), uploaded once.  With a seed per row every row draws with stream sample
        index 0 -- u(t, 0, c) of its own seed -- so ``sample`` is a zero array and the call's first global index is not read."""
        per_row = {m: v if isinstance(v, list) else None
                   for m, v in (("k", self.k), ("temperature", self.temperature), ("top_p", self.top_p), ("seed", self.seed))}
        tensors = {m: row_tensor(v, m, device) for m, v in per_row.items()}
        tensors["sample"] = None if tensors["seed"] is None else torch.zeros(self.rows, device=device, dtype=torch.int32)
        scalar = lambda m, placeholder: getattr(self, m) if tensors[m] is None else placeholder  # noqa: E731
        return SamplerUpload(self.rows, tensors, scalar("k", 1), scalar("temperature", 1.0), scalar("top_p", 1.0), scalar("seed", None),
                             row_tensor(self.guidance, "scale", device) if isinstance(self.guidance, list) else self.guidance)


def probe_tr16(out):
    call("omlm_probe_tr16", ptr(out), stream_ptr())
