"""KV-cached autoregressive decoding for TokenConditionedTransformer (host side of csrc/decode.hip).

The reference's ``generate`` (open_musiclm.py:253-326) re-runs the whole causal forward for every sampled id.  Because
every op of the trunk is causal, the same logits come out of computing one new row per step against a key/value cache
and the two-row state of the causal depthwise convolution -- that is what :class:`CachedDecoder` does:

    dec = CachedDecoder(model, batch, max_rows)
    logits = dec.prefill(cond_ids + [sampled_so_far])      # batched forward over the prompt rows, fills the caches
    logits = dec.step(new_ids, k)                           # one row: ids sampled from `logits`, k = index of that id

``step`` is one call into libomlm_hip.so (32 kernel launches: embedding gather, 5 per layer, logit head) plus the
counter advance; the row index lives on the device so that a step can be captured into a HIP graph.

A call holds ``max_batch`` samples (8, or 16 on the matrix-core step kernels); ``CachedDecoder(..., wide=True)`` holds up to
``max_call_batch`` (64 there): groups of 16 samples ride through one launch of every step kernel, each computed as a 16-sample call.

The K/V cache is fp32 by default.  ``CachedDecoder(..., kv_cache="operand")`` keeps it in the precision's 16-bit operand type: the step kernels
round every key and value to that type before they store them, so the 16-bit cache holds the same numbers in half the bytes (``cache_bytes``)
and the logits are the same bit for bit.

Classifier-free guidance on the condition (token sequence 0; include/omlm.h): a guided call of P prompts is a decoder of 2P rows, the
prompts followed by their null twins, and ``SamplingLoop(..., guidance=s)`` samples P ids per step from ``null + s (cond - null)`` --
one combine launch in front of the sampler, one twin copy behind it, the step kernels untouched.

Key mask (``CachedDecoder(..., key_mask=True)``; include/omlm.h: omlm_decode_step_masked): the decoder owns ``key_live`` [B, Nmax] bytes,
all ones; ``prefill(ids, key_mask=m)`` runs the batched forward under m and copies it into the first columns, and every step then goes
through the masked attention kernels, so a new row attends to the keys m allows and to every row after the prompt.  Off (the default):
``key_live`` is None and every call is omlm_decode_step, as it has always been.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Optional, Sequence

import torch

from . import engine, hip, ops
from .hip import call, ptr, stream_ptr

MAX_DECODE_BATCH = 8

# generate(): the most bytes of uniforms [n_new, B, V1] drawn up front before the default moves to the counter stream
UNIFORM_BUFFER_MAX_BYTES = 1 << 30


def sampler_rng_choice(requested, n_new: int, batch: int, V1: int, injected: bool) -> str:
    """Where generate() takes its uniforms from: "buffer" (all draws of the call up front, [n_new, batch, V1] floats -- the only way to
    inject draws) or "counter" (the stream of include/omlm.h, formed in the sampler's registers).  requested None: "buffer", unless no
    draws are injected and the buffer would exceed UNIFORM_BUFFER_MAX_BYTES.  Injected draws with "counter", or any other string, raise
    a ValueError."""
    if requested not in (None, "buffer", "counter"):
        raise ValueError(f"sampler_rng must be None, 'buffer' or 'counter', not {requested!r}")
    if requested == "counter" and injected:
        raise ValueError("sampler_rng='counter' draws its uniforms in the kernel: it cannot be combined with injected draws "
                         "(uniforms= or UNIFORM_SOURCE)")
    if requested is not None:
        return requested
    if injected or 4 * int(n_new) * int(batch) * int(V1) <= UNIFORM_BUFFER_MAX_BYTES:
        return "buffer"
    return "counter"


KV_CACHE_CHOICES = (None, "fp32", "operand")


def check_kv_cache(requested):
    """`requested` if it is one of KV_CACHE_CHOICES; a ValueError that names them otherwise."""
    if not any(requested is c or (isinstance(requested, str) and requested == c) for c in KV_CACHE_CHOICES):
        raise ValueError(f"kv_cache must be None, 'fp32' or 'operand', not {requested!r}")
    return requested


def kv_cache_choice(requested, precision: str) -> torch.dtype:
    """Element type of the decode K/V cache.  None or "fp32": torch.float32.  "operand": the attention operand dtype of `precision` -- bf16
    for "bf16", fp16 for "fp16" / "fp16ff", and fp32 for "bf16x3" (its operands are fp32, so the cache stays what it is).  Anything else
    raises a ValueError that names the accepted values."""
    if precision not in engine._PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; one of {sorted(engine._PRECISIONS)}")
    return engine._PRECISIONS[precision] if check_kv_cache(requested) == "operand" else torch.float32


def cache_bytes(model, batch: int, rows: int, precision: str, kv_cache=None) -> int:
    """Bytes of the K + V caches of all layers for `batch` samples of `rows` rows: batch * rows * 64 * 2 * depth * element size (one K/V head
    of 64 dims per layer).  kv_cache="operand" halves it on the 16-bit precisions."""
    esize = torch.empty(0, dtype=kv_cache_choice(kv_cache, precision)).element_size()
    return int(batch) * int(rows) * engine.DIM_HEAD * 2 * len(model.transformer.layers) * esize


_PTRS = ["Wq", "Wkv", "Wo", "W1p", "W2p", "attn_gamma", "q_scale", "k_scale", "ffin_gamma", "convw", "mid_gamma",
         "Kc", "Vc", "hist"]


class DecodeArgs(C.Structure):
    """Mirror of ``omlm_decode_args`` (include/omlm.h)."""
    _fields_ = ([(n, C.c_int) for n in ("B", "D", "H", "L", "F", "Fp", "Nmax", "w_dtype", "round_bf16", "nsplit")] +
                [("eps", C.c_float), ("scale", C.c_float), ("pos_dev", C.c_void_p)] +
                [(n, C.POINTER(C.c_void_p)) for n in _PTRS] +
                [("bias_table", C.c_void_p), ("bias_ld", C.c_int),
                 ("final_gamma", C.c_void_p), ("head_W", C.c_void_p), ("V1", C.c_int), ("ldV", C.c_int),
                 ("emb_table", C.c_void_p), ("emb_row_offset", C.c_longlong), ("emb_rows", C.c_longlong)] +
                [(n, C.c_void_p) for n in ("x", "x1", "q", "parts", "u", "logits", "advance_pos", "advance_step", "ln_parts")] +
                [("W1p_lo", C.POINTER(C.c_void_p)), ("W2p_lo", C.POINTER(C.c_void_p)), ("head_W_lo", C.c_void_p)] +
                [("splitk_ws", C.c_void_p), ("splitk_cnt", C.c_void_p)] +
                [("kv16", C.c_int), ("k_new", C.c_void_p)])


MAX_DECODE_HEADS = 16              # omlm_decode_step: H <= 16
DEC4_NB = 16                       # decode_plan.h: samples of a group of the matrix-core step kernels (one MFMA column tile)
DEC4_GMAX = 4                      # decode_plan.h: groups of DEC4_NB samples one call carries through every launch


def _geometry(model):
    tr = model.transformer
    inner = getattr(tr.layers[0][2], "inner_dim", 0) if len(tr.layers) else 0
    return tr.dim, tr.heads, engine.ceil_to(inner, 64)


def step_route(B: int, D: int, H: int, Fp: int, w16: bool, wide: bool = False) -> Optional[str]:
    """The one mirror of csrc/decode_plan.h (tests/test_decode_plan_host.py pins it to the plan over a grid): the route omlm_decode_step takes
    for B samples with every scratch pointer given, as CachedDecoder gives them -- "gen1" (first-generation kernels), or at dim 1024 "dec3"
    (row kernels, B = 1), "dec4" (matrix cores: 16-bit weights, B >= 2, Fp <= 3072 a multiple of 32) or "dec2" (vector kernels); None where
    no call holds B samples: more than 16 on the matrix cores (wide: 64), more than 8 elsewhere, or B * Fp floats past the 150 KiB the
    kernels of at most 8 samples stage in LDS.  (The heads limit is MAX_DECODE_HEADS, see supports.)"""
    gen2 = D == 1024 and H * 64 <= 1024 and Fp <= 4096 and Fp % 2 == 0 and (H * 64 + 128) % 4 == 0
    mc = bool(w16) and gen2 and B >= 2 and 0 < Fp <= 3072 and Fp % 32 == 0
    limit = (DEC4_GMAX * DEC4_NB if wide else DEC4_NB) if mc else min(MAX_DECODE_BATCH, (150 * 1024 - 1024) // (4 * max(Fp, 1)))
    if not 1 <= B <= limit:
        return None
    return "gen1" if not gen2 else "dec3" if B == 1 else "dec4" if mc else "dec2"


def _second_generation(D: int, H: int, Fp: int) -> bool:
    """The dec2 / dec3 / dec4 step kernels (dim 1024) rather than the first-generation ones: what step_route says of a one-sample call."""
    return step_route(1, D, H, Fp, True) == "dec3"


def _matrix_core(B: int, D: int, H: int, Fp: int) -> bool:
    """The matrix-core step kernels serve B samples (16-bit weights, every scratch pointer given): step_route's "dec4"."""
    return step_route(B, D, H, Fp, True, wide=True) == "dec4"


@functools.lru_cache(maxsize=None)
def step_max_batch(D: int, H: int, Fp: int, w16: bool, wide: bool = False) -> int:
    """The most samples step_route serves."""
    return max((B for B in range(1, DEC4_GMAX * DEC4_NB + 1) if step_route(B, D, H, Fp, w16, wide)), default=0)


def step_lo_planes_ok(B: int, D: int, H: int, Fp: int) -> bool:
    """Whether omlm_decode_step takes the lo planes of FF-in / FF-out / head for B samples (16-bit weights): everywhere on the first
    generation; at dim 1024 on the row kernels with Fp <= 3072 and on the matrix cores."""
    route = step_route(B, D, H, Fp, True, wide=True)
    if route is None:                                          # no call holds B samples: only the first generation's answer ignores the batch
        return step_route(1, D, H, Fp, True) == "gen1"
    return route in ("gen1", "dec4") or (route == "dec3" and Fp <= 3072)


def lo_planes_ok(model, batch: int) -> bool:
    """"fp16ff": whether omlm_decode_step takes the lo planes of FF-in / FF-out / head at this geometry (step_lo_planes_ok), and the batched
    forward keeps h1's lo plane for the prefill (Fp <= 4096).  Elsewhere the steps run on the fp16 kernels with the hi planes, as "fp16" does."""
    return engine.ff_planes_ok(_geometry(model)[2]) and step_lo_planes_ok(batch, *_geometry(model))


def max_batch(model, precision: str) -> int:
    """Samples one decode call holds: 16 where the matrix-core kernels serve the model (16-bit weights, dim 1024, at most 16 heads,
    feed-forward width <= 3072); otherwise 8, or fewer where B * Fp floats exceed the first-generation kernels' LDS."""
    return step_max_batch(*_geometry(model), precision in ("bf16", "fp16", "fp16ff"))


def max_call_batch(model, precision: str) -> int:
    """Samples one WIDE decode call holds (CachedDecoder(..., wide=True)): 64 -- four groups of 16 carried through one launch of every step
    kernel -- where max_batch is 16 (the matrix-core kernels serve the model); max_batch everywhere else."""
    return step_max_batch(*_geometry(model), precision in ("bf16", "fp16", "fp16ff"), wide=True)


def scratch_sizes(batch: int, D: int, Fp: int) -> dict:
    """Elements of the step's scratch for a call of `batch` samples (include/omlm.h: OMLM_DECODE_LN_PARTS_B floats, OMLM_DECODE_SPLITK_FLOATS_B
    floats, OMLM_DECODE_SPLITK_CNT_B ints): per group of 16 samples the sizes a 16-sample call has always had."""
    G = (batch + DEC4_NB - 1) // DEC4_NB
    tiles = (D + 15) // 16
    return {"ln_parts": 3 * G * max(tiles, (Fp + 7) // 8) * 32,           # [family][group][partial][16 samples][2]
            "splitk_ws": G * 4 * tiles * 256,                             # [group][tile][slice][16 rows][16 samples]
            "splitk_cnt": max(G * tiles, batch, DEC4_NB)}                 # FF-out: per (group, tile); attention combine: per sample


def supports(model, batch: int, precision: Optional[str] = None, prompt_rows: Optional[int] = None, wide: bool = False) -> bool:
    """Whether CachedDecoder (omlm_decode_step) serves `batch` samples of this model; where it does not, generate() re-runs the forward.
    A non-causal prefix of P rows is served only when the prompt holds all of it (prompt_rows >= P): a row i >= P sees the keys j <= i
    alone, so the cached rows never change -- a row generated inside the prefix would change the rows before it.
    wide=True (with a precision): the sample limit is max_call_batch instead of max_batch."""
    tr = model.transformer
    limit = max_batch(model, precision) if precision is not None else min(MAX_DECODE_BATCH, max_batch(model, "bf16x3"))
    if wide and precision is not None:
        limit = max_call_batch(model, precision)
    P = engine.prefix_rows(tr)
    prefix_ok = P == 0 or (prompt_rows is not None and P <= prompt_rows)
    return 1 <= batch <= limit and prefix_ok and 1 <= tr.heads <= MAX_DECODE_HEADS


class CachedDecoder:
    def __init__(self, model, batch: int, max_rows: int, precision: str, wide: bool = False, kv_cache=None, key_mask: bool = False):
        """kv_cache: None / "fp32" (fp32 K/V cache) or "operand" (the precision's 16-bit operand type; same logits, half of cache_bytes);
        self.kv_dtype tells which type the cache holds.
        key_mask: True -- the steps run under self.key_live ([B, Nmax] uint8, nonzero = attend; all ones until prefill is given a mask)
        through omlm_decode_step_masked; False -- self.key_live is None and the steps are omlm_decode_step."""
        self.kv_dtype = kv_cache_choice(kv_cache, precision)                   # refused by name before any device work
        if not isinstance(key_mask, bool):
            raise ValueError(f"key_mask must be a bool, not {key_mask!r}")
        # (a non-causal prefix is checked against the prompt in prefill)
        if not supports(model, batch, precision, prompt_rows=engine.prefix_rows(model.transformer), wide=wide):
            tr = model.transformer
            limit = max_call_batch(model, precision) if wide else max_batch(model, precision)
            raise ValueError(f"cached decode does not serve this model with {batch} samples per call (at most {limit} "
                             f"samples, at most {MAX_DECODE_HEADS} heads; got {tr.heads} heads)")
        self.model, self.B, self.Nmax, self.precision = model, batch, int(max_rows), precision
        tr = model.transformer
        dev = model.start_tokens[0].device
        hip.require_gpu(model.start_tokens[0], "model parameters")
        self.pw = engine.prepared_weights(model, precision)
        self.T = self.pw.T
        # "fp16ff": the steps read the FF-in / FF-out / head weights as hi + lo planes and keep LayerNorm outputs and h1 un-rounded, like the
        # three-product forward of the batched path (omlm_decode_args::W1p_lo) -- where the step kernels take lo planes (lo_planes_ok); elsewhere
        # they run on the fp16 kernels with the hi planes
        self.planes = bool(self.pw.ff3) and bool(self.pw.ff_planes) and lo_planes_ok(model, batch)
        L, D, H = len(tr.layers), tr.dim, tr.heads
        F, Fp = self.pw.layers[0]["F"], self.pw.layers[0]["Fp"]
        self.L, self.D, self.H, self.F, self.Fp = L, D, H, F, Fp
        B, Nmax = self.B, self.Nmax
        f32 = dict(device=dev, dtype=torch.float32)
        assert self.kv_dtype in (torch.float32, self.T), (self.kv_dtype, self.T)
        self.Kc = [torch.zeros(B, Nmax, engine.DIM_HEAD, device=dev, dtype=self.kv_dtype) for _ in range(L)]
        self.Vc = [torch.zeros(B, Nmax, engine.DIM_HEAD, device=dev, dtype=self.kv_dtype) for _ in range(L)]
        # 16-bit cache: the step's raw key waits here in fp32 until the attention kernel has normalised it (omlm_decode_args::k_new)
        self.k_new = torch.zeros(B, engine.DIM_HEAD, **f32) if self.kv_dtype != torch.float32 else None
        self.hist = [torch.zeros(B, 2, 2 * Fp, **f32) for _ in range(L)]
        self.x, self.x1 = torch.empty(B, D, **f32), torch.empty(B, D, **f32)
        self.q = torch.empty(B, H * engine.DIM_HEAD, **f32)
        self.nsplit = (Nmax + 63) // 64
        self.parts = torch.zeros(B, self.nsplit, H, 66, **f32)                 # attention partials (max, sum, o[64])
        self.pos_dev = torch.zeros(1, device=dev, dtype=torch.int32)           # row index, kept on the device
        # key mask of the masked steps: static for the decoder's life (a captured cycle holds its address); rows past the prompt stay live
        self.key_live = torch.ones(B, Nmax, device=dev, dtype=torch.uint8) if key_mask else None
        self.u = torch.empty(B, Fp, **f32)
        seq = model.token_sequences[-1]
        self.Q, self.V1 = seq.num_quantizers, seq.codebook_size + 1
        self.ldV = engine.ceil_to(self.V1, 8)
        self.logits = torch.zeros(B, self.ldV, **f32)
        self.codebook = seq.codebook_size
        self.emb = model.embeddings[-1].weight.detach()
        # learned absolute position embeddings (open_musiclm.py:134-136: row p of the LAST sequence's table is added to the embedding of
        # its p-th id): the single-row steps add the row of the id they embed
        self.pos_emb = (model.absolute_position_embeddings[-1].weight.detach()
                        if getattr(model, "use_absolute_position_embeddings", False) else None)
        # rel-pos table for every distance the cache can hold: [Nmax, ld] fp32 (row = i - j, column = head)
        self.table, _ = engine.relpos_forward(tr, Nmax, False)
        self.rows = 0                       # rows already in the caches == index of the next row
        self._keep = []                     # python references that keep the pointer arrays' targets alive
        a = DecodeArgs()
        a.B, a.D, a.H, a.L, a.F, a.Fp, a.Nmax, a.nsplit = B, D, H, L, F, Fp, Nmax, self.nsplit
        a.pos_dev = self.pos_dev.data_ptr()
        a.w_dtype = ops.dcode(self.T)                              # 0 fp32, 1 bf16, 2 fp16 (served by the library's fp16 copy)
        a.round_bf16 = 0 if self.T == torch.float32 else 1         # round activations to the 16-bit operand type like the batched path
        a.eps, a.scale = 1e-5, float(engine.ATTN_SCALE)

        def arr(tensors: Sequence[torch.Tensor]):
            ts = [t.detach() for t in tensors]
            for t in ts:
                hip.require_gpu(t, "decode operand")
                assert t.is_contiguous()
            self._keep.append(ts)
            out = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            self._keep.append(out)
            return C.cast(out, C.POINTER(C.c_void_p))
        lay = self.pw.layers
        a.Wq, a.Wkv, a.Wo = arr([w["Wq"] for w in lay]), arr([w["Wkv"] for w in lay]), arr([w["Wo"] for w in lay])
        a.W1p, a.W2p = arr([w["W1p"] for w in lay]), arr([w["W2p"] for w in lay])
        # fp32 views of the (operand-dtype) taps / gamma: same values as the batched path uses (fp16ff: hi + lo planes)
        if self.planes:
            a.convw = arr([w["convw"].float() + w["convw_lo"].float() for w in lay])
            a.mid_gamma = arr([w["gamma_mid"].float() + w["gamma_mid_lo"].float() for w in lay])
            a.W1p_lo, a.W2p_lo = arr([w["W1p_lo"] for w in lay]), arr([w["W2p_lo"] for w in lay])
        else:
            a.convw, a.mid_gamma = arr([w["convw"].float() for w in lay]), arr([w["gamma_mid"].float() for w in lay])
        a.attn_gamma = arr([attn.norm.gamma for attn, _, _ in tr.layers])
        a.q_scale = arr([attn.q_scale for attn, _, _ in tr.layers])
        a.k_scale = arr([attn.k_scale for attn, _, _ in tr.layers])
        a.ffin_gamma = arr([ff.norm_in.gamma for _, _, ff in tr.layers])
        a.Kc, a.Vc, a.hist = arr(self.Kc), arr(self.Vc), arr(self.hist)
        a.bias_table = self.table.data_ptr() if self.table is not None else None
        a.bias_ld = self.table.shape[-1] if self.table is not None else 0
        a.final_gamma = tr.norm.gamma.detach().data_ptr()
        a.V1, a.ldV = self.V1, self.ldV
        a.emb_table, a.emb_rows = self.emb.data_ptr(), self.emb.shape[0]
        for n in ("x", "x1", "q", "parts", "u", "logits"):
            setattr(a, n, getattr(self, n).data_ptr())
        # per-workgroup LayerNorm partial sums of the batched step kernels (OMLM_DECODE_LN_PARTS(D, Fp) floats x 3 producers x groups)
        sizes = scratch_sizes(B, a.D, a.Fp)
        self.ln_parts = torch.zeros(sizes["ln_parts"], device=self.x.device)      # [partial][16 samples][2] per group
        a.ln_parts = self.ln_parts.data_ptr()
        # split-K scratch of the batched FF-out launch (OMLM_DECODE_SPLITK_FLOATS): slabs + one zeroed arrival counter per 16 output rows; the
        # attention kernel's combine counts per sample in the same array, so it holds at least DEC4_NB counters (B > 16: per group, and B)
        self.splitk_ws = torch.empty(sizes["splitk_ws"], device=self.x.device)
        self.splitk_cnt = torch.zeros(sizes["splitk_cnt"], dtype=torch.int32, device=self.x.device)
        a.splitk_ws, a.splitk_cnt = self.splitk_ws.data_ptr(), self.splitk_cnt.data_ptr()
        a.kv16, a.k_new = (1, self.k_new.data_ptr()) if self.k_new is not None else (0, None)
        self.args = a

    # ---- prompt: the batched forward over all known rows, keeping what the single-row steps need ---------------------
    def prefill(self, all_token_ids: List[torch.Tensor], key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """all_token_ids: the conditioning sequences followed by the ids sampled so far (may be empty).  Returns the
        [B, ldV] logits of the last row (they predict the next id) and leaves the caches filled for rows < N.
        key_mask (a decoder built with key_mask=True only): [B, N] bool / uint8, True = attend -- the batched forward runs under it and the
        steps keep it for the prompt's rows; None: every row is attended."""
        if key_mask is not None and self.key_live is None:
            raise ValueError("prefill: a key mask needs a decoder built with key_mask=True")
        model, tr = self.model, self.model.transformer
        ids32, lens = engine.build_ids(model, all_token_ids)
        B, N = ids32.shape
        assert B == self.B and N <= self.Nmax, (B, N, self.B, self.Nmax)
        P = engine.prefix_rows(tr)
        if N < P:
            raise ValueError(f"cached decode of a model with a non-causal prefix of {P} rows needs them all in the prompt; got {N} rows")
        lay = engine.get_layout(model, B, lens, ids32.device, True)
        x = engine.embed_forward(model, ids32, lay)
        km = None
        if key_mask is not None:
            if tuple(key_mask.shape) != (B, N):
                raise ValueError(f"prefill: key_mask must be [{B}, {N}], got {tuple(key_mask.shape)}")
            km = key_mask.to(device=ids32.device, dtype=torch.uint8).contiguous()
        y, y_lo, saved = engine.trunk_forward(tr, self.pw, x, km, B, N, True, False, keep_h1_lo_tail=self.planes)
        nseq = len(model.token_sequences)
        logits = engine.heads_forward(model, self.pw, y, y_lo, lay, [s == nseq - 1 for s in range(nseq)])[-1]
        for l, sv in enumerate(saved["layers"]):
            self.Kc[l][:, :N].copy_(sv.k.view(B, N, -1))         # (sv.k / sv.v are in the operand dtype: a 16-bit cache takes them as they are)
            self.Vc[l][:, :N].copy_(sv.v.view(B, N, -1))
            h1 = sv.h1.view(B, N, -1)
            self.hist[l].zero_()
            take = min(2, N)
            self.hist[l][:, 2 - take:].copy_(h1[:, N - take:])
            if self.planes:                                  # the conv state of "fp16ff" is the un-rounded h1 = hi + lo
                self.hist[l][:, 2 - take:].add_(sv.h1_lo_tail[:, 2 - take:])
        if self.key_live is not None:
            self.key_live.fill_(1)
            if km is not None:
                self.key_live[:, :N].copy_(km)
        self.rows = N
        self.pos_dev.fill_(N)
        return logits

    def _step_call(self, ids: torch.Tensor):
        """The step's library call on the decoder's argument block: omlm_decode_step, or under a key mask omlm_decode_step_masked."""
        if self.key_live is None:
            call("omlm_decode_step", C.addressof(self.args), ptr(ids), stream_ptr())
        else:
            call("omlm_decode_step_masked", C.addressof(self.args), ptr(self.key_live), ptr(ids), stream_ptr())

    def step(self, new_ids: torch.Tensor, k: int) -> torch.Tensor:
        """Append the row of ``new_ids`` ([B] int64: the k-th sampled id of every sample, k counted from 0) and return the
        [B, ldV] logits that predict id k + 1 (quantizer head (k + 1) mod Q)."""
        if self.rows >= self.Nmax:
            raise RuntimeError(f"decode cache full ({self.Nmax} rows)")
        a = self.args
        a.emb_row_offset = self.codebook * (k % self.Q) if self.Q > 1 else 0
        head = self.pw.heads[-1][(k + 1) % self.Q]
        a.head_W = head.data_ptr()
        a.head_W_lo = self.pw.heads_lo[-1][(k + 1) % self.Q].data_ptr() if self.planes else None
        ids = new_ids.contiguous()
        assert ids.dtype == torch.int64 and ids.numel() == self.B
        a.emb_table = self.emb.data_ptr()
        if self.pos_emb is not None:
            # the new row = token embedding (with the reference's offset / clamp rule of dec_embed_kernel) + position row k, formed here
            rows = (ids + a.emb_row_offset).clamp_(0, self.emb.shape[0] - 1)
            self.x.copy_(self.emb[rows] + self.pos_emb[k])
            a.emb_table = None
        a.advance_pos, a.advance_step = self.pos_dev.data_ptr(), None        # the head kernel moves the row index on
        self._step_call(ids)
        self.rows += 1
        return self.logits


def _guided(guidance) -> bool:
    """Whether a guidance argument (not yet checked) turns guidance on: a per-row sequence always does; a number unless it is None or 1."""
    if isinstance(guidance, (list, tuple)) or getattr(guidance, "ndim", 0) == 1:
        return True
    return ops.check_cond_scale(guidance, "guidance") is not None


def _per_row_topk(topk, P: int, V1: int):
    """The sampler's count k: a number as it is; a sequence of length P as a list of ints, each in [1, V1] (a ValueError names the entry)."""
    def entry(v):
        return int(v) if isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= V1 else None
    return ops.per_row_checked(topk, P, "topk", lambda s: s, entry, f"an integer in [1, {V1}]")


class SamplingLoop:
    """sample -> embed -> 6 layers -> head -> advance, per id, for one CachedDecoder.

    The uniforms are a buffer [n_new, B, V1] or, with ``rng=(seed, row0)`` and ``uniforms=None``, the counter stream of include/omlm.h
    (row0: global index of this decoder's first sample).
    All per-step state (row index, step counter, uniforms, id history) is device resident, so the cycle of each quantizer
    phase can be captured into a HIP graph (``use_graph=True``: after one eager cycle per phase, the remaining ids are graph
    replays, ~1 host launch per id instead of ~32).  Measured on MI355X the step is GPU-bound (32 dependent kernels per id) and
    graph replay is no faster than back-to-back eager launches, so eager is the default; the graph path
    is kept (and tested) for hosts that cannot keep up.
    Both sampler calls of the cycle are omlm_sample on a block built once.  ``top_p`` < 1: the sampler keeps the nucleus of the top-k set
    (include/omlm.h).
    ``logprobs``: the loop owns ``lp_model`` and ``lp_sampled`` ([n_new, B] fp32, device resident: the two log-probabilities of every
    sampled id, include/omlm.h) and the calls go through omlm_sample_lp instead, which writes row *step_dev of each -- a
    captured cycle stays valid.  The ids are those of the loop without it; ``run()`` still returns them.
    ``guidance`` = s (classifier-free guidance, include/omlm.h; None or 1: off, the loop is the one it is without the argument): the
    decoder holds B = 2P rows -- rows [0, P) the prompts, rows [P, 2P) their null twins, stacked by the caller for ``prefill`` -- and the
    loop samples P ids per step: the uniforms are [n_new, P, V1] (counter stream: row0 is the global PROMPT index), ``hist``, ``lp_*`` and
    the result are sized P.  Per id: omlm_guide_logits forms g = null + s (cond - null) from the two halves of dec.logits into a buffer of
    the loop that the sampler reads (so ``lp_model`` is the log-softmax of g); the sampler gathers the embedding rows of the P ids;
    omlm_decode_twin hands ids and rows to the null half; then the step runs on all 2P rows as it is.  Two more launches per id, all
    pointers fixed: the captured cycle holds all of it.
    Per-row settings: ``temperature``, ``topk`` (the counts k), ``top_p``, ``guidance`` and the seed of ``rng`` may each be a sequence of
    length P, one value per row the sampler serves (checked here, before any device work: ops.per_row_*).  The loop uploads them once as
    [P] device arrays and stores the pointers beside the argument blocks it builds once per phase, so a captured cycle stays valid; the
    sampler calls are then omlm_sample_rows and a per-row ``guidance`` is combined by omlm_guide_logits_rows (every row beside its twin,
    the rows of scale 1 included).  With per-row seeds every row draws with stream sample index 0 -- u(t, 0, c) of its own seed, what a
    one-sample loop with that seed draws -- and ``rng[1]`` is not read.
    Which sampler and guidance entries the cycle calls follows from the settings alone (ops.sampler_call, ops.guide_call) and is resolved
    once, here: ``_cycle`` makes the calls it finds."""

    def __init__(self, dec: CachedDecoder, first_logits: torch.Tensor, uniforms: Optional[torch.Tensor], n0: int, n_new: int, topk: int,
                 temperature: float, forbid_by_phase: Sequence[bool], use_graph: bool = True, rng=None, top_p=None,
                 logprobs: bool = False, guidance=None):
        ops.check_sampler_width(dec.V1)                    # before any launch: the loop's first sampler call would refuse it
        P = self.P = dec.B // 2 if _guided(guidance) else dec.B                  # rows the sampler serves
        self.top_p = ops.per_row_top_p(top_p, P)           # 1.0: no nucleus
        self.guidance = ops.per_row_cond_scale(guidance, P, "guidance")        # None: off
        if self.guidance is not None and dec.B % 2:
            raise ValueError(f"SamplingLoop: guidance needs a decoder of 2P rows (prompts, then their null twins); it holds {dec.B}")
        if (uniforms is None) == (rng is None):
            raise ValueError("SamplingLoop: give either the uniforms [n_new, B, V1] or rng=(seed, row0), not both and not neither")
        temperature, topk = ops.per_row_temperature(temperature, P), _per_row_topk(topk, P, dec.V1)
        seeds = ops.per_row_seed(rng[0], P, "rng seed") if rng is not None else None
        self.dec, self.n0, self.n_new, self.topk = dec, n0, n_new, topk
        self.temperature = temperature if isinstance(temperature, list) else float(temperature)
        self.forbid = [bool(f) for f in forbid_by_phase]
        dev = dec.logits.device
        if rng is None:
            assert uniforms.shape == (n_new, P, dec.V1) and uniforms.dtype == torch.float32 and uniforms.is_contiguous()
        self.U = uniforms
        # counter stream (include/omlm.h): sample b of this decoder draws u(step, row0 + b, c) from the seed -- no buffer; seed halves
        # and row0 are plain arguments, so a captured cycle holds for the whole call.  Zeros where they are not read (a buffer; row seeds)
        self.seed, self.row0 = ((0, 0), 0) if rng is None or isinstance(seeds, list) else (ops.split_seed(seeds), int(rng[1]))
        self.hist = torch.zeros(n_new, P, device=dev, dtype=torch.long)
        self.cur = torch.zeros(dec.B, device=dev, dtype=torch.long)             # guided: the sampler writes [0, P), the twin copy [P, 2P)
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        self.logprobs = bool(logprobs)
        self.lp_model = torch.zeros(n_new, P, device=dev, dtype=torch.float32) if self.logprobs else None
        self.lp_sampled = torch.zeros(n_new, P, device=dev, dtype=torch.float32) if self.logprobs else None
        # guided: the sampler reads the combined rows from here, dec.logits keeps both branches
        self.guided = torch.zeros(P, dec.ldV, device=dev, dtype=torch.float32) if self.guidance is not None else None
        src = dec.logits if self.guidance is None else self.guided
        # per-row settings: uploaded once, [P] each, and kept here beside the row block that points at them (None: no list was given)
        up = self._upload = ops.SamplerSettings(P, topk, self.temperature, self.top_p, self.guidance, seeds, self.logprobs).upload(dev)
        self._rows = up.block()
        # the sampler's argument blocks (ops.SampleArgs), built once: per quantizer phase, without and with the embedding gather of the
        # sampled id.  Every pointer in them is a fixed buffer of this loop or its decoder.

        def block(phase: int, embed: bool):
            sa = ops.SampleArgs(ptr(src), P, dec.V1, dec.ldV, ptr(self.U), *self.seed, 0, self.row0, ptr(self.step_dev), ptr(self.cur),
                                ptr(self.hist), up.k, up.temperature, up.top_p, int(self.forbid[phase]))
            if embed:
                sa.emb_table, sa.emb_row_offset, sa.emb_rows = dec.emb.data_ptr(), dec.codebook * phase if dec.Q > 1 else 0, dec.emb.shape[0]
                sa.x, sa.D = ptr(dec.x), dec.D
            return sa
        self._blocks = [(block(phase, False), block(phase, True)) for phase in range(dec.Q)]
        # which entry points the cycle calls, with their arguments in front of the stream: resolved here, once (ops.sampler_call /
        # ops.guide_call); g = null + s (cond - null) goes from the two halves of dec.logits into the sampler's rows
        self._sample_calls = [tuple(ops.sampler_call(sa, self._rows, self.lp_model, self.lp_sampled) for sa in pair) for pair in self._blocks]
        self._guide_call = None if self.guidance is None else ops.guide_call(ptr(dec.logits), dec.logits[P:].data_ptr(), ptr(self.guided), P,
                                                                             dec.V1, dec.ldV, up.guidance)
        dec.logits.copy_(first_logits)
        self.use_graph = use_graph
        self.graphs = {}

    def _cycle(self, k: int, with_decode: bool):
        """Sample id number k (global index in the predicted sequence) from dec.logits, then compute its row."""
        dec, a = self.dec, self.dec.args
        # with_decode, 32 launches per id: the sampler also gathers the embedding row of the id it picked (the step's first launch), and
        # the head kernel (the step's last) moves the row index and the sampler's step counter on
        if self._guide_call is not None:
            call(self._guide_call[0], *self._guide_call[1], stream_ptr())
        name, args = self._sample_calls[k % dec.Q][with_decode]
        call(name, *args, stream_ptr())
        if not with_decode:
            return
        P = self.P
        if self.guidance is not None:      # the null twins decode the same ids: ids and gathered embedding rows to rows [P, 2P)
            call("omlm_decode_twin", ptr(self.cur), self.cur[P:].data_ptr(), ptr(dec.x), dec.x[P:].data_ptr(), P, dec.D, stream_ptr())
        if dec.pos_emb is not None:
            # + absolute position row of id k = n0 + (device step counter): device-side indexing, so a captured cycle stays valid
            dec.x.add_(dec.pos_emb.index_select(0, (self.step_dev + self.n0).long()))
        a.emb_table = None
        a.head_W = dec.pw.heads[-1][(k + 1) % dec.Q].data_ptr()
        a.head_W_lo = dec.pw.heads_lo[-1][(k + 1) % dec.Q].data_ptr() if dec.planes else None
        a.advance_pos, a.advance_step = dec.pos_dev.data_ptr(), self.step_dev.data_ptr()
        dec._step_call(self.cur)

    def run(self) -> torch.Tensor:
        """Returns the [n_new, B] sampled ids."""
        dec, Q = self.dec, self.dec.Q
        for i in range(self.n_new):
            k, last = self.n0 + i, i == self.n_new - 1
            if last:
                self._cycle(k, False)
                break
            if dec.rows >= dec.Nmax:
                raise RuntimeError(f"decode cache full ({dec.Nmax} rows)")
            g = self.graphs.get(k % Q)
            if g is not None:
                g.replay()
            elif self.use_graph and i >= Q and (self.n_new - 1 - i) >= 2 * Q:
                # every phase has run eagerly once: capture this phase's cycle (capture records, it does not execute) ...
                try:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._cycle(k, True)
                    self.graphs[k % Q] = g
                    g.replay()                                   # ... and run it for this id
                except Exception:                                # pragma: no cover - capture support depends on the runtime
                    self.use_graph = False
                    torch.cuda.synchronize()
                    self._cycle(k, True)
            else:
                self._cycle(k, True)
            dec.rows += 1
        return self.hist
