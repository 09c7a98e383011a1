"""Plain fp64 restatement of the multi-query attention of include/omlm.h -- forward, log2-domain lse and every gradient from explicit
formulas -- with, for every result, the tensor of TERM SUMS (the same expression with every factor replaced by its absolute value), the case
table of the tile-edge tests and their per-element checker.  Used by tests/test_attn_edge_host.py (CPU) and tests/test_gpu_attn_edges.py
(GPU, against the kernels).  No package import: torch only, on whatever device the inputs live.

Shapes: q, dout [B, N, H*64]; k, v [B, N, 64]; bias [N + Pn - 1, >= H] (row = i - j + Pn - 1, Pn = min(P, N); P = 0: [N, >= H]) or None;
keymask [B, N] bool or None.  Score (i, j) is live iff (j <= i or (i < Pn and j < Pn)) and the key mask keeps j.  With S the live scores
(scale q.k + bias) and P their row softmax:
    O = P V       lse = log2 sum_j exp(S)        dV = P^T dO      dP = dO V^T      delta = rowsum(dO o O)      dS = P o (dP - delta)
    dQ = scale dS K          dK = scale dS^T Q          dbias[i - j + Pn - 1, h] += dS[b, h, i, j]
A query row without any live key has out = 0, lse = DEAD_LSE and adds nothing to any gradient (Result.dead flags it).

Term sums: out -- max |v_j| over the row's live keys (a convex combination of them cannot leave that range); dS -- P o (|dO| |V|^T +
sum_d |dO_d| |O_d|), NOT |dS|: the kernels' error in dS comes from the rounding of O and P and does not shrink where dP - delta cancels;
dV -- P^T |dO|; dQ, dK, dbias -- the dS term sum through |K|, |Q| and the plain sum.  check() divides each element's error by its term
sum, so a dropped key, a distance off by one or a wrong head column shows at full size in the row it hits, however long the other rows are.
"""
import math
from collections import namedtuple

import torch

DEAD_LSE = 1.0e30
LOG2E = 1.4426950408889634
TENSORS = ("out", "dq", "dk", "dv", "dbias")         # the results check() takes; lse is compared in absolute terms
Result = namedtuple("Result", "val term dead")       # val: name -> fp64 tensor (with "lse"); term: name -> term sums; dead [B, N] bool

# wrong formulas, applied to the reference only (never to a kernel): what the edge cases must be able to tell from rounding
MUTANTS = {
    "dist_plus_1": "bias distance i - j + 1",
    "strict_causal": "j < i for j <= i",
    "drop_key_64": "key 64 dropped",
    "drop_key_last": "key N - 1 dropped",
    "mask_next_sample": "sample b's key mask applied to sample b + 1",
    "last_row_as_prev": "query row N - 1 computed as row N - 2",
    "head_next_column": "head h's bias column read as column (h + 1) mod H",
    "dbias_256": "d(bias) rows >= 256 dropped",
}


def _round(x, dtype):
    return x if dtype is None else x.to(dtype).double()


def _split(x):
    """(hi, lo) bf16 planes of fp32 operands, as the "bf16x3" forward takes them (csrc/common.h: split_pair): hi = x TRUNCATED to bf16,
    lo = bf16(x - hi) to nearest -- so lo reaches 2^-7 |x| and the lo lo product that is left out 2^-14 of the product"""
    x32 = x.float().contiguous()
    hi = (x32.view(torch.int32) & -65536).view(torch.float32).double()
    return hi, (x32.double() - hi).to(torch.bfloat16).double()


def _x3(eq, a, b):
    """a . b as three bf16 products with exact accumulation: hi hi + hi lo + lo hi (the lo lo product is left out)"""
    (ah, al), (bh, bl) = _split(a), _split(b)
    return torch.einsum(eq, ah, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, al, bh)


def _attention(q, k, v, bias, keymask, dout, H, scale, P, dtype, mutant, terms=True):
    assert mutant is None or mutant in MUTANTS, mutant
    B, N, _ = q.shape
    dev = q.device
    Pn = min(P, N)
    off = Pn - 1 if Pn > 0 else 0
    qh = q.double().view(B, N, H, 64).permute(0, 2, 1, 3)              # [B, H, N, 64]
    doh = dout.double().view(B, N, H, 64).permute(0, 2, 1, 3)
    kd, vd = k.double(), v.double()
    pos = torch.arange(N, device=dev)
    qpos = pos.clone()
    if mutant == "last_row_as_prev" and N >= 2:                          # row N - 1 takes row N - 2's query, position and causal limit
        qpos[N - 1] = N - 2
        qh = qh[:, :, qpos]
    rel = qpos[:, None] - pos[None, :]                                   # [N, N]
    live = (rel > 0 if mutant == "strict_causal" else rel >= 0) | ((qpos[:, None] < Pn) & (pos[None, :] < Pn))
    live = live[None].expand(B, N, N)
    if keymask is not None:
        km = keymask.bool()
        if mutant == "mask_next_sample":
            km = torch.roll(km, 1, 0)
        live = live & km[:, None, :]
    if mutant == "drop_key_64" and N > 64:
        live = live & (pos != 64)[None, None, :]
    if mutant == "drop_key_last":
        live = live & (pos != N - 1)[None, None, :]
    nrows = N + off
    idx = ((rel + 1 if mutant == "dist_plus_1" else rel) + off).clamp(0, nrows - 1)
    x3 = dtype == torch.float32          # fp32 operands: the forward runs the bf16x3 split, the backward single-pass bf16 MFMAs
    s = (_x3("bhid,bjd->bhij", qh, kd) if x3 else torch.einsum("bhid,bjd->bhij", qh, kd)) * scale
    if bias is not None:
        bh = bias.double()[:, :H]
        if mutant == "head_next_column":
            bh = torch.roll(bh, -1, 1)
        s = s + bh.t()[:, idx][None]
    lv = live[:, None]                                                   # [B, 1, N, N]
    s2 = torch.where(lv, s * LOG2E, torch.full_like(s, -math.inf))
    m = s2.max(-1, keepdim=True).values
    dead = ~live.any(-1)                                                 # [B, N]
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = _round(torch.exp2(s2 - m), dtype)                                # the forward's P: rounded BEFORE it is summed and multiplied by V
    l = p.sum(-1, keepdim=True)
    ok = l > 0
    lsafe = torch.where(ok, l, torch.ones_like(l))
    o = _round((_x3("bhij,bjd->bhid", p, vd) if x3 else torch.einsum("bhij,bjd->bhid", p, vd)) / lsafe, dtype)     # out in the operand type
    if x3:                                                               # the backward's operands: q, k, v, dO in bf16 (delta: unrounded)
        b16 = lambda t: t.to(torch.bfloat16).double()
        dtype, delta_do, qh, kd, vd, doh = torch.bfloat16, doh, b16(qh), b16(kd), b16(vd), b16(doh)
        s2 = torch.einsum("bhid,bjd->bhij", qh, kd) * scale
        if bias is not None:
            s2 = s2 + bh.t()[:, idx][None]
        s2 = torch.where(lv, s2 * LOG2E, torch.full_like(s2, -math.inf))
    else:
        delta_do = doh
    lse = torch.where(ok, m + torch.log2(lsafe), torch.full_like(l, DEAD_LSE))[..., 0]
    pb = torch.where(lv & ok, torch.exp2(s2 - torch.where(ok, lse[..., None], torch.zeros_like(l))), torch.zeros_like(s))
    pbr = _round(pb, dtype)                                              # the backward's P, from the forward's lse
    dv = torch.einsum("bhij,bhid->bjd", pbr, doh)
    dp = torch.einsum("bhid,bjd->bhij", doh, vd)
    delta = (delta_do * o).sum(-1, keepdim=True)
    ds = _round(pb * (dp - delta), dtype)
    dq = scale * torch.einsum("bhij,bjd->bhid", ds, kd)
    dk = scale * torch.einsum("bhij,bhid->bjd", ds, qh)
    flat = idx.reshape(-1)
    dbias = torch.zeros(nrows, H, dtype=torch.float64, device=dev).index_add_(0, flat, ds.sum(0).reshape(H, N * N).t().contiguous())
    if mutant == "dbias_256":
        dbias[off + 256:] = 0.0
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * 64)
    val = dict(out=rows(o), lse=lse, dq=rows(dq), dk=dk, dv=dv, dbias=dbias)
    if not terms:
        return Result(val, None, dead)
    # ---- term sums: every factor by its absolute value
    vmax = vd.abs().max(-1).values                                       # [B, N]
    t_out = torch.where(live, vmax[:, None, :].expand(B, N, N), torch.zeros((), dtype=torch.float64, device=dev)).max(-1).values
    t_out = t_out[:, :, None].expand(B, N, H * 64)
    t_ds = pb * (torch.einsum("bhid,bjd->bhij", doh.abs(), vd.abs()) + (doh.abs() * o.abs()).sum(-1, keepdim=True))
    t_dv = torch.einsum("bhij,bhid->bjd", pb, doh.abs())
    t_dq = scale * torch.einsum("bhij,bjd->bhid", t_ds, kd.abs())
    t_dk = scale * torch.einsum("bhij,bhid->bjd", t_ds, qh.abs())
    t_db = torch.zeros(nrows, H, dtype=torch.float64, device=dev).index_add_(0, flat, t_ds.sum(0).reshape(H, N * N).t().contiguous())
    term = dict(out=t_out, dq=rows(t_dq), dk=t_dk, dv=t_dv, dbias=t_db)
    return Result(val, term, dead)


def reference(q, k, v, bias, keymask, dout, H, scale, P=0, *, mutant=None, terms=True):
    """The fp64 results and their term sums (Result).  Inputs are already rounded to the operand type.  mutant: one of MUTANTS (the
    wrong formula's results); terms=False leaves the term sums out (Result.term is None)."""
    return _attention(q, k, v, bias, keymask, dout, H, scale, P, None, mutant, terms)


def emulate(q, k, v, bias, keymask, dout, H, scale, dtype, P=0):
    """The same reference with the kernels' stated rounding points (include/omlm.h; the comments of test_attention_fwd_bwd): the forward's P
    rounded to `dtype` before it is summed (the denominator, hence lse) and multiplied by V; O in `dtype`; dO as given; the backward's P
    (from that lse) and dS rounded to `dtype`.  Everything else fp64.
    dtype = float32 ("bf16x3"): the forward's two products from the operands' bf16 hi / lo planes without the lo lo term, P and O in fp32;
    the backward as for bf16 on q, k, v and dO rounded to bf16 (its kernels run single-pass bf16 MFMAs), delta from the unrounded dO and O."""
    return _attention(q, k, v, bias, keymask, dout, H, scale, P, dtype, None)


def check(got, ref, termsum, tol=None):
    """(worst, index): the largest |got - ref| / max(termsum, 1e-6 max termsum) over the elements and where it is reached, so that a failure
    names the row, head and distance.  tol is only reported by callers; nothing is asserted here."""
    ref = ref.double()
    got = got.double().reshape(ref.shape)
    floor = max(1e-6 * float(termsum.max()), 1e-300)
    err = ((got - ref).abs() / termsum.double().clamp(min=floor)).reshape(-1)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)        # a NaN is the worst error, not an ignored one
    at = int(err.argmax())
    worst, index = float(err[at]), []
    for n in reversed(ref.shape):
        index.append(at % n)
        at //= n
    return worst, tuple(reversed(index))


# ---- tolerances: the project's own (test_attention_fwd_bwd), applied per element of the term sums --------------------------------------
# fp32 operands, forward: the project's 2e-5 is a bound on max |a - b| / max |b| over the whole tensor.  Per element the "bf16x3" forward does
# not meet it and is not meant to: its hi planes are TRUNCATED (split_pair), so a lo plane reaches 2^-7 of its operand, the lo lo product that
# is left out 2^-14 of the product, and the two roundings of lo another 2^-16 each -- X3_EPS = 1.5 2^-14 per product.  With unit q and k
# (sum_d |q_d| |k_d| <= 1) a score is off by at most scale X3_EPS, lse (log2) by that times log2 e, the probabilities by at most twice that in
# sum, and P V adds X3_EPS of its own.  emulate(float32) reproduces the kernels' worst elements to three digits (3.29e-5 of the row's
# max |v|, 9.8e-5 in lse, where these bounds are 1.6e-3 and 1.1e-3): the bounds are the format's, not fitted to them.
X3_EPS = 1.5 * 2.0 ** -14
SCALE_CASES = 8.0


def tol_fwd(dtype):
    return {torch.float32: (2 * SCALE_CASES + 1) * X3_EPS, torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype]


def tol_bwd(dtype):
    return {torch.float32: 2e-2, torch.bfloat16: 2e-2, torch.float16: 4e-3}[dtype]


def tol_lse(dtype):
    """absolute, log2 domain: the lse of the 16-bit kernels takes the MFMA denominator of the rounded P"""
    return {torch.float32: SCALE_CASES * X3_EPS * LOG2E, torch.bfloat16: 1e-2, torch.float16: 2e-3}[dtype]


def tol_of(name, dtype):
    return tol_fwd(dtype) if name == "out" else tol_lse(dtype) if name == "lse" else tol_bwd(dtype)


def worst_ratio(got, ref, dtype):
    """{tensor: (metric / tolerance, metric, index)} of `got` (name -> tensor) against the Result `ref`; lse in absolute terms."""
    res = {}
    for name in TENSORS:
        e, at = check(got[name], ref.val[name], ref.term[name])
        res[name] = (e / tol_of(name, dtype), e, at)
    d = (got["lse"].double() - ref.val["lse"]).abs()
    sentinel = float(torch.tensor(DEAD_LSE, dtype=got["lse"].dtype))                  # 1e30 as the result's type holds it
    d = torch.where((ref.val["lse"] == DEAD_LSE) & (got["lse"].double() == sentinel), torch.zeros_like(d), d)
    d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
    at = int(d.reshape(-1).argmax())
    B, H, N = d.shape
    res["lse"] = (float(d.reshape(-1)[at]) / tol_lse(dtype), float(d.reshape(-1)[at]), (at // (H * N), at // N % H, at % N))
    return res


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
B_CASES = 3            # rowbase = b N is non-zero and no power of two
EDGE_N = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257)
HEAD_N = (33, 129, 257)            # these also run H = 1, 8, 9, 16 (9: a second 8-head group with one active head)
PATTERNS = ("none", "dense", "picket", "rpad", "rpad2", "hole")
Case = namedtuple("Case", "name N H pattern")


def _cases():
    out = []
    for N in EDGE_N:
        for H in (3,) + ((1, 8, 9, 16) if N in HEAD_N else ()):
            for pat in PATTERNS:
                if pat == "rpad2" and N < 65:        # lengths (64, 65, min(128, N)): a second right-padded batch where N allows
                    continue
                if pat == "hole" and N <= 64:        # no key of [64, 128) or [128, 256) exists: the same mask as `dense`
                    continue
                out.append(Case(f"N{N}-H{H}-{pat}", N, H, pat))
    return tuple(out)


CASES = _cases()


def _dense(N, g):
    km = torch.rand(B_CASES, N, generator=g) > 0.2
    km[:, 0] = True
    return km


def make_keymask(case, g):
    """[B, N] bool (None for `none`), a different mask per sample; key 0 is live in every pattern (rows without a live key have a test of
    their own)."""
    N, pat = case.N, case.pattern
    if pat == "none":
        return None
    if pat in ("dense", "hole"):
        km = _dense(N, g)
        if pat == "hole":
            km[0, 64:128] = False          # a whole 64-key tile
            km[1, 128:256] = False         # a whole 128-key range
        return km
    km = torch.zeros(B_CASES, N, dtype=torch.bool)
    if pat == "picket":                    # at most ten live keys, all on seams, every other tile dead
        for b in range(B_CASES):
            for j in (0, 31 + b, 32, 33, 63, 64 + b, 65, 127, 128 + b, N - 1 - b):
                if 0 <= j < N:
                    km[b, j] = True
        return km
    lengths = (N, 1, min(33, N)) if pat == "rpad" else (64, 65, min(128, N))
    for b, n in enumerate(lengths):
        km[b, :n] = True
    return km


def make_inputs(case, dtype, seed=None):
    """CPU tensors of one case, rounded to the operand type: unit-normalised q and k, random v and dout, a table of 2 randn
    (as test_attention_fwd_bwd draws them).  Returns dict(q, k, v, dout [.., dtype], bias [N, ceil8(H)] fp32, keymask bool or None)."""
    N, H = case.N, case.H
    g = torch.Generator().manual_seed(1000 * N + 10 * H + PATTERNS.index(case.pattern) if seed is None else seed)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    q = unit(torch.randn(B_CASES, N, H, 64, generator=g)).reshape(B_CASES, N, H * 64).to(dtype)
    k = unit(torch.randn(B_CASES, N, 64, generator=g)).to(dtype)
    v = torch.randn(B_CASES, N, 64, generator=g).to(dtype)
    dout = torch.randn(B_CASES, N, H * 64, generator=g).to(dtype)
    if N > 256:
        # Distance 256 -- the first row of the d(bias) reduce's second block -- holds ONE score pair per sample and head: (N - 1, 0).  A random
        # dO makes dP - delta of that pair cancel to anything between 0 and 1 of its term sum; dO = v_0 in every head makes dP the full
        # sum |v_0|^2, so that losing the row costs about half its term sum wherever row N - 1 sees more than one key.
        dout[:, N - 1] = v[:, 0].repeat(1, H)
    ldb = (H + 7) // 8 * 8
    bias = torch.zeros(N, ldb)
    bias[:, :H] = torch.randn(N, H, generator=g) * 2
    keymask = make_keymask(case, g)
    if N > 256 and keymask is not None:
        # ... and a sample with ONE live key (rpad's length 1) has P = 1 there and dS = 0 whatever the formula: with dO = 0 in that row it
        # adds nothing to the distance's term sum either, instead of burying the other samples' pairs under a term nothing can produce
        dout[keymask.sum(1) == 1, N - 1] = 0
    return dict(q=q, k=k, v=v, dout=dout, bias=bias, keymask=keymask)


# ---- the routes of tests/test_gpu_attn_edges.py: what it hands ops.attn_fwd / ops.attn_bwd, and hence which kernels serve it -------------------
# table: "raw" (the fp32 table; ops prepares it for P = 0), "fixed" (an AttnBias with the fixed reference point; fp16: on the table x 0.05,
# which its 28-octave window takes), "none" (no bias, no d(bias)).  ws: the d(bias) workspace (False: atomics into the table).
Route = namedtuple("Route", "name dtypes table P ws cases")
FIXED_TABLE_SCALE = {torch.bfloat16: 1.0, torch.float16: 0.05}
ROUTES = (
    Route("fp32", (torch.float32,), "raw", 0, True, CASES),                               # first generation, precise
    Route("online", (torch.bfloat16, torch.float16), "raw", 0, True, CASES),              # second / third generation, online softmax
    Route("fixed", (torch.bfloat16, torch.float16), "fixed", 0, True, CASES),             # ... the fixed reference point
    Route("nobias", (torch.bfloat16, torch.float16), "none", 0, True, CASES),             # the empty-descriptor path
    Route("prefix1", (torch.bfloat16, torch.float16), "raw", 1, True, CASES),             # first generation, 16-bit (a prefix of one row is causal)
    Route("atomic", (torch.bfloat16, torch.float16), "raw", 0, False, tuple(c for c in CASES if c.N in HEAD_N)),
)


def plan_row(route, dtype, case, backward):
    """the call a route makes for a case, in the vocabulary of tests/attn_routes.json (tests/test_attn_plan_host.py: call_of)"""
    prepared = route.P == 0                   # ops.attn_fwd / attn_bwd: a raw table (or none) is prepared for P = 0, handed over as it is for P >= 1
    bias = {"raw": "T" if prepared else "raw", "fixed": "T", "none": "zeroT"}[route.table]
    return dict(dir="bwd" if backward else "fwd", dt=str(dtype).replace("torch.", ""), B=B_CASES, N=case.N, H=case.H, P=route.P, bias=bias,
                dbias=backward and route.table != "none", ws=route.ws, split=True)
