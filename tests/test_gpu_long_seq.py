"""GPU: causal attention with 16-bit operands past 4096 positions per sample (the long forms of attention2.hip / attention3.hip), through the
C ABI against fp64 torch, and the model at such a length against the CPU oracle.

The fp64 reference is test_gpu_kernels.naive_attention's arithmetic (test_gpu_attn_dropout.masked_attention's with a keep-mask) evaluated head
by head and in blocks of REF_BLK queries against the keys up to the block's last row, each block's backward run before the next block's
forward: the [B, H, N, N] scores of the original would be 2 GB per head at N = 16384, a block is 130 MB.

Inputs follow test_attention_fwd_bwd (unit q and k, randn v, a randn * 2 table, 20 % dead keys with key 0 alive); where N allows, the whole
key tile 4160 .. 4223 is dead as well -- a V tile read as zeros and a ballot word past the 64 the short forward holds.  The bars are that
test's own: forward 1e-2 (bf16) / 2e-3 (fp16), backward and d(bias) 2e-2 / 4e-3, max-norm relative."""
import pytest
import torch

from test_gpu_model import RELPOS_TENSORS, TOL, grad_unscale, rel_l2, relerr as model_relerr, report

pytestmark = pytest.mark.gpu

REF_BLK = 1024
TOL_F = {torch.bfloat16: 1e-2, torch.float16: 2e-3}
TOL_B = {torch.bfloat16: 2e-2, torch.float16: 4e-3}


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from open_musiclm_amd import ops as o
    return o


@pytest.fixture(scope="module")
def NL(ops):
    return ops.attn_max_positions(torch.float16, 0)


def blocked_attention(q, k, v, bias, keymask, H, do=None, keep=None, p=0.0, scale=8.0):
    """q [B, N, H*64], k, v [B, N, 64] fp64; bias [N, >= H] fp64 or None; keymask [B, N] bool; keep [B, H, N, N] bool or None (dropout p).
    Returns out [B, N, H*64] fp64 and, with do [B, N, H*64], the gradients (dq, dk, dv, dbias) of sum(out * do)."""
    B, N, _ = q.shape
    leaves = [t.detach().clone().requires_grad_(do is not None) for t in (q, k, v)] + \
             ([bias.detach().clone().requires_grad_(do is not None)] if bias is not None else [])
    qr, kr, vr = leaves[:3]
    br = leaves[3] if bias is not None else None
    out = torch.empty(B, N, H * 64, dtype=torch.float64, device=q.device)
    neg = -torch.finfo(torch.float32).max
    for b in range(B):
        for h in range(H):
            for i0 in range(0, N, REF_BLK):
                i1 = min(N, i0 + REF_BLK)
                sim = (qr[b, i0:i1, 64 * h:64 * h + 64] @ kr[b, :i1].t()) * scale
                rel = torch.arange(i0, i1, device=q.device)[:, None] - torch.arange(i1, device=q.device)[None, :]
                if br is not None:
                    sim = sim + br[:, h][rel.clamp(min=0)]
                sim = sim.masked_fill(~keymask[b, None, :i1], neg).masked_fill(rel < 0, neg)
                attn = sim.softmax(-1)
                if keep is not None:
                    attn = attn * keep[b, h, i0:i1, :i1].to(attn.dtype) / (1.0 - p)
                o = attn @ vr[b, :i1]
                out[b, i0:i1, 64 * h:64 * h + 64] = o.detach()
                if do is not None:
                    (o * do[b, i0:i1, 64 * h:64 * h + 64]).sum().backward()
    if do is None:
        return out, None
    return out, tuple(t.grad for t in leaves) + ((None,) if bias is None else ())


_CASES = {}


def _case(dev, dtype, B, N, H, p=0.0, ops=None):
    """Inputs of one (dtype, B, N, H) case and its fp64 forward / backward, built once and shared by the tests that need them."""
    key = (dtype, B, N, H, p)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(N + H)
    M = B * N
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    q = unit(torch.randn(B, N, H, 64, generator=g)).reshape(M, H * 64).to(dev)
    k = unit(torch.randn(M, 64, generator=g)).to(dev)
    v = torch.randn(M, 64, generator=g).to(dev)
    ldb = (H + 7) // 8 * 8
    bias = torch.zeros(N, ldb)
    bias[:, :H] = torch.randn(N, H, generator=g) * 2
    bias = bias.to(dev)
    keymask = (torch.rand(B, N, generator=g) > 0.2)
    keymask[:, 0] = True
    if N >= 4224:
        keymask[:, 4160:4224] = False                     # one whole 64-key tile past the short forward's 64 ballot words
    keymask = keymask.to(dev)
    do = torch.randn(B, N, H * 64, generator=g).to(dev)
    c = dict(B=B, N=N, H=H, M=M, ldb=ldb, qd=q.to(dtype), kd=k.to(dtype), vd=v.to(dtype), bias=bias, keymask=keymask,
             km8=keymask.to(torch.uint8), do=do, dod=do.reshape(M, -1).to(dtype).contiguous())
    if p > 0:
        c["seed"], c["salt"] = 0xC0FFEE + N, torch.tensor([3], dtype=torch.int64, device=dev)
        c["keep"] = ops.attn_dropout_keep(B, N, H, p, c["seed"], seed_dev=c["salt"], device=dev).bool()
    c["ref"], c["grads"] = blocked_attention(c["qd"].double().view(B, N, H * 64), c["kd"].double().view(B, N, 64), c["vd"].double().view(B, N, 64),
                                             bias.double(), keymask, H, do=c["dod"].double().view(B, N, H * 64), keep=c.get("keep"), p=p)
    c.pop("keep", None)
    _CASES[key] = c
    return c


def _forward(ops, dev, c, bias, dtype, **kw):
    out = torch.empty(c["M"], c["H"] * 64, device=dev, dtype=dtype)
    lse = torch.empty(c["B"], c["H"], c["N"], device=dev)
    ops.attn_fwd(c["qd"], c["kd"], c["vd"], bias, c["km8"], out, lse, c["B"], c["N"], c["H"], 8.0, **kw)
    return out, lse


def _backward(ops, dev, c, bias, out, lse, dbias=None, **kw):
    B, N, H, M = c["B"], c["N"], c["H"], c["M"]
    dq = torch.empty(M, H * 64, device=dev)
    dk = torch.empty(M, 64, device=dev)
    dv = torch.empty(M, 64, device=dev)
    dbias = torch.zeros(N, c["ldb"], device=dev) if dbias is None else dbias
    delta = torch.empty(B, H, N, device=dev)
    ops.attn_bwd(c["qd"], c["kd"], c["vd"], bias, c["km8"], out, c["dod"], lse, delta, dq, dk, dv, dbias, B, N, H, 8.0, **kw)
    return dq, dk, dv, dbias


def _flag(ab, H):
    return float(ab.tableT.view(-1, ab.tableT.numel() // ((H + 7) // 8 * 8))[0, -2])


def _shapes(NL):
    return [(2, 4097, 2), (1, 5003, 3), (1, 8229, 9), (1, NL, 1)]


# T1 ----------------------------------------------------------------------------------------------------------------------------------------
# (2, 4097, 2): the first ragged tile past the old limit, one key in ballot word 64.  (1, 5003, 3): past the first-generation dQ kernel's
# LDS limit (about 4330), H not a multiple of 8 (idle waves), N odd.  (1, 8229, 9): two head groups, crosses 8192, more than a hundred
# flushes of the dQ kernel's 128-bin window.  (1, NL, 1), fp16 only: the ceiling -- LDS budget and workspace layout at their largest.
@pytest.mark.parametrize("dtype,case", [(torch.bfloat16, 0), (torch.float16, 0), (torch.bfloat16, 1), (torch.float16, 1),
                                        (torch.bfloat16, 2), (torch.float16, 2), (torch.float16, 3)])
def test_long_attention_vs_fp64(ops, dev, NL, dtype, case):
    B, N, H = _shapes(NL)[case]
    c = _case(dev, dtype, B, N, H)
    ref, (rq, rk, rv, rb) = c["ref"], c["grads"]
    out, lse = _forward(ops, dev, c, c["bias"], dtype)                     # raw table: prepared on the way, online softmax
    e_f = relerr(out.view(B, N, -1), ref)
    dq, dk, dv, dbias = _backward(ops, dev, c, c["bias"], out, lse)        # the workspace form
    errs = dict(fwd=e_f, dq=relerr(dq.view(B, N, -1), rq), dk=relerr(dk.view(B, N, -1), rk), dv=relerr(dv.view(B, N, -1), rv),
                dbias=relerr(dbias[:, :H], rb[:, :H]))
    print(f"long_attention[{dtype},{B},{N},{H}] " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    report(f"long_attention[{dtype},{B},{N},{H}]", **errs)
    assert float(dbias[:, H:].abs().max() if c["ldb"] > H else 0.0) == 0.0
    assert e_f < TOL_F[dtype], errs
    assert max(errs["dq"], errs["dk"], errs["dv"], errs["dbias"]) < TOL_B[dtype], errs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_long_attention_prepared_forms_and_null_workspace(ops, dev, dtype):
    """(2, 4097, 2): the AttnBias(qk_bound=1.0) prepared form -- bf16 takes the fixed reference point with the +-2 table, fp16 with the narrow
    bias * 0.05 table and half=True -- with the flag and |lse - lse_online| asserted as test_attention_fwd_bwd does, and the null-workspace
    d(bias) form on top of an existing table (the * 0.5 check of that test)."""
    B, N, H = 2, 4097, 2
    c = _case(dev, dtype, B, N, H)
    out, lse = _forward(ops, dev, c, c["bias"], dtype)
    if dtype == torch.bfloat16:
        ab = ops.AttnBias(c["bias"], N, H, dev, qk_bound=1.0, scale=8.0)
        assert _flag(ab, H) == 1.0                                        # the fixed path is taken
        out2, lse2 = _forward(ops, dev, c, ab, dtype)
        e_f2, e_lse = relerr(out2.view(B, N, -1), c["ref"]), float((lse2 - lse).abs().max())
        print(f"long_attention_fixed[{dtype}] fwd {e_f2:.2e} lse_diff {e_lse:.2e}")
        assert e_f2 < TOL_F[dtype] and e_lse < 1e-2, (e_f2, e_lse)
        # the backward from the fixed form's lse (relative to the table's reference point)
        dq, dk, dv, dbias = _backward(ops, dev, c, ab, out2, lse2)
        rq, rk, rv, rb = c["grads"]
        eb = (relerr(dq.view(B, N, -1), rq), relerr(dk.view(B, N, -1), rk), relerr(dv.view(B, N, -1), rv), relerr(dbias[:, :H], rb[:, :H]))
        print(f"long_attention_fixed[{dtype}] bwd " + " ".join(f"{e:.2e}" for e in eb))
        assert max(eb) < TOL_B[dtype], eb
    else:
        ab0 = ops.AttnBias(c["bias"], N, H, dev, qk_bound=1.0, scale=8.0, half=True)
        assert _flag(ab0, H) == 0.0                                       # the +-2 table is too wide for half: online softmax
        out0, lse0 = _forward(ops, dev, c, ab0, dtype)
        assert torch.equal(out0, out) and torch.equal(lse0, lse)          # same online kernel, same bits
        bias_s = c["bias"] * 0.05
        ab = ops.AttnBias(bias_s, N, H, dev, qk_bound=1.0, scale=8.0, half=True)
        assert _flag(ab, H) == 1.0                                        # the fixed path is taken
        out2, lse2 = _forward(ops, dev, c, ab, dtype)
        out3, lse3 = _forward(ops, dev, c, bias_s, dtype)                 # raw table: online softmax
        ref_s, _ = blocked_attention(c["qd"].double().view(B, N, H * 64), c["kd"].double().view(B, N, 64), c["vd"].double().view(B, N, 64),
                                     bias_s.double(), c["keymask"], H)
        e_f2, e_f3 = relerr(out2.view(B, N, -1), ref_s), relerr(out3.view(B, N, -1), ref_s)
        e_lse = float((lse2 - lse3).abs().max())
        print(f"long_attention_fixed[{dtype}] fwd {e_f2:.2e} fwd_online {e_f3:.2e} lse_diff {e_lse:.2e}")
        assert e_f2 < TOL_F[dtype] and e_f3 < TOL_F[dtype] and e_lse < 2e-3, (e_f2, e_f3, e_lse)
    # null workspace: d(bias) by atomics straight into the table, accumulated on top of what is there
    dq, dk, dv, dbias = _backward(ops, dev, c, c["bias"], out, lse)
    dbias2 = dbias.clone()
    _backward(ops, dev, c, c["bias"], out, lse, dbias=dbias2, workspace=False)
    e_b2 = relerr(dbias2[:, :H] * 0.5, c["grads"][3][:, :H])
    print(f"long_attention_null_workspace[{dtype}] dbias {e_b2:.2e}")
    assert e_b2 < TOL_B[dtype], e_b2


# T2 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_forward_is_causal_across_4096(ops, dev, dtype):
    """The long forward walks the key tiles as the short one does: rows < 4096 of an N = 4097 call are, bit for bit, the N = 4096 call on the
    first 4096 rows of the same tensors and mask (online form from the raw table, and the fixed form where the dtype takes it)."""
    B, H, N = 2, 2, 4097
    c = _case(dev, dtype, B, N, H)
    first = lambda t, w: t.view(B, N, w)[:, :4096].contiguous().view(B * 4096, w)
    forms = [c["bias"]]
    if dtype == torch.bfloat16:
        forms.append("fixed")
    for form in forms:
        if isinstance(form, str):
            # one table prepared at N = 4097 cannot serve N = 4096 (another row pitch): prepare each from the same rows; the reference point
            # m_h must be the same, so the largest entry of every head is put inside the first 4096 rows
            bias = c["bias"].clone()
            bias[0, :H] = bias[:, :H].max() + 1.0
            b_long = ops.AttnBias(bias, N, H, dev, qk_bound=1.0, scale=8.0)
            b_short = ops.AttnBias(bias[:4096].contiguous(), 4096, H, dev, qk_bound=1.0, scale=8.0)
            assert _flag(b_long, H) == 1.0 and _flag(b_short, H) == 1.0
        else:
            b_long, b_short = form, form[:4096].contiguous()
        out, lse = _forward(ops, dev, c, b_long, dtype)
        o2 = torch.empty(B * 4096, H * 64, device=dev, dtype=dtype)
        l2 = torch.empty(B, H, 4096, device=dev)
        ops.attn_fwd(first(c["qd"], H * 64), first(c["kd"], 64), first(c["vd"], 64), b_short, c["km8"][:, :4096].contiguous(), o2, l2,
                     B, 4096, H, 8.0)
        assert torch.equal(out.view(B, N, -1)[:, :4096], o2.view(B, 4096, -1))
        assert torch.equal(lse[..., :4096], l2)


# T3 ----------------------------------------------------------------------------------------------------------------------------------------
def test_long_attention_dropout(ops, dev):
    """p = 0.1 at (1, 4200, 2), fp16: forward and backward against fp64 with the keep-mask of ops.attn_dropout_keep (35 MB) at the bars of
    test_gpu_attn_dropout's kernel test for fp16 (2e-3 / 4e-3); lse is the p = 0 call's, bit for bit."""
    dtype, B, N, H, p = torch.float16, 1, 4200, 2, 0.1
    c = _case(dev, dtype, B, N, H, p=p, ops=ops)
    kw = dict(p=p, seed=c["seed"], seed_dev=c["salt"])
    out, lse = _forward(ops, dev, c, c["bias"], dtype, **kw)
    out0, lse0 = _forward(ops, dev, c, c["bias"], dtype)
    assert torch.equal(lse, lse0)                                         # the denominator is the undropped one
    assert not torch.equal(out, out0)
    rq, rk, rv, rb = c["grads"]
    e_f = relerr(out.view(B, N, -1), c["ref"])
    dq, dk, dv, dbias = _backward(ops, dev, c, c["bias"], out, lse, **kw)
    eb = (relerr(dq.view(B, N, -1), rq), relerr(dk.view(B, N, -1), rk), relerr(dv.view(B, N, -1), rv), relerr(dbias[:, :H], rb[:, :H]))
    print(f"long_attention_dropout fwd {e_f:.2e} dq {eb[0]:.2e} dk {eb[1]:.2e} dv {eb[2]:.2e} dbias {eb[3]:.2e}")
    assert e_f < 2e-3, e_f
    assert max(eb) < 4e-3, eb


# T4 ----------------------------------------------------------------------------------------------------------------------------------------
def _tiny_inputs(dev, dtype, B, N, H):
    g = torch.Generator().manual_seed(5)
    M = B * N
    q = torch.nn.functional.normalize(torch.randn(M, H, 64, generator=g), dim=-1).reshape(M, H * 64).to(dev, dtype)
    k = torch.nn.functional.normalize(torch.randn(M, 64, generator=g), dim=-1).to(dev, dtype)
    v = torch.randn(M, 64, generator=g).to(dev, dtype)
    return q, k, v


def test_limits_binding(ops, NL):
    from open_musiclm_amd import hip
    lib = hip.lib()
    assert NL >= 16384
    assert lib.omlm_attn_max_positions(1, 0) == NL and lib.omlm_attn_max_positions(2, 0) == NL
    assert 3000 < lib.omlm_attn_max_positions(0, 0) < 4096                # fp32 operands: the LDS-resident table of the first-generation dQ kernel
    assert 4096 <= lib.omlm_attn_max_positions(1, 14) < 5003              # a prefix: the first-generation kernels past 4096
    assert lib.omlm_attn_max_positions(9, 0) == 0 and lib.omlm_attn_max_positions(1, -1) == 0


def test_above_the_ceiling_is_refused_before_any_launch(ops, dev, NL):
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    dtype, B, N, H = torch.float16, 1, NL + 1, 1
    q, k, v = _tiny_inputs(dev, dtype, B, N, H)
    bias = torch.randn(N, 8, device=dev)
    out = torch.full((N, H * 64), 7.0, device=dev, dtype=dtype)
    lse = torch.full((B, H, N), 7.0, device=dev)
    with pytest.raises(RuntimeError, match=str(NL)):
        ops.attn_fwd(q, k, v, bias, None, out, lse, B, N, H, 8.0)
    # the library itself, handed a prepared table of that length
    tabT = torch.zeros(int(ops.hip.lib().omlm_attn_bias_table_floats(N, H, 0)), device=dev)
    with pytest.raises(RuntimeError, match=str(NL)):
        call("omlm_mqa_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(bias), ptr(tabT), None, ptr(out), ptr(lse), B, N, H, 8.0, 8, ops.dcode(dtype), 0, 0.0,
             0, None, stream_ptr())
    grads = [torch.full((N, w), 7.0, device=dev) for w in (H * 64, 64, 64, 8)]
    delta = torch.full((B, H, N), 7.0, device=dev)
    with pytest.raises(RuntimeError, match=str(NL)):
        ops.attn_bwd(q, k, v, bias, None, out, out, lse, delta, *grads, B, N, H, 8.0)
    with pytest.raises(RuntimeError, match=str(NL)):
        call("omlm_mqa_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(bias), ptr(tabT), None, ptr(out), ptr(out), ptr(lse), ptr(delta), ptr(grads[0]),
             ptr(grads[1]), ptr(grads[2]), ptr(grads[3]), None, B, N, H, 8.0, 8, ops.dcode(dtype), 0, 0.0, 0, None, stream_ptr())
    torch.cuda.synchronize(dev)
    for t in [out, lse, delta] + grads:
        assert bool((t == 7.0).all())                                     # nothing was launched on the outputs


def test_fp32_operands_keep_their_limit_and_say_so(ops, dev):
    """fp32 operands ("bf16x3") run the first-generation kernels: at N = 5003 the backward is refused with the fp32 limit in the message
    (the forward alone still fits its half-sized table, as before)."""
    B, N, H = 1, 5003, 2
    lim = ops.attn_max_positions(torch.float32, 0)
    q, k, v = _tiny_inputs(dev, torch.float32, B, N, H)
    bias = torch.randn(N, 8, device=dev)
    out = torch.empty(N, H * 64, device=dev)
    lse = torch.empty(B, H, N, device=dev)
    ops.attn_fwd(q, k, v, bias, None, out, lse, B, N, H, 8.0)
    grads = [torch.full((N, w), 7.0, device=dev) for w in (H * 64, 64, 64, 8)]
    delta = torch.empty(B, H, N, device=dev)
    with pytest.raises(RuntimeError, match=rf"fp32 operands.*N <= {lim}\b"):
        ops.attn_bwd(q, k, v, bias, None, out, out, lse, delta, *grads, B, N, H, 8.0)
    torch.cuda.synchronize(dev)
    assert all(bool((t == 7.0).all()) for t in grads)


def test_prefix_past_4096_says_so(ops, dev):
    """A non-causal prefix is served by the second-generation kernels to N = 4096; past it the first-generation kernels take over as far as
    their LDS-resident tables reach -- P = 14 at N = 4097 with 8 heads is past that (the dK / dV kernel stages 8 columns), and the refusal
    names the prefix and the limits instead of the bare LDS message."""
    dtype, B, N, H, P = torch.float16, 1, 4097, 8, 14
    q, k, v = _tiny_inputs(dev, dtype, B, N, H)
    bias = torch.randn(N + P - 1, 8, device=dev)
    out = torch.empty(N, H * 64, device=dev, dtype=dtype)
    lse = torch.empty(B, H, N, device=dev)
    ops.attn_fwd(q, k, v, bias, None, out, lse, B, N, H, 8.0, P=P)         # the first-generation forward's table still fits
    grads = [torch.full((N, w), 7.0, device=dev) for w in (H * 64, 64, 64)] + [torch.full((N + P - 1, 8), 7.0, device=dev)]
    delta = torch.empty(B, H, N, device=dev)
    with pytest.raises(RuntimeError, match=r"non-causal prefix \(P = 14\).*4096"):
        ops.attn_bwd(q, k, v, bias, None, out, out, lse, delta, *grads, B, N, H, 8.0, P=P)
    torch.cuda.synchronize(dev)
    assert all(bool((t == 7.0).all()) for t in grads)
    # far enough out, the first-generation forward's table no longer fits either
    N2 = 11003
    q, k, v = _tiny_inputs(dev, dtype, B, N2, H)
    with pytest.raises(RuntimeError, match=r"non-causal prefix \(P = 14\)"):
        ops.attn_fwd(q, k, v, torch.randn(N2 + P - 1, 8, device=dev), None, torch.empty(N2, H * 64, device=dev, dtype=dtype),
                     torch.empty(B, H, N2, device=dev), B, N2, H, 8.0, P=P)


# T5 ----------------------------------------------------------------------------------------------------------------------------------------
def test_long_backward_is_bit_reproducible(ops, dev):
    """(1, 8229, 9) fp16, workspace form, three runs: dq, dk, dv and dbias are the same bits.  (The dK / dV kernel leaves per-workgroup slots
    that are summed in a fixed order; at B = 1 the d(bias) reduction adds one value per bin.)"""
    dtype, B, N, H = torch.float16, 1, 8229, 9
    c = _case(dev, dtype, B, N, H)
    out, lse = _forward(ops, dev, c, c["bias"], dtype)
    runs = []
    for rep in range(3):
        if rep == 1:                                                      # recycled, non-zero memory behind every torch.empty of the call
            junk = [torch.full((n,), float("nan"), device=dev) for n in (B * N * H * 64, B * N * 64, B * N * 64, 1 << 24)]
            del junk
        runs.append(_backward(ops, dev, c, c["bias"], out, lse))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


# T6 ----------------------------------------------------------------------------------------------------------------------------------------
# The model of test_gpu_geometry.py's pattern past 4096 positions: coarse stage, dim 128, 2 heads, depth 2, conv feed-forward, continuous
# rel-pos bias, ff_dropout 0, B = 1, time steps [1, 400, 1500] -> N = 4917.
LONG_LENS = [1, 400, 1500]
DEPTH = 2


def _build(precision, dev):
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    torch.manual_seed(0)                                                  # same weights in every precision: one oracle
    model = M.create_coarse_transformer(dim=128, depth=DEPTH, heads=2, use_conv_ff=True, relative_position_bias_type="continuous",
                                        ff_dropout=0.0, precision=precision, num_coarse_quantizers=3)
    spec = O.coarse_spec(dim=128, depth=DEPTH, heads=2, use_conv_ff=True, relative_position_bias_type="continuous")
    return model.to(dev), spec


def _grad_names(nseq):
    return ["transformer.layers.0.0.to_q.weight", "transformer.layers.1.0.to_kv.weight", "transformer.layers.0.0.to_out.0.weight",
            "transformer.layers.1.0.norm.gamma", "transformer.layers.0.2.0.gamma", "transformer.layers.1.2.4.gamma",
            "transformer.layers.0.2.1.weight", "transformer.layers.1.2.1.weight", "transformer.layers.1.2.6.weight",
            "transformer.layers.0.2.6.weight", "transformer.norm.gamma", f"embeddings.{nseq - 1}.weight", f"logit_weights.{nseq - 1}",
            "transformer.layers.0.2.2.ds_conv.weight", "transformer.layers.1.2.2.ds_conv.weight"] + RELPOS_TENSORS


_ORACLE = {}


def _oracle(model, spec):
    """Oracle loss, final-sequence logits (of every row: the cached steps read them too) and gradients of the training step, once."""
    from oracle import musiclm_oracle as O
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if not _ORACLE:
        ids = O.synthetic_ids(spec, 1, LONG_LENS, seed=1234)
        N = O.build_training_inputs(ids, spec)[2].shape[1]
        assert N == 4917, N
        noise = torch.randn(1, N, generator=torch.Generator().manual_seed(7))
        nseq = len(ids)
        weights = [0.] * (nseq - 1) + [1.]
        names = _grad_names(nseq)
        sdo = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
        assert all(sdo[k].requires_grad for k in names)
        o_loss, o_logits, _ = O.wrapper_forward_loss(sdo, spec, ids, weights, forget_noise=noise)
        o_grads = dict(zip(names, torch.autograd.grad(o_loss, [sdo[k] for k in names])))
        _ORACLE.update(ids=ids, noise=noise, weights=weights, names=names, loss=float(o_loss.detach()), logits=o_logits[-1].detach(),
                       grads=o_grads, N=N)
    return _ORACLE


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp16ff"])
def test_model_training_step_past_4096(dev, precision):
    """(a) forward + backward of TokenConditionedTransformerWrapper at N = 4917, forgetful mask injected: final-sequence logits, loss and the
    gradient families of test_gpu_geometry at TOL[precision]."""
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    import open_musiclm_amd.open_musiclm as MM
    model, spec = _build(precision, dev)
    o = _oracle(model, spec)
    orig = MM.generate_mask_with_prob
    MM.generate_mask_with_prob = lambda shape, p, device: O.forgetful_mask_from_noise(o["noise"], p).to(device)
    try:
        wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False,
                                                       cross_entropy_loss_weights=o["weights"], mask_prob=0.15)
        wrapper.train()
        loss, logits, _ = wrapper(all_token_ids=[t.to(dev) for t in o["ids"]], return_loss=True)
        loss.backward()
    finally:
        MM.generate_mask_with_prob = orig
    assert logits[-1].shape == o["logits"].shape
    e_inf, e_l2 = model_relerr(logits[-1], o["logits"]), rel_l2(logits[-1], o["logits"])
    e_loss = abs(float(loss) - o["loss"]) / o["loss"]
    params = dict(model.named_parameters())
    gmax = max(float(v.abs().max()) for v in o["grads"].values())
    grads = {k: model_relerr(params[k].grad * grad_unscale(precision), o["grads"][k],
                             floor=1e-2 * gmax if (k in RELPOS_TENSORS and k.endswith("bias")) else 0.0) for k in o["names"]}
    worst = max(grads.items(), key=lambda kv: kv[1])
    print(f"long_model_train[{precision}] N {o['N']} logits_inf {e_inf:.2e} logits_l2 {e_l2:.2e} loss {e_loss:.2e} worst_grad {worst}")
    report(f"long_model_train[{precision}]", N=o["N"], logits_inf=e_inf, logits_l2=e_l2, loss=e_loss, worst_grad=worst, grads=grads)
    tol = TOL[precision]
    assert e_inf < tol["logits"], (e_inf, e_l2)
    assert e_loss < tol["loss"], e_loss
    assert worst[1] < tol["grad"], grads


def _flat_prompt(o, spec):
    """The training ids as a prompt: the conditioning sequences with their eos, and the predicted sequence's ids flattened."""
    from open_musiclm_amd.utils import append_eos_id
    ids = o["ids"]
    condx = [append_eos_id(t.reshape(1, -1).long(), e) for t, e in zip(ids[:-1], spec.eos_ids)]
    return condx, ids[-1].reshape(1, -1).long()


def test_cached_steps_from_a_long_prompt(dev):
    """(b) CachedDecoder(model, 1, N + 8, "fp16") prefilled with the first N - 8 rows, then 8 teacher-forced steps, each against the oracle's
    forward of the whole sequence at TOL["fp16"]["logits"]: sampling from a long prompt needs only the batched forward."""
    from open_musiclm_amd import decode
    from oracle import musiclm_oracle as O
    model, spec = _build("fp16", dev)
    model.eval()
    o = _oracle(model, spec)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    condx, flat = _flat_prompt(o, spec)
    N = o["N"]
    head = sum(t.shape[-1] + 1 for t in condx) + 1                        # rows in front of the predicted sequence's first id (start tokens)
    n_known = N - 8 - head                                                # ids of the predicted sequence inside the first N - 8 rows
    with torch.no_grad():
        ref = O.token_conditioned_forward(sd, spec, condx + [flat], only_final=True)[-1]     # row j predicts id j
        dec = decode.CachedDecoder(model, 1, N + 8, "fp16")
        got = [dec.prefill([t.to(dev) for t in condx] + [flat[:, :n_known].to(dev)]).clone()]
        fl = flat.to(dev)
        assert head + flat.shape[1] == N and dec.rows == N - 8
        for kk in range(n_known, n_known + 8):
            got.append(dec.step(fl[:, kk].contiguous(), kk).clone())
        torch.cuda.synchronize(dev)
    V1 = spec.token_sequences[-1].codebook_size + 1
    errs = [model_relerr(lg[:, :V1], ref[:1, n_known + i]) for i, lg in enumerate(got)]
    print(f"long_cached_steps prefill rows {head + n_known} errs {[f'{e:.2e}' for e in errs]}")
    assert dec.rows == N and len(errs) == 9 and max(errs) < TOL["fp16"]["logits"], errs


def test_generate_from_a_long_prompt(dev):
    """(c) generate(use_cache=True) from a prompt of more than 4096 rows completes and returns ids inside the codebook."""
    from open_musiclm_amd import open_musiclm as M
    model, spec = _build("fp16", dev)
    model.eval()
    o = _oracle(model, spec)
    ids = o["ids"]
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    first_step = ids[-1].shape[1] - 100                                   # 1400 time steps of 3 quantizers known: 4617 rows in front
    assert sum(t[0].numel() + 1 for t in ids[:-1]) + 1 + first_step * 3 > 4096
    out = wrapper.generate(conditioning_token_ids=[t.to(dev) for t in ids[:-1]], pred_token_ids=ids[-1][:, :first_step].to(dev),
                           max_time_steps=first_step + 2, use_cache=True)
    Q = spec.token_sequences[-1].num_quantizers
    assert out.shape == (1, first_step + 2, Q)
    cb = spec.token_sequences[-1].codebook_size
    assert bool(((out >= 0) & (out < cb)).all())
    assert torch.equal(out[:, :first_step].cpu(), ids[-1][:, :first_step])
