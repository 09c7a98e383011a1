"""Attention dropout on the GPU: the keep-mask hook against the numpy restatement of include/omlm.h, the kernels against fp64 torch
with that mask, the to_out dropout kernels, and a training step against the oracle with the same masks injected."""
import numpy as np
import pytest
import torch

import attn_dropout_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from open_musiclm_amd import ops as o
    return o


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("salt", [None, 11])
def test_keep_hook_equals_numpy_restatement(ops, dev, salt):
    sd = torch.tensor([salt], dtype=torch.int64, device=dev) if salt is not None else None
    for p in (0.1, 0.5):
        got = ops.attn_dropout_keep(2, 77, 2, p, 0x123456789ABCDEF, seed_dev=sd, device=dev).cpu().numpy().astype(bool)
        assert np.array_equal(got, R.attn_keep(2, 77, 2, p, 0x123456789ABCDEF, salt)), p


def masked_attention(q, k, v, bias, keymask, H, keep, p, scale=8.0):
    """fp64 reference: softmax probabilities times keep / (1 - p) before P V.  keep [B, H, N, N] bool."""
    B, N, _ = q.shape
    qh = q.view(B, N, H, 64).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bjd->bhij", qh, k) * scale
    idx = (torch.arange(N, device=q.device)[:, None] - torch.arange(N, device=q.device)[None, :]).clamp(min=0)
    sim = sim + bias[:, :H].t()[:, idx]
    neg = -torch.finfo(torch.float32).max
    sim = sim.masked_fill(~keymask[:, None, None, :], neg)
    sim = sim.masked_fill(torch.ones(N, N, dtype=torch.bool, device=q.device).triu(1), neg)
    attn = sim.softmax(-1) * keep.to(sim.dtype) / (1.0 - p)
    out = torch.einsum("bhij,bjd->bhid", attn, v)
    return out.permute(0, 2, 1, 3).reshape(B, N, H * 64)


CASES = [(torch.float32, 2, 77, 2), (torch.bfloat16, 2, 77, 2), (torch.float16, 2, 77, 2), (torch.bfloat16, 1, 200, 5),
         (torch.float16, 1, 200, 5), (torch.float32, 1, 200, 5), (torch.bfloat16, 1, 1817, 16), (torch.float16, 1, 1817, 16),
         (torch.float32, 1, 1817, 16), (torch.bfloat16, 2, 20, 3), (torch.float16, 2, 20, 3),
         (torch.float16, 32, 1116, 8), (torch.bfloat16, 8, 1817, 16)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype,B,N,H", CASES)
def test_attention_dropout_fwd_bwd(ops, dev, dtype, B, N, H, p):
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
    keymask = keymask.to(dev)
    km8 = keymask.to(torch.uint8)
    qd, kd, vd = q.to(dtype), k.to(dtype), v.to(dtype)
    seed, salt = 0xC0FFEE + N, torch.tensor([3], dtype=torch.int64, device=dev)
    # the bf16 fixed softmax form too: q, k unit vectors (|q.k| <= 1)
    forms = [("raw", bias)] + ([("fixed", ops.AttnBias(bias, N, H, dev, qk_bound=1.0, scale=8.0))] if dtype == torch.bfloat16 else [])
    keep = ops.attn_dropout_keep(B, N, H, p, seed, seed_dev=salt, device=dev).bool() if N <= 200 else \
        torch.from_numpy(R.attn_keep(B, N, H, p, seed, 3)).to(dev)
    qr = qd.double().view(B, N, H * 64).requires_grad_(True)
    kr = kd.double().view(B, N, 64).requires_grad_(True)
    vr = vd.double().view(B, N, 64).requires_grad_(True)
    br = bias.double().requires_grad_(True)
    ref = masked_attention(qr, kr, vr, br, keymask, H, keep, p)
    do = torch.randn(B, N, H * 64, generator=g).to(dev)
    ref.backward(do.double())
    dod = do.reshape(M, -1).to(dtype).contiguous()
    tol_f = 2e-5 if dtype == torch.float32 else (1e-2 if dtype == torch.bfloat16 else 2e-3)
    tol_b = 4e-3 if dtype == torch.float16 else 2e-2
    for form, ab in forms:
        out = torch.empty(M, H * 64, device=dev, dtype=dtype)
        lse = torch.empty(B, H, N, device=dev)
        ops.attn_fwd(qd, kd, vd, ab, km8, out, lse, B, N, H, 8.0, p=p, seed=seed, seed_dev=salt)
        out0 = torch.empty_like(out); lse0 = torch.empty_like(lse)
        ops.attn_fwd(qd, kd, vd, ab, km8, out0, lse0, B, N, H, 8.0)
        assert torch.equal(lse, lse0), form                                  # the denominator is the undropped one
        e_f = relerr(out.view(B, N, -1), ref.detach())
        # same (seed, salt): same bits; another salt or seed: another output
        out2 = torch.empty_like(out); out3 = torch.empty_like(out); lse2 = torch.empty_like(lse)
        ops.attn_fwd(qd, kd, vd, ab, km8, out2, lse2, B, N, H, 8.0, p=p, seed=seed, seed_dev=salt)
        ops.attn_fwd(qd, kd, vd, ab, km8, out3, lse2, B, N, H, 8.0, p=p, seed=seed, seed_dev=salt + 1)
        assert torch.equal(out, out2) and not torch.equal(out, out3), form
        ops.attn_fwd(qd, kd, vd, ab, km8, out3, lse2, B, N, H, 8.0, p=p, seed=seed + 1, seed_dev=salt)
        assert not torch.equal(out, out3), form
        dq = torch.empty(M, H * 64, device=dev)
        dk = torch.empty(M, 64, device=dev)
        dv = torch.empty(M, 64, device=dev)
        dbias = torch.zeros(N, ldb, device=dev)
        delta = torch.empty(B, H, N, device=dev)
        ops.attn_bwd(qd, kd, vd, ab, km8, out, dod, lse, delta, dq, dk, dv, dbias, B, N, H, 8.0, p=p, seed=seed, seed_dev=salt)
        e_q, e_k, e_v = relerr(dq.view(B, N, -1), qr.grad), relerr(dk.view(B, N, -1), kr.grad), relerr(dv.view(B, N, -1), vr.grad)
        e_b = relerr(dbias[:, :H], br.grad[:, :H])
        print(f"attn_dropout[{dtype},{B},{N},{H},p={p},{form}] fwd {e_f:.2e} dq {e_q:.2e} dk {e_k:.2e} dv {e_v:.2e} dbias {e_b:.2e}")
        assert e_f < tol_f, (form, e_f)
        assert max(e_q, e_k, e_v, e_b) < tol_b, (form, e_q, e_k, e_v, e_b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_attn_at_p0_ignores_seed_and_salt(ops, dev, dtype):
    """p = 0 is no dropout whatever the seed and salt: omlm_mqa_attn_fwd / _bwd with p = 0, seed 77 and a device salt give what the
    default call (p = 0, seed 0, no salt) gives."""
    from open_musiclm_amd import hip
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    B, N, H = 2, 150, 3
    g = torch.Generator().manual_seed(1)
    M = B * N
    q = torch.nn.functional.normalize(torch.randn(M, H, 64, generator=g), dim=-1).reshape(M, -1).to(dev, dtype)
    k = torch.nn.functional.normalize(torch.randn(M, 64, generator=g), dim=-1).to(dev, dtype)
    v = torch.randn(M, 64, generator=g).to(dev, dtype)
    bias = torch.randn(N, 8, generator=g).to(dev)
    ab = ops.AttnBias(bias, N, H, dev)
    salt = torch.tensor([5], dtype=torch.int64, device=dev)
    outs = []
    for seed, seed_dev in ((0, None), (77, salt)):
        out = torch.empty(M, H * 64, device=dev, dtype=dtype); lse = torch.empty(B, H, N, device=dev)
        call("omlm_mqa_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(bias), ptr(ab.tableT), None, ptr(out), ptr(lse), B, N, H, 8.0, 8, ops.dcode(dtype),
             0, 0.0, seed, ptr(seed_dev), stream_ptr())
        do = torch.randn(M, H * 64, generator=g).to(dev, dtype) if not outs else outs[0][-1]
        dq = torch.empty(M, H * 64, device=dev); dk = torch.empty(M, 64, device=dev); dv = torch.empty(M, 64, device=dev)
        db = torch.zeros(N, 8, device=dev); delta = torch.empty(B, H, N, device=dev)
        call("omlm_mqa_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(bias), ptr(ab.tableT), None, ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dq),
             ptr(dk), ptr(dv), ptr(db), None, B, N, H, 8.0, 8, ops.dcode(dtype), 0, 0.0, seed, ptr(seed_dev), stream_ptr())
        outs.append((out, lse, dq, dk, dv, db, do))
    # out, lse and dQ are written without atomics: the same bits; dK / dV / d(bias) are summed with float atomics in a run-dependent order
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0][3:6], outs[1][3:6]):
        assert relerr(a, b) < 1e-5
    assert hip.lib() is not None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dropout_residual_kernels(ops, dev, dtype):
    M, D, p, seed = 300, 136, 0.3, 4242
    salt = torch.tensor([9], dtype=torch.int64, device=dev)
    g = torch.Generator().manual_seed(2)
    x, y, dx1 = (torch.randn(M, D, generator=g).to(dev) for _ in range(3))
    keep = torch.from_numpy(R.resid_keep(M, D, p, seed, 9)).to(dev)
    x1 = torch.empty(M, D, device=dev)
    ops.dropout_residual_fwd(x, y, x1, p, seed, seed_dev=salt)
    ref = x.double() + keep.double() * y.double() / (1 - p)
    assert relerr(x1, ref) < 1e-6
    dy = torch.empty(M, D, device=dev, dtype=dtype)
    ops.dropout_residual_bwd(dx1, dy, p, seed, seed_dev=salt)
    rs = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))              # the kernel's fp32 scale, one rounding of the product
    ref_b = torch.where(keep, dx1 * rs.to(dev), torch.zeros_like(dx1))
    assert torch.equal(dy != 0, keep)                                     # the mask exactly (dx1 has no zeros)
    ulp = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}[dtype]
    assert float(((dy.float() - ref_b).abs() / ref_b.abs().clamp(min=1e-30))[keep].max()) <= ulp


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _model(dev, precision, attn_dropout, dim=128, depth=2, heads=2):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_coarse_transformer(dim=dim, depth=depth, heads=heads, num_coarse_quantizers=3, attn_dropout=attn_dropout, ff_dropout=0.0,
                                       clap_codebook_size=64, semantic_codebook_size=64, acoustic_codebook_size=64,
                                       precision=precision).to(dev)


def _spec(dim, depth, heads):
    from oracle import musiclm_oracle as O
    return O.ModelSpec([O.SeqInfo(64, 12), O.SeqInfo(64, 1), O.SeqInfo(64, 3)], dim=dim, depth=depth, heads=heads)


def _masked_oracle_attention(O, state, p, B, dev):
    """the oracle's attention (oracle/musiclm_oracle.py) with layer l's engine masks applied: the probabilities before P V and the output of
    to_out, rebuilt from engine.dropout_state through the keep hook and the numpy restatement"""
    import torch.nn.functional as F
    salt = torch.tensor([state["salt"]], dtype=torch.int64, device=dev)
    from open_musiclm_amd import ops

    def attention(sd, pfx, x, bias, key_mask, spec):
        l = int(pfx.split("layers.")[1].split(".")[0])
        b, n, _ = x.shape
        h, dh = spec.heads, spec.dim_head
        keep = ops.attn_dropout_keep(b, n, h, p, state["attn"][l], seed_dev=salt, device=dev).bool().cpu()
        keep_o = torch.from_numpy(R.resid_keep(b * n, x.shape[-1], p, state["out"][l], state["salt"])).view(b, n, -1)
        xn = O.layer_norm(x, sd[pfx + "norm.gamma"])
        q = F.linear(xn, sd[pfx + "to_q.weight"])
        kv = F.linear(x, sd[pfx + "to_kv.weight"])
        k, v = kv[..., :dh], kv[..., dh:]
        q = q.view(b, n, h, dh).permute(0, 2, 1, 3)
        q = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        k = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        q = q * sd[pfx + "q_scale"]
        k = k * sd[pfx + "k_scale"]
        sim = torch.einsum("bhid,bjd->bhij", q, k) * spec.attn_scale
        if bias is not None:
            sim = sim + bias
        neg = -torch.finfo(sim.dtype).max
        if key_mask is not None:
            sim = sim.masked_fill(~key_mask[:, None, None, :], neg)
        sim = sim.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), neg)
        attn = sim.softmax(dim=-1) * keep.to(sim.dtype) / (1.0 - p)
        out = torch.einsum("bhij,bjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(b, n, h * dh)
        return F.linear(out, sd[pfx + "to_out.0.weight"]) * keep_o.to(x.dtype) / (1.0 - p)
    return attention


def _relerr(a, b, floor=0.0):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16", "fp16ff"])
@pytest.mark.parametrize("dim,depth,heads", [(128, 2, 2), (1024, 2, 8)])
def test_training_step_with_attn_dropout_matches_oracle_with_the_same_masks(dev, monkeypatch, precision, dim, depth, heads):
    from open_musiclm_amd import engine
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    from test_gpu_model import TOL, grad_unscale
    p = 0.1
    model = _model(dev, precision, p, dim, depth, heads)
    spec = _spec(dim, depth, heads)
    ids = O.synthetic_ids(spec, 2, [2, 30, 20], seed=1234)
    N = O.build_training_inputs(ids, spec)[2].shape[1]
    noise = torch.randn(2, N, generator=torch.Generator().manual_seed(7))
    weights = [0., 0., 1.]
    monkeypatch.setattr(M, "generate_mask_with_prob", lambda shape, p_, device: O.forgetful_mask_from_noise(noise, p_).to(device))
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=weights,
                                                   mask_prob=0.15)
    wrapper.train()
    loss, logits, _ = wrapper(all_token_ids=[t.to(dev) for t in ids], return_loss=True)
    loss.backward()
    state = engine.dropout_state(model.transformer)
    assert state["salt"] is not None
    monkeypatch.setattr(O, "attention", _masked_oracle_attention(O, state, p, 2, dev))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    names = [k for k, _ in model.named_parameters() if ".layers." in k]
    sdo = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
    o_loss, o_logits, _ = O.wrapper_forward_loss(sdo, spec, ids, weights, forget_noise=noise)
    o_grads = dict(zip(names, torch.autograd.grad(o_loss, [sdo[k] for k in names])))
    tol = TOL[precision]
    e_loss = abs(float(loss) - float(o_loss)) / float(o_loss)
    e_logits = _relerr(logits[-1], o_logits[-1])
    params = dict(model.named_parameters())
    gmax = max(float(v.abs().max()) for v in o_grads.values())
    grads = {k: _relerr(params[k].grad * grad_unscale(precision), o_grads[k], floor=1e-3 * gmax) for k in names}
    worst = max(grads.items(), key=lambda kv: kv[1])
    print(f"train_attn_dropout[{precision},{dim}] loss {e_loss:.2e} logits {e_logits:.2e} worst grad {worst}")
    assert e_loss < tol["loss"] and e_logits < tol["logits"], (e_loss, e_logits)
    assert worst[1] < tol["grad"], worst
    # the oracle without the masks is much further off: the dropout really happened, with these masks
    monkeypatch.undo()
    u_loss, u_logits, _ = O.wrapper_forward_loss(sd, spec, ids, weights, forget_noise=noise)
    assert _relerr(u_logits[-1], o_logits[-1]) > 5 * e_logits, (_relerr(u_logits[-1], o_logits[-1]), e_logits)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16", "fp16ff"])
def test_attn_dropout_model_switches(dev, precision):
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    spec = _spec(128, 2, 2)
    ids = [t.to(dev) for t in O.synthetic_ids(spec, 2, [2, 30, 20], seed=1234)]
    m1, m0 = _model(dev, precision, 0.1), _model(dev, precision, 0.0)
    m0.load_state_dict(m1.state_dict())
    w1 = M.TokenConditionedTransformerWrapper(transformer=m1, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0)
    w0 = M.TokenConditionedTransformerWrapper(transformer=m0, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0)
    # eval: no dropout, bit for bit
    w1.eval(); w0.eval()
    with torch.no_grad():
        e1, e0 = w1(all_token_ids=ids, return_loss=False), w0(all_token_ids=ids, return_loss=False)
    assert all(torch.equal(a, b) for a, b in zip(e1, e0))
    torch.manual_seed(5)
    g1 = w1.generate(conditioning_token_ids=ids[:2], max_time_steps=3)
    torch.manual_seed(5)
    g0 = w0.generate(conditioning_token_ids=ids[:2], max_time_steps=3)
    assert torch.equal(g1, g0)
    # train mode under no_grad drops, with a new mask per call
    w1.train(); w0.train()
    with torch.no_grad():
        a = w1(all_token_ids=ids, return_loss=False)[-1].clone()
        b = w1(all_token_ids=ids, return_loss=False)[-1].clone()
        c = w0(all_token_ids=ids, return_loss=False)[-1].clone()
    assert not torch.equal(a, b) and not torch.equal(a, c)
    # .p set after construction is read at the next forward
    for attn, _, _ in m0.transformer.layers:
        attn.attn_dropout.p = 0.2
    with torch.no_grad():
        d = w0(all_token_ids=ids, return_loss=False)[-1].clone()
    assert not torch.equal(d, c)
    for attn, _, _ in m0.transformer.layers:
        attn.attn_dropout.p = 0.0
    with torch.no_grad():
        e = w0(all_token_ids=ids, return_loss=False)[-1].clone()
    assert torch.equal(e, c)


def test_graphed_step_with_attn_dropout_draws_new_masks_and_matches_eager(dev):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.graph import GraphedForwardBackward
    from oracle import musiclm_oracle as O
    model = _model(dev, "fp16ff", 0.1)
    spec = _spec(128, 2, 2)
    ids = [t.to(dev) for t in O.synthetic_ids(spec, 2, [2, 30, 20], seed=1234)]
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.],
                                                   mask_prob=0.0)
    wrapper.train()
    fb = GraphedForwardBackward(lambda a, b, c: wrapper(all_token_ids=[a, b, c], return_loss=True)[0])
    inputs = dict(a=ids[0], b=ids[1], c=ids[2])
    fb.prepare(inputs)
    assert fb.graph is not None, fb.capture_error
    st = model.transformer.__dict__["_omlm_dropout"]
    l1 = float(fb(**inputs)); torch.cuda.synchronize()
    salt1 = int(st["counter"].item())
    l2 = float(fb(**inputs)); torch.cuda.synchronize()
    assert int(st["counter"].item()) == salt1 + 1 and l1 != l2           # every replay bumps the salt: new masks
    st["counter"].fill_(salt1 - 1)                                       # the eager forward takes salt1 again
    le = float(wrapper(all_token_ids=ids, return_loss=True)[0].detach())
    assert abs(le - l1) <= 1e-6 * abs(l1) and abs(l2 - l1) > 100 * abs(le - l1), (le, l1, l2)
