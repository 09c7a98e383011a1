"""Non-causal prefix (non_causal_prefix_size = P > 0) on the GPU.

  (1) the attention entries with P >= 1 against fp64 torch with the same mask and bias, fp32 / bf16 / fp16 operands, with and without a key
      mask, continuous / t5 / no bias, once with dropout (the keep-mask of omlm_attn_dropout_keep): out, lse, dQ, dK, dV and d(bias),
      the negative-distance rows included;
  (2) the prefix is really non-causal: the id at row P - 1 moves the logits of row 0, and at P = 0 it does not;
  (3) the model against the oracle: eval logits in all four precisions, one training step (loss, gradients incl. the rel-pos MLP and the
      T5 rows), at a geometry other than the shipped ones;
  (4) generate: cached (P <= prompt rows) against oracle.generate and against the uncached path, and P > prompt rows (re-forward route).
"""
import pytest
import torch

from test_gpu_model import RELPOS_TENSORS, TOL, grad_unscale, rel_l2, relerr, report

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16x3", "bf16", "fp16", "fp16ff"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from open_musiclm_amd import ops as o
    return o


# ---- (1) kernels -------------------------------------------------------------------------------------------------------------------------
def prefix_attention(q, k, v, table, keymask, H, P, keep=None, p=0.0, scale=8.0):
    """fp64 reference.  table [N + Pn - 1, ld] (row = i - j + Pn - 1) or None; live iff j <= i or (i < P and j < P), and the key mask."""
    B, N, _ = q.shape
    Pn = min(P, N)
    qh = q.view(B, N, H, 64).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bjd->bhij", qh, k) * scale
    ar = torch.arange(N, device=q.device)
    rel = ar[:, None] - ar[None, :]
    if table is not None:
        sim = sim + table[:, :H].t()[:, (rel + Pn - 1).clamp(min=0)]
    live = (rel >= 0) | ((ar[:, None] < P) & (ar[None, :] < P))
    neg = -torch.finfo(torch.float32).max
    sim = sim.masked_fill(~live, neg)
    if keymask is not None:
        sim = sim.masked_fill(~keymask[:, None, None, :], neg)
    attn = sim.softmax(-1)
    if keep is not None:
        attn = attn * keep.to(attn.dtype) / (1.0 - p)
    return torch.einsum("bhij,bjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(B, N, H * 64), \
        torch.logsumexp(sim, -1) / torch.log(torch.tensor(2.0, dtype=sim.dtype))


def _table(kind, rows, x0, H, g):
    ldb = (H + 7) // 8 * 8
    if kind == "none":
        return None
    t = torch.zeros(rows, ldb)
    if kind == "continuous":
        t[:, :H] = torch.randn(rows, H, generator=g) * 2
    else:                                                  # t5: one value per bucket of the distance (bucket 0 for every past key)
        from open_musiclm_amd.transformer import t5_bucket_of_distance
        emb = torch.randn(32, H, generator=g) * 2
        t[:, :H] = emb[t5_bucket_of_distance(torch.arange(x0, x0 + rows))]
    return t


def _kernel_case(ops, dev, dtype, B, N, H, P, kind, masked, p=0.0, form="raw"):
    """form: "raw" (the plain table: the first-generation kernels), "fixed" / "online" (the table prepared by AttnBias.group(..., P=P): for
    16-bit operands the second-generation kernels, with the fixed reference point or -- a bound too loose for it -- the online softmax)."""
    from open_musiclm_amd.engine import relpos_rows
    g = torch.Generator().manual_seed(N * 131 + P * 7 + H)
    M = B * N
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    q = unit(torch.randn(B, N, H, 64, generator=g)).reshape(M, H * 64).to(dev, dtype)
    k = unit(torch.randn(M, 64, generator=g)).to(dev, dtype)
    v = torch.randn(M, 64, generator=g).to(dev, dtype)
    rows, x0 = relpos_rows(N, P)
    table = _table(kind, rows, x0, H, g)
    table = table.to(dev) if table is not None else None
    if table is not None and form == "fixed" and dtype == torch.float16:
        table = table * 0.1              # half's fixed form needs 2 c bound + the table's range < 28 octaves (omlm_attn_bias_prepare)
    keymask = None
    if masked:
        keymask = torch.rand(B, N, generator=g) > 0.2
        keymask[:, 0] = True
        keymask = keymask.to(dev)
    km8 = keymask.to(torch.uint8) if keymask is not None else None
    seed, salt = 0xBEEF + N, torch.tensor([5], dtype=torch.int64, device=dev)
    keep = ops.attn_dropout_keep(B, N, H, p, seed, seed_dev=salt, device=dev).bool() if p > 0 else None
    qr = q.double().view(B, N, -1).requires_grad_(True)
    kr = k.double().view(B, N, 64).requires_grad_(True)
    vr = v.double().view(B, N, 64).requires_grad_(True)
    tr_ = table.double().requires_grad_(True) if table is not None else None
    ref, ref_lse = prefix_attention(qr, kr, vr, tr_, keymask, H, P, keep, p)
    do = torch.randn(B, N, H * 64, generator=g).to(dev)
    ref.backward(do.double())
    ab = table
    if form != "raw":
        bound = torch.full((64,), 1.0 if form == "fixed" else 3.0, device=dev)          # |q.k| <= 1 <= 9: both are valid bounds
        ab = ops.AttnBias.group(table, N, H, dev, [bound], [bound], half=dtype == torch.float16, P=P)[0]
        ldT = ab.tableT.numel() // ((H + 7) // 8 * 8)
        tail = ab.tableT.view(-1, ldT)[:H]
        assert bool((tail[:, -2] == 1.0).all()) == (form == "fixed"), "the bound did not select the intended softmax form"
    out = torch.empty(M, H * 64, device=dev, dtype=dtype)
    lse = torch.empty(B, H, N, device=dev)
    ops.attn_fwd(q, k, v, ab, km8, out, lse, B, N, H, 8.0, P=P, p=p, seed=seed, seed_dev=salt if p > 0 else None)
    dq = torch.empty(M, H * 64, device=dev)
    dk = torch.empty(M, 64, device=dev)
    dv = torch.empty(M, 64, device=dev)
    delta = torch.empty(B, H, N, device=dev)
    dtab = torch.zeros_like(table) if table is not None else None
    ops.attn_bwd(q, k, v, ab, km8, out, do.reshape(M, -1).to(dtype), lse, delta, dq, dk, dv, dtab, B, N, H, 8.0, P=P,
                 p=p, seed=seed, seed_dev=salt if p > 0 else None)
    torch.cuda.synchronize()
    errs = dict(fwd=relerr(out.view(B, N, -1), ref), lse=float((lse.double().cpu() - ref_lse.detach().cpu()).abs().max()),
                dq=relerr(dq.view(B, N, -1), qr.grad), dk=relerr(dk.view(B, N, -1), kr.grad), dv=relerr(dv.view(B, N, -1), vr.grad))
    if table is not None:
        Pn = min(P, N)
        errs["dbias"] = relerr(dtab[:, :H], tr_.grad[:, :H])
        if Pn > 1:                                                     # the negative-distance rows on their own
            errs["dbias_neg"] = relerr(dtab[:Pn - 1, :H], tr_.grad[:Pn - 1, :H], floor=float(tr_.grad[:, :H].abs().max()))
    # the dropout tests' bars, fp32's forward at 5e-5: bias entries of size 2 over up to N + P keys (measured 2.1e-5)
    tol_f = 5e-5 if dtype == torch.float32 else (1e-2 if dtype == torch.bfloat16 else 2e-3)
    tol_b = 4e-3 if dtype == torch.float16 else 2e-2
    tol_lse = 1e-4 if dtype == torch.float32 else 1e-2                  # log2 units: 0.7 % of the denominator in 16 bits
    name = f"prefix_kernel[{dtype},{B},{N},{H},P={P},{kind},mask={masked},p={p},{form}]"
    print(name, {k_: f"{v_:.2e}" for k_, v_ in errs.items()})
    assert errs["fwd"] < tol_f, (name, errs)
    assert errs["lse"] < tol_lse, (name, errs)
    assert max(v_ for k_, v_ in errs.items() if k_ not in ("fwd", "lse")) < tol_b, (name, errs)


KINDS = ["continuous", "t5", "none"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
FORMS = {torch.float32: ["raw", "fixed"], torch.bfloat16: ["raw", "fixed", "online"], torch.float16: ["raw", "fixed", "online"]}


@pytest.mark.parametrize("P", [1, 31, 32, 33, 65, 76, 77, 82])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_kernels_n77(ops, dev, dtype, P):
    for form in FORMS[dtype]:
        for i, kind in enumerate(KINDS):
            _kernel_case(ops, dev, dtype, 2, 77, 8, P, kind, masked=(i + P) % 2 == 0, form=form)


@pytest.mark.parametrize("P", [1, 33, 216, 1115, 1116, 1121])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_kernels_n1116(ops, dev, dtype, P):
    kind = KINDS[P % 3]
    for form in FORMS[dtype]:
        _kernel_case(ops, dev, dtype, 1, 1116, 16 if P % 2 else 8, P, kind, masked=P % 2 == 0, form=form)


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_kernels_with_dropout(ops, dev, dtype):
    for form in FORMS[dtype]:
        _kernel_case(ops, dev, dtype, 2, 77, 8, 33, "continuous", masked=True, p=0.1, form=form)
        _kernel_case(ops, dev, dtype, 1, 300, 8, 216, "t5", masked=False, p=0.1, form=form)


# ---- model helpers -------------------------------------------------------------------------------------------------------------------------
def _build(dev, precision, P, relpos="continuous", dim=208, heads=3, stage="coarse"):
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    kw = {"coarse": dict(num_coarse_quantizers=3), "semantic": {}}[stage]
    torch.manual_seed(0)
    model = getattr(M, f"create_{stage}_transformer")(dim=dim, depth=2, heads=heads, relative_position_bias_type=relpos, ff_dropout=0.0,
                                                      non_causal_prefix_size=P, precision=precision, **kw).to(dev)
    spec = getattr(O, f"{stage}_spec")(dim=dim, depth=2, heads=heads, relative_position_bias_type=relpos, non_causal_prefix_size=P)
    return model, spec


# ---- (2) non-causality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 13])
def test_prefix_row_moves_row_zero(dev, P):
    from oracle import musiclm_oracle as O
    model, spec = _build(dev, "bf16x3", P, stage="semantic", dim=128, heads=2)
    model.eval()
    ids = O.synthetic_ids(spec, 1, [1, 20], seed=3)                   # rows: start, 12 CLAP ids, start, 20 semantic ids
    ids2 = [t.clone() for t in ids]
    ids2[0][0, 0, 11] = (ids2[0][0, 0, 11] + 1) % spec.token_sequences[0].codebook_size      # the last CLAP id: row 12 = P - 1
    with torch.no_grad():
        a = model(all_token_ids=[t.to(dev) for t in ids])
        b = model(all_token_ids=[t.to(dev) for t in ids2])
    d0 = float((a[0][:, 0] - b[0][:, 0]).abs().max())
    if P == 0:
        assert d0 == 0.0, d0
    else:
        assert d0 > 1e-4, d0


# ---- (3) the model against the oracle -----------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_train(key, model, spec, lens):
    from oracle import musiclm_oracle as O
    if key not in _ORACLE:
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ids = O.synthetic_ids(spec, 2, lens, seed=1234)
        N = O.build_training_inputs(ids, spec)[2].shape[1]
        noise = torch.randn(2, N, generator=torch.Generator().manual_seed(7))
        nseq = len(ids)
        weights = [0.] * (nseq - 1) + [1.]
        names = ["transformer.layers.0.0.to_q.weight", "transformer.layers.1.0.to_kv.weight", "transformer.layers.0.0.to_out.0.weight",
                 "transformer.norm.gamma", f"embeddings.{nseq - 1}.weight", f"logit_weights.{nseq - 1}", "start_tokens.0"]
        names += RELPOS_TENSORS if spec.relative_position_bias_type == "continuous" else ["transformer.rel_pos_bias.relative_attention_bias.weight"]
        sdo = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
        o_loss, o_logits, _ = O.wrapper_forward_loss(sdo, spec, ids, weights, forget_noise=noise)
        grads = dict(zip(names, torch.autograd.grad(o_loss, [sdo[k] for k in names])))
        with torch.no_grad():
            ev = O.token_conditioned_forward(sd, spec, ids, None)
        _ORACLE[key] = dict(ids=ids, noise=noise, weights=weights, names=names, loss=float(o_loss.detach()), grads=grads, eval=ev, N=N)
    return _ORACLE[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("relpos,P", [("continuous", 37), ("t5", 90), ("continuous", 500)])
def test_model_vs_oracle(dev, precision, relpos, P):
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    model, spec = _build(dev, precision, P, relpos=relpos)
    o = _oracle_train((relpos, P), model, spec, [1, 50, 70])
    # eval logits of every sequence
    model.eval()
    with torch.no_grad():
        ev = model(all_token_ids=[t.to(dev) for t in o["ids"]])
    e_eval = max(relerr(a, b) for a, b in zip(ev, o["eval"]))
    # one training step, forgetful mask injected
    model.train()
    import open_musiclm_amd.open_musiclm as MM
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
    e_loss = abs(float(loss.detach()) - o["loss"]) / o["loss"]
    params = dict(model.named_parameters())
    gmax = max(float(v.abs().max()) for v in o["grads"].values())
    grads = {k: relerr(params[k].grad * grad_unscale(precision), o["grads"][k],
                       floor=1e-2 * gmax if (k in RELPOS_TENSORS and k.endswith("bias")) else 0.0) for k in o["names"]}
    worst = max(grads.items(), key=lambda kv: kv[1])
    tol = TOL[precision]
    report(f"prefix_model[{relpos},P={P},{precision}]", N=o["N"], eval_logits=e_eval, loss=e_loss, worst_grad=worst, grads=grads)
    assert e_eval < tol["logits"], e_eval
    assert e_loss < tol["loss"], e_loss
    assert worst[1] < tol["grad"], grads
    if relpos == "t5":                       # buckets 1 .. 31 are live inside the prefix: a real, non-zero gradient
        g = o["grads"]["transformer.rel_pos_bias.relative_attention_bias.weight"]
        assert float(g[1:].abs().max()) > 1e-3 * gmax


# ---- (4) generate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relpos,P", [("continuous", 14), ("t5", 40)])
def test_generate_cached_vs_oracle(dev, relpos, P):
    from open_musiclm_amd import decode
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    model, spec = _build(dev, "bf16x3", P, relpos=relpos, stage="semantic", dim=128, heads=2)
    model.eval()
    cond = O.synthetic_ids(spec, 2, [1], seed=9)                      # start, 12 CLAP ids, eos, start: 15 prompt rows
    prompt_rows = 15
    assert decode.supports(model, 1, prompt_rows=prompt_rows) == (P <= prompt_rows)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    V1 = spec.token_sequences[-1].codebook_size + 1
    steps = 5
    U = torch.rand(steps, 2, V1, generator=torch.Generator().manual_seed(5))
    kw = dict(conditioning_token_ids=[t.to(dev) for t in cond], max_time_steps=steps, uniforms=U)
    a = wrapper.generate(use_cache=True, **kw)
    b = wrapper.generate(use_cache=False, **kw)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    o = O.generate(sd, spec, cond, steps, U)
    assert torch.equal(a.cpu(), b.cpu()), (a.tolist(), b.tolist())
    assert torch.equal(a.cpu(), o), (a.tolist(), o.tolist())


def test_prefill_refuses_short_prompt(dev):
    from open_musiclm_amd import decode
    from oracle import musiclm_oracle as O
    model, spec = _build(dev, "bf16", 30, stage="semantic", dim=128, heads=2)
    model.eval()
    cond = O.synthetic_ids(spec, 1, [1], seed=9)
    dec = decode.CachedDecoder(model, 1, 40, "bf16")
    with pytest.raises(ValueError):                                   # 15 prompt rows, P = 30
        dec.prefill([torch.cat([cond[0].reshape(1, -1), torch.tensor([[spec.token_sequences[0].codebook_size]])], dim=1).to(dev),
                     torch.empty(1, 0, dtype=torch.long, device=dev)])
