"""GPU: the model at geometries other than the shipped ones, against the CPU oracle (oracle/musiclm_oracle.py).

The full-size tests of test_gpu_model.py run dim 1024 with 8 or 16 heads; the golden models run dim 128 with 2 heads.  Beneath the model the
host and the C ABI choose kernels by geometry -- the fp8-corrected FF GEMMs of "fp16ff" need K % 64 == 0, the plane kernels of the
ConvFeedForward forward Fp <= 4096, the fused rel-pos MLP Hd in {256, 512} and H <= 16, the cached decoder's second-generation step kernels
dim 1024, its matrix-core kernels and the lo planes of "fp16ff" Fp <= 3072, every step kernel H <= 16 -- and each geometry below sits on at
least one of those edges.  Every geometry runs in all four precisions from the same seed; the oracle runs once per geometry.

  (a) a training step (forgetful mask injected from noise): final-sequence logits, loss and gradients of every tensor family;
  (b) teacher-forced KV-cached steps against the oracle's forward of the same sequence, or -- where the decoder cannot serve the geometry --
      a ValueError from CachedDecoder before any launch and decode.supports() False;
  (c) generate(use_cache=True) completes, and in bf16x3 samples the ids of the uncached path;
  (d) decode.max_batch / decode.supports agree with what the library accepts.

Bars are test_gpu_model.TOL's.  Where "fp16ff" legitimately runs a part of the model on the fp16 kernels (Fp > 4096: the feed-forward
forward; a decoder without lo planes: the cached steps), that part is held to the fp16 bar.
"""
import pytest
import torch

from test_gpu_model import RELPOS_TENSORS, TOL, grad_unscale, rel_l2, relerr, report

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16x3", "bf16", "fp16", "fp16ff"]
DEPTH = 2

# id: stage, dim, heads, use_conv_ff, rel-pos type, training lengths (time steps per sequence, B = 2), whether the "fp16ff" cached decoder
# keeps its lo planes (None: the decoder refuses the geometry).  F = 4 dim (plain) or int(8 dim / 3) (conv), Fp = F rounded up to 64.
GEOMETRIES = {
    # F 256: dim % 64 != 0 (the fp8-corrected FF GEMM needs K % 64 == 0), Hd = 48 (layer-by-layer rel-pos MLP), decode D < 16 B
    "A": dict(stage="coarse", dim=96, heads=2, conv=True, relpos="continuous", lens=[1, 40, 60], lo=True),
    # F 554 / Fp 576: dim % 32 != 0, ragged F, H * 64 != dim (dim % 16 != 0 is refused with the continuous rel-pos MLP: its own test below)
    "B": dict(stage="coarse", dim=208, heads=3, conv=True, relpos="continuous", lens=[1, 50, 70], lo=True),
    # F 1365 / Fp 1408: fused rel-pos MLP at Hd = 256, decode at dim < 1024
    "C": dict(stage="fine", dim=512, heads=8, conv=True, relpos="continuous", lens=[1, 30, 30], lo=True),
    # F = Fp = 4096: plain FeedForward at the shipped dim -- Fp at the plane kernels' limit, above the decode lo-plane limit of 3072
    "D": dict(stage="semantic", dim=1024, heads=16, conv=False, relpos="t5", lens=[1, 290], lo=False),
    # F 3413 / Fp 3456: dim > 1024, Fp > 3072, H = 20 > 16 (the decoder's head limit; rel-pos MLP without fusion)
    "E": dict(stage="coarse", dim=1280, heads=20, conv=True, relpos="continuous", lens=[1, 40, 70], lo=None),
    # F 4640 / Fp 4672: Fp > 4096 (past the "fp16ff" plane kernels), dim % 32 != 0, no rel-pos bias
    "F": dict(stage="coarse", dim=1160, heads=5, conv=False, relpos="none", lens=[1, 60, 60], lo=False),
}
GIDS = list(GEOMETRIES)


def _inner(g):
    return 4 * g["dim"] if not g["conv"] else int(2 * g["dim"] * 4 / 3)


def _fp(g):
    return (_inner(g) + 63) // 64 * 64


def _build(gid, precision, dev):
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    g = GEOMETRIES[gid]
    kw = {"coarse": dict(num_coarse_quantizers=3), "fine": dict(num_coarse_quantizers=3, num_fine_quantizers=5), "semantic": {}}[g["stage"]]
    torch.manual_seed(0)                              # same weights in every precision: one oracle per geometry
    model = getattr(M, f"create_{g['stage']}_transformer")(dim=g["dim"], depth=DEPTH, heads=g["heads"], use_conv_ff=g["conv"],
                                                          relative_position_bias_type=g["relpos"], ff_dropout=0.0, precision=precision, **kw)
    spec = getattr(O, f"{g['stage']}_spec")(dim=g["dim"], depth=DEPTH, heads=g["heads"], use_conv_ff=g["conv"],
                                            relative_position_bias_type=g["relpos"])
    assert model.transformer.layers[0][2].inner_dim == _inner(g)
    return model.to(dev), spec


_MODELS = {}


def _eval_model(gid, precision, dev):
    """One eval-mode model per (geometry, precision) for the decode / generate tests (they do not change the weights)."""
    if (gid, precision) not in _MODELS:
        model, spec = _build(gid, precision, dev)
        model.eval()
        _MODELS[(gid, precision)] = (model, spec)
    return _MODELS[(gid, precision)]


def _weights_fingerprint(sd):
    return [float(sd[k].double().sum()) for k in sorted(sd) if k.endswith("to_q.weight") or k.startswith("logit_weights")]


def _grad_names(gid, nseq):
    g = GEOMETRIES[gid]
    ff_in, ff_mid, ff_out = ("1.weight", "4.gamma", "6.weight") if g["conv"] else ("1.weight", "3.gamma", "5.weight")
    names = ["transformer.layers.0.0.to_q.weight", "transformer.layers.1.0.to_kv.weight", "transformer.layers.0.0.to_out.0.weight",
             "transformer.layers.1.0.norm.gamma", "transformer.layers.0.2.0.gamma", f"transformer.layers.1.2.{ff_mid}",
             f"transformer.layers.0.2.{ff_in}", f"transformer.layers.1.2.{ff_in}", f"transformer.layers.1.2.{ff_out}",
             f"transformer.layers.0.2.{ff_out}", "transformer.norm.gamma", f"embeddings.{nseq - 1}.weight", f"logit_weights.{nseq - 1}"]
    if g["conv"]:
        names += ["transformer.layers.0.2.2.ds_conv.weight", "transformer.layers.1.2.2.ds_conv.weight"]
    if g["relpos"] == "continuous":
        names += RELPOS_TENSORS
    elif g["relpos"] == "t5":
        names += ["transformer.rel_pos_bias.relative_attention_bias.weight"]
    return names


_TRAIN_ORACLE = {}


def _train_oracle(gid, model, spec):
    """Oracle loss, logits and gradients of the training step of geometry `gid` (B = 2), computed once per geometry."""
    from oracle import musiclm_oracle as O
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if gid not in _TRAIN_ORACLE:
        g = GEOMETRIES[gid]
        ids = O.synthetic_ids(spec, 2, g["lens"], seed=1234)
        N = O.build_training_inputs(ids, spec)[2].shape[1]
        assert 200 <= N <= 400 and N % 16 != 0, N                    # a ragged sequence: no whole 16-row tile at the end
        noise = torch.randn(2, N, generator=torch.Generator().manual_seed(7))
        nseq = len(ids)
        weights = [0.] * (nseq - 1) + [1.]
        names = _grad_names(gid, nseq)
        sdo = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
        assert all(sdo[k].requires_grad for k in names)
        o_loss, o_logits, _ = O.wrapper_forward_loss(sdo, spec, ids, weights, forget_noise=noise)
        o_grads = dict(zip(names, torch.autograd.grad(o_loss, [sdo[k] for k in names])))
        _TRAIN_ORACLE[gid] = dict(fp=_weights_fingerprint(sd), ids=ids, noise=noise, weights=weights, names=names, loss=float(o_loss.detach()),
                                  logits=o_logits[-1].detach(), grads=o_grads, N=N)
    o = _TRAIN_ORACLE[gid]
    assert _weights_fingerprint(sd) == o["fp"], "the seed no longer gives every precision the same weights"
    return o


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("gid", GIDS)
def test_training_step_vs_oracle(dev, gid, precision):
    """(a) forward + backward of TokenConditionedTransformerWrapper, forgetful mask injected: logits, loss, gradients of every family."""
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    model, spec = _build(gid, precision, dev)
    o = _train_oracle(gid, model, spec)
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
    assert logits[-1].shape == o["logits"].shape
    e_inf, e_l2 = relerr(logits[-1], o["logits"]), rel_l2(logits[-1], o["logits"])
    e_loss = abs(float(loss) - o["loss"]) / o["loss"]
    params = dict(model.named_parameters())
    gmax = max(float(v.abs().max()) for v in o["grads"].values())
    # rel-pos MLP biases: near-invariant directions of the softmax, judged against 1e-2 of the largest gradient (test_gpu_model's floor)
    grads = {k: relerr(params[k].grad * grad_unscale(precision), o["grads"][k],
                       floor=1e-2 * gmax if (k in RELPOS_TENSORS and k.endswith("bias")) else 0.0) for k in o["names"]}
    # the causal T5 table: the reference maps every visible key to bucket 0, so its gradient is analytically zero (a per-head constant cancels
    # in the softmax) -- rounding noise on both sides, bounded against 1e-3 of the largest gradient by TOL's `invariant` bar, as the golden test does
    invariant = {k: relerr(params[k].grad * grad_unscale(precision), o["grads"][k], floor=1e-3 * gmax)
                 for k in o["names"] if k.endswith("relative_attention_bias.weight")}
    for k in invariant:
        grads.pop(k)
    worst = max(grads.items(), key=lambda kv: kv[1])
    g = GEOMETRIES[gid]
    # "fp16ff" past the plane kernels' Fp <= 4096: the feed-forward forward runs on the fp16 kernels, and is held to the fp16 bar
    tol = TOL["fp16"] if (precision == "fp16ff" and _fp(g) > 4096) else TOL[precision]
    report(f"geometry_train[{gid},{precision}]", dim=g["dim"], heads=g["heads"], Fp=_fp(g), N=o["N"], logits_inf=e_inf, logits_l2=e_l2,
           loss=e_loss, worst_grad=worst, grads=grads, invariant=invariant)
    assert e_inf < tol["logits"], (e_inf, e_l2)
    assert e_loss < tol["loss"], e_loss
    assert worst[1] < tol["grad"], grads
    assert all(v < tol["invariant"] for v in invariant.values()), invariant


def test_continuous_relpos_refuses_dim_not_multiple_of_16():
    """dim % 16 != 0 with the continuous rel-pos bias: the MLP's width dim / 2 is not a whole number of 8-element GEMM rows -- refused when
    the model is built, with the limit named, instead of an argument error inside the first forward."""
    from open_musiclm_amd import open_musiclm as M
    with pytest.raises(ValueError, match="dim % 16"):
        M.create_coarse_transformer(dim=200, depth=1, heads=3, num_coarse_quantizers=3)
    for rp in ("t5", "none"):                          # the other bias types have no MLP: dim % 8 == 0 is enough
        M.create_coarse_transformer(dim=200, depth=1, heads=3, num_coarse_quantizers=3, relative_position_bias_type=rp)


# ---- (b) cached decode ---------------------------------------------------------------------------------------------------------------
DECODE_BATCHES = {"bf16x3": [1, 3], "bf16": [1, 2, 8], "fp16": [1, 2, 8], "fp16ff": [1, 2, 8]}
DECODE_CASES = [(gid, p, b) for gid in GIDS for p in PRECISIONS for b in DECODE_BATCHES[p]]
DEC_SAMPLES, DEC_N0, DEC_STEPS = 8, 4, 8
_DECODE_ORACLE = {}


def _decode_inputs(gid, model, spec):
    """Prompt (conditioning sequences with eos + DEC_N0 known ids of the predicted sequence) and DEC_STEPS teacher-forced ids for
    DEC_SAMPLES samples, and the oracle's final-sequence logits of the whole sequence (row j predicts id j): once per geometry."""
    from oracle import musiclm_oracle as O
    from open_musiclm_amd.utils import append_eos_id
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if gid not in _DECODE_ORACLE:
        gen = torch.Generator().manual_seed(11)
        seqs = spec.token_sequences
        cond_steps = [1, 9][:len(seqs) - 1]
        cond = [torch.randint(0, s.codebook_size, (DEC_SAMPLES, t, s.num_quantizers) if s.num_quantizers > 1 else (DEC_SAMPLES, t),
                              generator=gen) for s, t in zip(seqs[:-1], cond_steps)]
        condx = [append_eos_id(t.reshape(DEC_SAMPLES, -1).long(), e) for t, e in zip(cond, spec.eos_ids)]
        flat = torch.randint(0, seqs[-1].codebook_size, (DEC_SAMPLES, DEC_N0 + DEC_STEPS), generator=gen)
        with torch.no_grad():
            o = O.token_conditioned_forward(sd, spec, condx + [flat[:, :DEC_N0 + DEC_STEPS - 1]], only_final=True)[-1]
        rows = sum(t.shape[-1] + 1 for t in condx) + 1 + DEC_N0 + DEC_STEPS
        _DECODE_ORACLE[gid] = dict(fp=_weights_fingerprint(sd), cond=cond, condx=condx, flat=flat, logits=o.detach(), rows=rows,
                                   V1=seqs[-1].codebook_size + 1)
    d = _DECODE_ORACLE[gid]
    assert _weights_fingerprint(sd) == d["fp"]
    return d


def _poison_small_blocks(dev):
    """Hand the caching allocator a few hundred freed small blocks full of 0x7f7f7f7f: a zeroed allocation shorter than what a kernel reads
    then meets non-zero words behind its end (a split-K arrival counter that is too short never sees its combine fire)."""
    junk = [torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device=dev) for n in (1, 2, 4, 6, 8, 12, 16, 32, 64, 100) * 40]
    torch.cuda.synchronize(dev)
    del junk


@pytest.mark.parametrize("gid,precision,B", DECODE_CASES)
def test_cached_steps_vs_oracle(dev, gid, precision, B):
    """(b) prefill + DEC_STEPS teacher-forced cached steps, each against the oracle's forward of the same sequence."""
    from open_musiclm_amd import decode
    model, spec = _eval_model(gid, precision, dev)
    d = _decode_inputs(gid, model, spec)
    g = GEOMETRIES[gid]
    if g["lo"] is None:
        # the step kernels hold at most 16 heads: the decoder refuses before any launch, generate() takes the uncached path
        assert not decode.supports(model, B, precision) and not decode.supports(model, 1)
        with pytest.raises(ValueError):
            decode.CachedDecoder(model, B, d["rows"], precision)
        report(f"geometry_decode[{gid},{precision},B={B}]", refused=True)
        return
    assert decode.supports(model, B, precision)
    if gid == "A" and B == 8:
        _poison_small_blocks(dev)
    with torch.no_grad():
        dec = decode.CachedDecoder(model, B, d["rows"], precision)
        if precision == "fp16ff":
            assert dec.planes == g["lo"], (dec.planes, g["lo"])
        flat = d["flat"][:B].to(dev)
        got = [dec.prefill([t[:B].to(dev) for t in d["condx"]] + [flat[:, :DEC_N0]]).clone()]
        for k in range(DEC_N0, DEC_N0 + DEC_STEPS - 1):
            got.append(dec.step(flat[:, k].contiguous(), k).clone())
        torch.cuda.synchronize(dev)
    V1 = d["V1"]
    errs = [relerr(lg[:, :V1], d["logits"][:B, DEC_N0 + i]) for i, lg in enumerate(got)]
    # a decoder of "fp16ff" without lo planes runs its steps on the fp16 kernels: the fp16 bar
    bar = TOL["fp16" if (precision == "fp16ff" and not dec.planes) else precision]["logits"]
    report(f"geometry_decode[{gid},{precision},B={B}]", max_rel_err=max(errs), prefill=errs[0], lo_planes=bool(dec.planes), steps=len(errs))
    assert max(errs) < bar, errs


# ---- (c) generate() routing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("gid", GIDS)
def test_generate_with_cache_completes(dev, gid, precision):
    """(c) generate(use_cache=True) takes a route that exists for the geometry; in bf16x3 it samples the ids of the uncached re-forward."""
    from open_musiclm_amd import open_musiclm as M
    model, spec = _eval_model(gid, precision, dev)
    d = _decode_inputs(gid, model, spec)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    Q = spec.token_sequences[-1].num_quantizers
    steps = max(6 // Q, 2)
    U = torch.rand(steps * Q, 2, d["V1"], generator=torch.Generator().manual_seed(5))
    kw = dict(conditioning_token_ids=[t[:2].to(dev) for t in d["cond"]], max_time_steps=steps, uniforms=U)
    a = wrapper.generate(use_cache=True, **kw)
    assert a.shape == (2, steps, Q)
    assert bool(((a >= 0) & (a < d["V1"] - 1)).all()), a
    if precision == "bf16x3":
        b = wrapper.generate(use_cache=False, **kw)
        assert torch.equal(a, b), (a.tolist(), b.tolist())


# ---- (d) the Python mirror of the decoder's eligibility --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("gid", GIDS)
def test_decode_supports_mirrors_the_library(dev, gid, precision):
    """(d) every batch size decode.supports() allows builds a CachedDecoder that prefills and steps without a library error; one sample
    more than decode.max_batch() is not supported; a geometry it refuses raises ValueError in CachedDecoder before any launch."""
    from open_musiclm_amd import decode
    model, spec = _eval_model(gid, precision, dev)
    d = _decode_inputs(gid, model, spec)
    mb = decode.max_batch(model, precision)
    assert not decode.supports(model, mb + 1, precision)
    allowed = [b for b in range(1, mb + 1) if decode.supports(model, b, precision)]
    if not allowed:
        assert GEOMETRIES[gid]["lo"] is None
        with pytest.raises(ValueError):
            decode.CachedDecoder(model, 1, d["rows"], precision)
        return
    assert allowed == list(range(1, mb + 1)), allowed
    for B in sorted({1, 2, mb}):
        reps = (B + DEC_SAMPLES - 1) // DEC_SAMPLES
        flat = d["flat"].repeat(reps, 1)[:B].to(dev)
        with torch.no_grad():
            dec = decode.CachedDecoder(model, B, d["rows"], precision)
            dec.prefill([t.repeat(reps, 1)[:B].to(dev) for t in d["condx"]] + [flat[:, :DEC_N0]])
            lg = dec.step(flat[:, DEC_N0].contiguous(), DEC_N0)
            torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(lg[:, :d["V1"]]).all()), (B, mb)


# ---- (e) a refused step launches nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id,emb,ln", [("refused/late: lo planes B=2 L=0 no ln_parts, emb_table", True, False),
                                           ("refused/lo planes head without partials L=0", False, True)])
def test_refused_step_leaves_x_untouched(dev, row_id, emb, ln):
    """(e) omlm_decode_step at D = 1024, B = 2, L = 0, H = 2, Fp = 64, V1 = 17 with head_W and all three lo-plane pointers.  With an embedding
    table and no ln_parts the lo planes are refused (B >= 2 needs the matrix-core kernels' partials) -- by the commit the route table was
    recorded from only AFTER the embedding gather had overwritten x; with ln_parts and no table the head misses its LayerNorm partials.
    Both are argument refusals with that commit's return code and message (tests/decode_routes.json), and x still holds its sentinel."""
    import ctypes as C
    import json
    import os
    from open_musiclm_amd import decode, hip
    table = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_routes.json")))
    row = next(r for r in table["rows"] if r["id"] == row_id)
    B, D, H, Fp, V1 = 2, 1024, 2, 64, 17
    assert (row["B"], row["D"], row["L"], row["H"], row["Fp"], row["V1"], row["emb"], row["ln"], row["lo"]) == (B, D, 0, H, Fp, V1, emb, ln, "all")
    z = lambda *s, t=torch.float32: torch.zeros(*s, dtype=t, device=dev)
    x = torch.full((B, D), 7.25, device=dev)
    t = dict(pos_dev=z(1, t=torch.int32), parts=z(B, 1, H, 66), head_W=z(V1, D, t=torch.float16), head_W_lo=z(V1, D, t=torch.float16),
             emb=z(32, D), logits=z(B, 24), ids=z(B, t=torch.int64), x1=z(B, D), q=z(B, H * 64), u=z(B, Fp), adv=z(1, t=torch.int32),
             ln=z(decode.scratch_sizes(B, D, Fp)["ln_parts"]), lo=z(8, t=torch.float16))
    planes = (C.c_void_p * 1)(t["lo"].data_ptr())              # L = 0: no layer reads its planes
    a = decode.DecodeArgs()
    a.B, a.D, a.H, a.L, a.F, a.Fp, a.Nmax, a.nsplit, a.w_dtype, a.round_bf16 = B, D, H, 0, Fp, Fp, 64, 1, 2, 1
    a.eps, a.scale, a.V1, a.ldV, a.emb_rows = 1e-5, 8.0, V1, 24, 32
    a.pos_dev, a.parts, a.head_W, a.head_W_lo, a.logits = (t[n].data_ptr() for n in ("pos_dev", "parts", "head_W", "head_W_lo", "logits"))
    a.x, a.x1, a.q, a.u, a.advance_pos = x.data_ptr(), t["x1"].data_ptr(), t["q"].data_ptr(), t["u"].data_ptr(), t["adv"].data_ptr()
    a.W1p_lo = a.W2p_lo = C.cast(planes, C.POINTER(C.c_void_p))
    a.emb_table = t["emb"].data_ptr() if emb else None
    a.ln_parts = t["ln"].data_ptr() if ln else None
    torch.cuda.synchronize(dev)
    rc = hip.lib().omlm_decode_step(C.addressof(a), t["ids"].data_ptr(), hip.stream_ptr())
    msg = hip.lib().omlm_last_error().decode()
    torch.cuda.synchronize(dev)
    assert (rc, msg) == (row["refused"]["rc"], row["refused"]["message"])
    assert bool((x == 7.25).all()) and int(t["adv"].item()) == 0 and not bool(t["logits"].any())
