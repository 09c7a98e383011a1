"""GPU: the last layer's feed-forward block on the live rows only (engine.live_rows; the rule itself: test_live_rows_host.py).

Kernels, at d = 1024 (the row-pair LayerNorm kernels) and d = 512 (the general ones), B = 2, N = 40, p0 = 8 -- more than one sample, the
segment starting and ending on either parity of the row-pair walk:
  * the gathering LayerNorm forwards (plain, hi/lo planes, fp8 planes) are bit-equal to the plain entry run on a gathered copy of the input,
    and their second output is that gathered copy;
  * the scattering LayerNorm backward is bit-equal, on the segment's rows, to the plain backward run on the compact inputs, writes exact
    zeros to every row in front of the segment (the destination is NaN-filled first) and leaves bit-equal d(gamma) partial rows;
  * the ConvFeedForward forward with a segment draws the keep bits of the full launch, and everything from the third row of a sample on is
    bit-equal to the full launch; the backward on the compact buffers gives the full launch's dh1.
Model (dim 1024, depth 2, heads 8, layout lens [13, 20, 59], B = 2; "fp16ff" and "bf16"), the hook on (default) against OMLM_LIVE_ROWS=0:
loss / wanted logits inside test_gpu_model.TOL against the oracle in fp64; per parameter tensor the gradient error against the oracle with
the hook on is at most 1.25 x the error with it off (the 25 %: the changed fp32 summation order of the last layer's dW1 / dW2 and the GEMMs'
peeled tails at the other row count, random in sign); with ff_dropout = 0.1 on and off draw the same masks, so they agree as closely as at
p = 0 (twice the p = 0 figure); one captured-graph step runs with the hook on.
"""
import os

import pytest
import torch

from test_gpu_model import RELPOS_TENSORS, TOL, grad_unscale, relerr, report

pytestmark = pytest.mark.gpu

B, N, P0 = 2, 40, 8
SEG = (N, P0, N - P0)
H16 = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from open_musiclm_amd import ops as _ops
    return _ops


def _idx(dev):
    from open_musiclm_amd import engine
    return engine.live_to_full(torch.arange(B * SEG[2]), SEG).to(dev)


def bits(t):
    """The tensor's bytes (bit equality, NaN-safe)."""
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", H16)
@pytest.mark.parametrize("D", [1024, 512])
def test_gather_layernorm_forward_plain_and_planes(ops, dev, D, T):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(B * N, D, generator=g) * 3 + 0.5).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    idx = _idx(dev)
    xg = x[idx].contiguous()
    M = xg.shape[0]
    new = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device=dev)
    # plain
    y0, m0, r0 = new(M, D, dt=T), new(M), new(M)
    ops.layernorm_fwd(xg, gamma, y0, None, m0, r0)
    y1, m1, r1, xc = new(M, D, dt=T), new(M), new(M), new(M, D)
    ops.layernorm_fwd(x, gamma, y1, None, m1, r1, seg=SEG, xc=xc)
    assert same(y0, y1) and same(m0, m1) and same(r0, r1) and same(xc, xg)
    y2, m2, r2 = new(M, D, dt=T), new(M), new(M)
    ops.layernorm_fwd(x, gamma, y2, None, m2, r2, seg=SEG)                    # the second output is optional
    assert same(y0, y2) and same(m0, m2) and same(r0, r2)
    # hi / lo planes
    y0, l0, m0, r0 = new(M, D, dt=T), new(M, D, dt=T), new(M), new(M)
    ops.layernorm_fwd_planes(xg, gamma, y0, l0, m0, r0)
    y1, l1, m1, r1, xc = new(M, D, dt=T), new(M, D, dt=T), new(M), new(M), new(M, D)
    ops.layernorm_fwd_planes(x, gamma, y1, l1, m1, r1, seg=SEG, xc=xc)
    assert same(y0, y1) and same(l0, l1) and same(m0, m1) and same(r0, r1) and same(xc, xg)
    assert not torch.isnan(y1.float()).any() and not torch.isnan(l1.float()).any()


@pytest.mark.parametrize("D", [1024, 512])
def test_gather_layernorm_forward_mx(ops, dev, D):
    g = torch.Generator().manual_seed(D + 1)
    x = (torch.randn(B * N, D, generator=g) * 3 + 0.5).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    xg = x[_idx(dev)].contiguous()
    M = xg.shape[0]
    out = []
    for src, kw in ((xg, {}), (x, dict(seg=SEG, xc=torch.full((M, D), float("nan"), device=dev)))):
        y = torch.full((M, D), float("nan"), dtype=torch.float16, device=dev)
        m, r = torch.full((M,), float("nan"), device=dev), torch.full((M,), float("nan"), device=dev)
        P = ops.Fp8Planes(M, D, dev, zero=True)
        ops.layernorm_fwd_mx(src, gamma, y, P, m, r, **kw)
        out.append((y, m, r, P.planes[:, :M], P.scale[:M], kw.get("xc")))
    for a, b in zip(out[0][:5], out[1][:5]):
        assert same(a, b)
    assert same(out[1][5], xg)


@pytest.mark.parametrize("T", H16)
@pytest.mark.parametrize("D", [1024, 512])
def test_scatter_layernorm_backward(ops, dev, D, T):
    g = torch.Generator().manual_seed(D + 2)
    M, Mf = B * SEG[2], B * N
    x = (torch.randn(M, D, generator=g) * 2 - 0.3).to(dev)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(dev)
    dy = torch.randn(M, D, generator=g).to(dev).to(T)
    dres = torch.randn(M, D, generator=g).to(dev)
    y, mean, rstd = torch.empty(M, D, dtype=T, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev)
    ops.layernorm_fwd(x, gamma, y, None, mean, rstd)
    idx = _idx(dev)
    dead = torch.ones(Mf, dtype=torch.bool, device=dev)
    dead[idx] = False
    assert int(dead.sum()) == B * P0
    for with_dres in (True, False):
        for with_cast in (True, False):
            d = dres if with_dres else None
            dx0 = torch.full((M, D), float("nan"), device=dev)
            dc0 = torch.full((M, D), float("nan"), dtype=T, device=dev) if with_cast else None
            dg0, cg0 = torch.zeros(D, device=dev), ops.ColsumGroup()
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, d, dx0, dc0, dg0, defer=cg0)
            dx1 = torch.full((Mf, D), float("nan"), device=dev)
            dc1 = torch.full((Mf, D), float("nan"), dtype=T, device=dev) if with_cast else None
            dg1, cg1 = torch.zeros(D, device=dev), ops.ColsumGroup()
            ops.layernorm_bwd(dy, x, gamma, mean, rstd, d, dx1, dc1, dg1, defer=cg1, seg=SEG)
            assert same(dx1[idx], dx0), (D, T, with_dres, with_cast)
            assert same(dx1[dead], torch.zeros(B * P0, D, device=dev))
            if with_cast:
                assert same(dc1[idx], dc0) and same(dc1[dead], torch.zeros(B * P0, D, dtype=T, device=dev))
            # d(gamma): what the kernel leaves is one partial row per workgroup, and those are bit-equal.  The column sum behind them
            # (omlm_colsum_group, not part of this change) adds its 16 slices with atomics in whatever order they arrive, so the summed
            # d(gamma) of ANY two launches agrees to fp32 re-association only: checked against the fp64 sum of the partial rows
            part0, part1 = cg0.items[0][0], cg1.items[0][0]
            assert same(part0, part1) and part0.numel() == M * D
            cg0.flush(); cg1.flush()
            ref = part0.view(M, D).double().sum(0)
            bar = (M - 1) * 2.0 ** -24 * float(part0.view(M, D).double().abs().sum(0).max())     # fp32 sum of M terms in any order: (M - 1) u sum|x|
            assert float((dg0.double() - ref).abs().max()) <= bar
            assert float((dg1.double() - ref).abs().max()) <= bar
    # the immediate d(gamma) path (a shared workspace, summed by the call itself)
    dg0, dg1 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres, torch.empty(M, D, device=dev), torch.empty(M, D, dtype=T, device=dev), dg0)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dres, torch.empty(Mf, D, device=dev), torch.empty(Mf, D, dtype=T, device=dev), dg1, seg=SEG)
    assert float((dg0.double() - ref).abs().max()) <= bar and float((dg1.double() - ref).abs().max()) <= bar


# ---- ConvFeedForward middle ---------------------------------------------------------------------------------------------------------------
F_, FP, P_DROP, SEED = 2730, 2752, 0.1, 4321


def _ff_inputs(ops, dev, T):
    g = torch.Generator().manual_seed(F_)
    Mf = B * N
    h1 = torch.zeros(Mf, 2 * FP)
    h1[:, :F_] = torch.randn(Mf, F_, generator=g)
    h1[:, FP:FP + F_] = torch.randn(Mf, F_, generator=g)
    convw = (torch.randn(2 * F_, 3, generator=g) * 0.5).to(dev)
    gamma = (1 + 0.1 * torch.randn(F_, generator=g)).to(dev)
    return h1.to(dev), ops.pack_conv_taps(convw, F_, FP), ops.pad_vector(gamma, FP)


def _planes(v, T):
    hi = v.to(T)
    return hi, (v - hi.float()).to(T)


def _check_ff_forward(full, comp, dev):
    """full / comp: dicts of the outputs of the launch over all rows and of the compact launch with the segment."""
    idx = _idx(dev)
    later = (torch.arange(B * SEG[2], device=dev) % SEG[2]) >= 2           # rows >= p0 + 2 of every sample
    assert same(comp["bits"], full["bits"][idx]), "keep bits of the compact launch != the full launch's rows p0.."
    frac = 1.0 - float(((comp["bits"][:, : F_ // 8, None] >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).float().mean())
    assert abs(frac - P_DROP) < 0.01, frac
    for k in full:
        if k != "bits":
            assert same(comp[k][later], full[k][idx][later]), k
            assert not torch.isnan(comp[k].float()).any(), k


@pytest.mark.parametrize("T", H16)
def test_ffmid_forward_and_backward_with_a_segment(ops, dev, T):
    h1, taps, gpad = _ff_inputs(ops, dev, T)
    h1, taps, gpad = h1.to(T), taps.to(T), gpad.to(T)
    idx = _idx(dev)
    res = []
    for src, nseq, seg in ((h1, N, None), (h1[idx].contiguous(), SEG[2], SEG)):
        M = src.shape[0]
        o = dict(h2=torch.full((M, FP), float("nan"), dtype=T, device=dev), gh=torch.full((M, FP), float("nan"), dtype=T, device=dev),
                 mean=torch.full((M,), float("nan"), device=dev), rstd=torch.full((M,), float("nan"), device=dev),
                 bits=torch.zeros(M, FP // 8, dtype=torch.uint8, device=dev))
        ops.ffmid_fwd(src, taps, gpad, o["h2"], o["mean"], o["rstd"], nseq, F_, FP, P_DROP, SEED, drop_bits=o["bits"], gh=o["gh"], seg=seg)
        res.append((src, nseq, o))
    _check_ff_forward(res[0][2], res[1][2], dev)
    # backward: dh2 is zero in front of row p0 + 2 of every sample (no head reads those rows), the compact launch reads its own buffers
    g = torch.Generator().manual_seed(5)
    dh2 = torch.zeros(B * N, FP)
    dh2[:, :F_] = torch.randn(B * N, F_, generator=g)
    dh2[(torch.arange(B * N) % N) < P0 + 2] = 0
    dh2 = dh2.to(dev).to(T)
    dh1s = []
    for (src, nseq, o), d in zip(res, (dh2, dh2[idx].contiguous())):
        M = src.shape[0]
        dh1 = torch.full((M, 2 * FP), float("nan"), dtype=T, device=dev)
        du = torch.empty(M, 2 * FP, dtype=T, device=dev)
        dgamma, dconv = torch.zeros(F_, device=dev), torch.zeros(2 * F_ * 3, device=dev)
        ws = torch.empty(ops.ffmid_bwd_workspace_floats(F_, FP), device=dev)
        ops.ffmid_bwd(d, src, taps, gpad, o["mean"], o["rstd"], du, dh1, dgamma, dconv, ws, nseq, F_, FP, P_DROP, SEED, drop_bits=o["bits"], gh=o["gh"])
        dh1s.append((dh1, dgamma, dconv))
    full, comp = dh1s
    assert not torch.isnan(comp[0].float()).any()
    assert torch.equal(comp[0].float(), full[0][idx].float()), "dh1 of the compact launch != the full launch's rows p0.."
    assert float(full[0][(torch.arange(B * N, device=dev) % N) < P0].float().abs().max()) == 0.0       # what the compact launch leaves out is zero
    # the parameter gradients sum the same terms in another order
    assert relerr(comp[1], full[1]) < 1e-5 and relerr(comp[2], full[2]) < 1e-5


@pytest.mark.parametrize("T", H16)
def test_ffmid_forward_planes_with_a_segment(ops, dev, T):
    h1, taps, gpad = _ff_inputs(ops, dev, T)
    (h1h, h1l), (tph, tpl), (gph, gpl) = _planes(h1, T), _planes(taps, T), _planes(gpad, T)
    idx = _idx(dev)
    res = []
    for sel, nseq, seg in ((None, N, None), (idx, SEG[2], SEG)):
        a, b_ = (h1h, h1l) if sel is None else (h1h[sel].contiguous(), h1l[sel].contiguous())
        M = a.shape[0]
        o = dict(h2=torch.full((M, FP), float("nan"), dtype=T, device=dev), h2_lo=torch.full((M, FP), float("nan"), dtype=T, device=dev),
                 gh=torch.full((M, FP), float("nan"), dtype=T, device=dev), mean=torch.full((M,), float("nan"), device=dev),
                 rstd=torch.full((M,), float("nan"), device=dev), bits=torch.zeros(M, FP // 8, dtype=torch.uint8, device=dev))
        ops.ffmid_fwd_planes(a, b_, tph, tpl, gph, gpl, o["h2"], o["h2_lo"], o["mean"], o["rstd"], nseq, F_, FP, P_DROP, SEED,
                             drop_bits=o["bits"], gh=o["gh"], seg=seg)
        res.append(o)
    _check_ff_forward(res[0], res[1], dev)


def test_ffmid_forward_mx_with_a_segment(ops, dev):
    T = torch.float16
    h1, taps, gpad = _ff_inputs(ops, dev, T)
    h1h = h1.to(T)
    h1l8 = (((h1 - h1h.float()).to(T).view(torch.int16) >> 8) & 0xFF).to(torch.uint8)          # the lo plane as bf8 bytes: the upper byte of the half
    (tph, tpl), (gph, gpl) = _planes(taps, T), _planes(gpad, T)
    idx = _idx(dev)
    res = []
    for sel, nseq, seg in ((None, N, None), (idx, SEG[2], SEG)):
        a, b_ = (h1h, h1l8) if sel is None else (h1h[sel].contiguous(), h1l8[sel].contiguous())
        M = a.shape[0]
        P = ops.Fp8Planes(M, FP, dev, zero=True)
        o = dict(h2=torch.full((M, FP), float("nan"), dtype=T, device=dev), gh=torch.full((M, FP), float("nan"), dtype=T, device=dev),
                 mean=torch.full((M,), float("nan"), device=dev), rstd=torch.full((M,), float("nan"), device=dev),
                 bits=torch.zeros(M, FP // 8, dtype=torch.uint8, device=dev))
        ops.ffmid_fwd_mx(a, b_, tph, tpl, gph, gpl, o["h2"], P, o["mean"], o["rstd"], nseq, F_, FP, P_DROP, SEED, drop_bits=o["bits"], gh=o["gh"], seg=seg)
        o["hi8"], o["lo8"], o["scale"] = P.planes[0, :M], P.planes[1, :M], P.scale[:M]
        res.append(o)
    _check_ff_forward(res[0], res[1], dev)


# ---- model --------------------------------------------------------------------------------------------------------------------------------
MODEL = dict(dim=1024, depth=2, heads=8)
LENS = (13, 20, 59)                           # tokens per sequence as the layout sees them: 12 clap + eos, 19 semantic + eos, 59 coarse (eos appended, last dropped)
MODEL_SEG = (95, 31, 64)
_ORACLE = {}
_RUNS = {}


def _ids():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, 1024, (B, 12), generator=g), torch.randint(0, 1024, (B, 19), generator=g), torch.randint(0, 1024, (B, 59), generator=g)]


def _run(dev, precision, p, hook):
    """One training step (loss, wanted logits, gradients) of the model built from seed 0, with the hook on or off; cached."""
    key = (precision, p, hook)
    if key in _RUNS:
        return _RUNS[key]
    from open_musiclm_amd import engine
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)                       # the same weights and the same dropout keys in every run
    model = M.create_coarse_transformer(num_coarse_quantizers=3, ff_dropout=p, precision=precision, **MODEL).to(dev)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0)
    wrapper.train()
    seen = []
    orig = engine.trunk_forward

    def spy(*a, **kw):
        seen.append(kw.get("live"))
        return orig(*a, **kw)
    old = os.environ.get("OMLM_LIVE_ROWS")
    os.environ["OMLM_LIVE_ROWS"] = "1" if hook else "0"
    engine.trunk_forward = spy
    try:
        # the trainers' call: only the heads of sequences with a loss weight are evaluated (with every head wanted the rule keeps full rows)
        loss, logits, _ = wrapper(all_token_ids=[t.to(dev) for t in _ids()], return_loss=True, return_logits=False)
        assert logits[0] is None and logits[1] is None
        loss.backward()
    finally:
        engine.trunk_forward = orig
        if old is None:
            del os.environ["OMLM_LIVE_ROWS"]
        else:
            os.environ["OMLM_LIVE_ROWS"] = old
    assert seen == [MODEL_SEG if hook else None], seen
    assert any(k[1] == LENS for k in model.__dict__["_omlm_layouts"])
    s = grad_unscale(precision)
    grads = {k: (v.grad.detach().float() * s if v.grad is not None else None) for k, v in model.named_parameters()}     # (kept on the device)
    _RUNS[key] = dict(loss=float(loss), logits=logits[-1].detach().double().cpu(), grads=grads)
    if not _ORACLE:
        _oracle({k: v.detach().cpu() for k, v in model.state_dict().items()}, list(grads))
    return _RUNS[key]


def _oracle(sd=None, names=None):
    """Loss, wanted logits and the gradient of every parameter from the CPU oracle in fp64 (p = 0), once (every run starts from the same weights)."""
    if not _ORACLE:
        from oracle import musiclm_oracle as O
        spec = O.coarse_spec(**MODEL)
        sdo = {k: (v.double().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
        loss, logits, _ = O.wrapper_forward_loss(sdo, spec, _ids(), [0., 0., 1.], forget_noise=None)
        gr = torch.autograd.grad(loss, [sdo[k] for k in names], allow_unused=True)
        _ORACLE.update(loss=float(loss.detach()), logits=logits[-1].detach(), grads=dict(zip(names, gr)))
    return _ORACLE


def _grad_errors(run, o):
    """Per parameter tensor: error of the gradient against the oracle, with test_gpu_geometry's floors (rel-pos MLP biases: near-invariant
    directions of the softmax, judged against 1e-2 of the largest gradient).  Tensors no wanted head reaches have no gradient on either side."""
    gmax = max(float(v.abs().max()) for v in o["grads"].values() if v is not None)
    errs = {}
    for k, ref in o["grads"].items():
        got = run["grads"].get(k)
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        assert got is not None, k
        errs[k] = relerr(got, ref, floor=1e-2 * gmax if (k in RELPOS_TENSORS and k.endswith("bias")) else 0.0)
    return errs


@pytest.mark.parametrize("precision", ["fp16ff", "bf16"])
def test_model_hook_on_against_off_and_the_oracle(dev, precision):
    """p = 0.  Measured on an MI355X: worst on/off ratio of the per-tensor gradient errors 1.0001 (fp16ff, transformer.norm.gamma) and
    1.00002 (bf16); with the hook on, loss 2.9e-6 / logits 8.6e-5 / worst gradient 5.7e-3 (fp16ff) and 1.8e-5 / 5.1e-3 / 8.1e-2 (bf16)
    against the oracle (profiles/live_rows.md)."""
    on, off = _run(dev, precision, 0.0, True), _run(dev, precision, 0.0, False)
    o = _oracle()
    tol = TOL[precision]
    e_on, e_off = _grad_errors(on, o), _grad_errors(off, o)
    ratios = {k: e_on[k] / max(e_off[k], 1e-300) for k in e_on}
    worst = max(ratios.items(), key=lambda kv: kv[1])
    fig = dict(loss_on=abs(on["loss"] - o["loss"]) / o["loss"], loss_off=abs(off["loss"] - o["loss"]) / o["loss"],
               logits_on=relerr(on["logits"], o["logits"]), logits_off=relerr(off["logits"], o["logits"]),
               worst_grad_on=max(e_on.items(), key=lambda kv: kv[1]), worst_grad_off=max(e_off.items(), key=lambda kv: kv[1]), worst_ratio=worst)
    print(f"live_rows_model[{precision}] {fig}")
    for k in sorted(ratios, key=ratios.get, reverse=True)[:8]:
        print(f"  {k}: on {e_on[k]:.4e} off {e_off[k]:.4e} ratio {ratios[k]:.4f}")
    report(f"live_rows_model[{precision}]", **fig)
    assert on["logits"].shape == o["logits"].shape
    assert fig["logits_on"] < tol["logits"] and fig["loss_on"] < tol["loss"], fig
    assert max(e_on.values()) < tol["grad"], fig
    bad = {k: (e_on[k], e_off[k]) for k, r in ratios.items() if r > 1.25}
    assert not bad, bad


RESOLUTION = 2.0 ** -20                       # 8 ulp of fp32: below it an on/off figure is the atomics' summation order, not the change


def _on_off(dev, precision, p):
    on, off = _run(dev, precision, p, True), _run(dev, precision, p, False)
    d_loss = abs(on["loss"] - off["loss"]) / abs(off["loss"])
    # (the floor of _grad_errors: the rel-pos MLP's biases are near-invariant directions of the softmax -- their computed gradient is mostly
    # rounding noise --, judged against 1e-2 of the largest gradient as everywhere else in the suite)
    gmax = max(float(g.abs().max()) for g in off["grads"].values() if g is not None)
    d_grad = {k: relerr(on["grads"][k], g, floor=1e-2 * gmax if (k in RELPOS_TENSORS and k.endswith("bias")) else 0.0)
              for k, g in off["grads"].items() if g is not None and float(g.abs().max()) > 0}
    return d_loss, d_grad


@pytest.mark.parametrize("precision", ["fp16ff", "bf16"])
def test_model_with_ff_dropout_hook_on_matches_off(dev, precision):
    """ff_dropout = 0.1: the compact launch draws the keep bits of the full one, so on and off differ by what they differ by at p = 0 (summation
    order, peeled tails) and no more: twice the p = 0 figure, for the loss and for the worst gradient tensor.  Both figures sit at the
    resolution of the numbers themselves -- the loss and the gradients are fp32 sums that the kernels accumulate with atomics, so two runs
    of the SAME configuration differ by a few ulp -- and "twice" of such a figure is not resolved: nothing below 8 fp32 ulp (2^-20) counts.
    A mask that moved with the rows would show as a difference of the order of the gradients themselves (1e-1).
    Measured on an MI355X, on/off, p = 0 | p = 0.1: loss 2.3e-7 | 7.5e-8 (fp16ff), 7.5e-8 | 0 (bf16); worst tensor 7.2e-7 | 2.7e-7, 5.0e-7 | 6.0e-7."""
    l0, g0 = _on_off(dev, precision, 0.0)
    l1, g1 = _on_off(dev, precision, 0.1)
    w0, w1 = max(g0.items(), key=lambda kv: kv[1]), max(g1.items(), key=lambda kv: kv[1])
    print(f"live_rows_dropout[{precision}] loss on/off p=0 {l0:.3e} p=0.1 {l1:.3e}; worst grad on/off p=0 {w0} p=0.1 {w1}")
    report(f"live_rows_dropout[{precision}]", loss_p0=l0, loss_p01=l1, worst_grad_p0=w0, worst_grad_p01=w1)
    for k in sorted(g1, key=g1.get, reverse=True)[:6]:
        print(f"  {k}: on/off p=0 {g0[k]:.3e} p=0.1 {g1[k]:.3e}")
    assert abs(_run(dev, precision, 0.1, True)["loss"] - _run(dev, precision, 0.0, True)["loss"]) > 1e-4      # the dropout is on
    assert l1 <= max(2 * l0, RESOLUTION), (l0, l1)
    assert w1[1] <= max(2 * w0[1], RESOLUTION), (w0, w1)


def test_captured_graph_step_with_the_hook_on(dev):
    from open_musiclm_amd import engine
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.graph import GraphedForwardBackward
    from open_musiclm_amd.optimizer import get_optimizer
    old = os.environ.pop("OMLM_LIVE_ROWS", None)             # the default: hook on (the rule reads the variable at every call)
    try:
        _captured_graph_step(dev, engine, M, GraphedForwardBackward, get_optimizer)
    finally:
        if old is not None:
            os.environ["OMLM_LIVE_ROWS"] = old


def _captured_graph_step(dev, engine, M, GraphedForwardBackward, get_optimizer):
    torch.manual_seed(0)
    model = M.create_coarse_transformer(num_coarse_quantizers=3, ff_dropout=0.1, precision="fp16ff", **MODEL).to(dev)
    stage = M.CoarseStage(coarse_transformer=model, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0).train()
    opt = get_optimizer(model.parameters(), lr=1e-4, wd=0.01)
    opt.zero_grad()
    g = torch.Generator().manual_seed(4)
    kw = dict(clap_token_ids=torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev), semantic_token_ids=torch.randint(0, 1024, (B, 19), generator=g).to(dev),
              coarse_token_ids=torch.randint(0, 1024, (B, 20, 3), generator=g).to(dev))
    seen = []
    orig = engine.trunk_forward

    def spy(*a, **k):
        seen.append(k.get("live"))
        return orig(*a, **k)
    engine.trunk_forward = spy
    try:
        fb = GraphedForwardBackward(lambda **k: stage(**k, return_loss=True, return_logits=False)[0])
        fb.prepare(kw, after_warmup=lambda: (opt.mark_grads_dirty(), opt.zero_grad()))
    finally:
        engine.trunk_forward = orig
    assert fb.graph is not None, fb.capture_error
    assert seen and all(s is not None and s[2] * B % 64 == 0 for s in seen), seen
    opt.zero_grad()
    l1 = float(fb(**kw))
    gn1 = float(opt.flat_grad.double().norm())
    l_eager = float(fb._eager({k: v.clone() for k, v in kw.items()}))
    assert l1 == l1 and gn1 > 0 and gn1 == gn1
    # a replay draws a new dropout mask (the salt is a device counter): the losses agree to the dropout's noise, not to rounding
    assert abs(l1 - l_eager) < 0.05 * abs(l_eager), (l1, l_eager)
