"""GPU: label smoothing and z-loss in the fused cross entropy (include/omlm.h) -- omlm_cross_entropy_fwd_reg / _bwd_reg
(csrc/embed_ce.hip: the REG instantiations of the four cross-entropy kernels) against the fp64 restatement of tests/ce_reg_ref.py on
every route of the two launchers, the zero case against the plain entries bit for bit, and the keywords from
TokenConditionedTransformerWrapper down: against the CPU oracle with the regularised loss formed in fp64, eval() / score() as the plain
cross entropy, the library calls of a run without the keywords, the captured training step and the trainer."""
import numpy as np
import pytest
import torch

import ce_reg_ref as CR
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_loss_optim_sampler import _ce_inputs, _ulp
from test_gpu_model import TOL, grad_unscale

pytestmark = pytest.mark.gpu

NAN = float("nan")
START = (1.5, -0.75, 2.25)                                        # the three sums ACCUMULATE onto what is there

# V: 1088 is the widest row of the wave-per-row forward (64 lanes x 17 slots), 1089 the first workgroup-kernel row; 64 / 65 straddle one
# lane trip.  R: 5 is a second workgroup of the wave kernel (4 rows each), 4097 one row past a full trip of both forward grids.
CE_REG_SHAPES = [(R_, V) for R_ in (1, 3, 5, 4097) for V in (1, 63, 64, 65, 1025, 1088, 1089, 2049)]
CE_REG_PARAMS = [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-2)]
_INPUTS = {}


def _shared_inputs(R_, V):
    """_ce_inputs of tests/test_gpu_loss_optim_sampler.py and the fp64 row terms, made once per shape and left unchanged."""
    if (R_, V) not in _INPUTS:
        _INPUTS.clear()                                          # (the cases of one shape run back to back: one shape is kept)
        x, logits, labels = _ce_inputs(R_, V, seed=R_ * 31 + V)
        _INPUTS[R_, V] = (x, logits, labels, CR.row_terms(x, labels))
    return _INPUTS[R_, V]


def _fwd_reg(logits, labels, lse, sums, V):
    from open_musiclm_amd import hip
    from open_musiclm_amd import ops as O
    R, ld = logits.shape
    hip.call("omlm_cross_entropy_fwd_reg", hip.ptr(logits), hip.ptr(labels), hip.ptr(lse), hip.ptr(sums), R, V, ld,
             hip.ptr(O.index_error_flag(logits.device)), hip.stream_ptr())


def _bwd_reg(logits, labels, lse, gs, coef, dl, V, eps, zeta):
    from open_musiclm_amd import hip
    from open_musiclm_amd import ops as O
    R, ld = logits.shape
    hip.call("omlm_cross_entropy_bwd_reg", hip.ptr(logits), hip.ptr(labels), hip.ptr(lse), hip.ptr(gs), float(coef), hip.ptr(dl),
             R, V, ld, dl.shape[-1], O.dcode(dl.dtype), float(eps), float(zeta), hip.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against fp64
@pytest.mark.parametrize("R_,V,eps,zeta", [(R_, V, e, z) for R_, V in CE_REG_SHAPES for e, z in CE_REG_PARAMS])
def test_regularised_cross_entropy_routes_against_fp64(ops, dev, R_, V, eps, zeta):
    x, logits, labels, (lse_ref, nll_r, smooth_r, z_r) = _shared_inputs(R_, V)
    lg, lb = logits.to(dev), labels.to(dev)
    lse = torch.full((R_,), NAN, device=dev)
    sums = torch.tensor(START, device=dev)
    ops.ce_fwd(lg, lb, lse, sums, V, label_smoothing=eps, z_loss=zeta)
    lse_got = lse.cpu().double()
    e_lse = float(((lse_got - lse_ref).abs() / lse_ref.abs().clamp(min=1.0)).max())
    want = [s + float(t.sum()) for s, t in zip(START, (nll_r, smooth_r, z_r))]
    got = [float(v) for v in sums.cpu()]
    e_nll, e_smooth, e_z = (abs(g - w) / abs(w) for g, w in zip(got, want))
    # backward: every route of the launcher.  The reference takes the kernel's own row_lse (an input of ce_bwd, checked above), so this
    # check sees the backward alone: dl = coef * g * (exp(l - lse) (1 + 2 zeta lse) - (1 - eps) onehot - eps / V)
    live = labels >= 0
    g64 = CR.grad(x, labels, eps, zeta, lse=lse_got)
    amp = 1.0 + 2.0 * zeta * float(lse_got.abs().max())           # the bars of the plain test with |g| -> |g| (1 + 2 zeta max|lse|)
    ldw = ((V + 8) // 8) * 8                                     # ldd % 8 == 0 + 16-byte aligned buffers: the 16-bit wave kernel
    ldo = V + 3 if (V + 3) % 8 else V + 5                        # ldd % 8 != 0: the element-wise fallback
    gdev = torch.tensor([0.25], device=dev)
    variants = [("fp32", torch.float32, ldw, 0, None, 3.0), ("fp32_gs", torch.float32, ldo, 0, gdev, 0.7)]
    for dt, nm in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        variants += [(f"{nm}_wave", dt, ldw, 0, gdev, 3.0), (f"{nm}_wave_nogs", dt, ldw, 0, None, 0.7),
                     (f"{nm}_odd_ldd", dt, ldo, 0, gdev, 0.7), (f"{nm}_offset", dt, ldw, 1, None, 3.0)]
    errs = {}
    for name, dt, ldd, off, gs, coef in variants:
        gtot = coef * (0.25 if gs is not None else 1.0)
        buf = torch.full((R_ * ldd + 8,), NAN, dtype=dt, device=dev)
        dl = buf[off:off + R_ * ldd].view(R_, ldd)               # off = 1: a 2- or 4-byte misaligned view -> the fallback kernel
        ops.ce_bwd(lg, lb, lse, gs, coef, dl, V, label_smoothing=eps, z_loss=zeta)
        got_d = dl.cpu()
        assert bool((got_d[:, V:] == 0).all()), name             # pad columns [V, ldd) written as exact zeros
        assert bool((got_d[~live] == 0).all()), name             # ignored rows: exact zeros
        if off:
            assert bool(torch.isnan(buf[:off].cpu()).all()) and bool(torch.isnan(buf[off + R_ * ldd:].cpu()).all()), name
        ref = gtot * g64
        d = (got_d[:, :V].double() - ref).abs()
        if dt == torch.float32:
            errs[name] = float(d.max()) / (gtot * amp)           # |err| / (|g| (1 + 2 zeta max|lse|))
        else:
            errs[name] = float((d / (_ulp(ref, dt) + 1e-5 * gtot * amp)).max())
    # the one-off all-ignored batch: nothing is added to any sum, every gradient is zero
    if R_ == 3:
        lb_none = torch.full((R_,), -1, dtype=torch.int32, device=dev)
        sums2 = torch.tensor(START, device=dev)
        ops.ce_fwd(lg, lb_none, lse, sums2, V, label_smoothing=eps, z_loss=zeta)
        dl = torch.full((R_, ldw), NAN, dtype=torch.bfloat16, device=dev)
        ops.ce_bwd(lg, lb_none, lse, gdev, 3.0, dl, V, label_smoothing=eps, z_loss=zeta)
        assert sums2.cpu().tolist() == list(START) and bool((dl == 0).all())
    report(f"ce_reg[{R_}x{V},{eps},{zeta}]", lse_rel=e_lse, nll_rel=e_nll, smooth_rel=e_smooth, z_rel=e_z, **{f"bwd_{k}": v for k, v in errs.items()})
    print(f"ce_reg[{R_}x{V},{eps},{zeta}] lse {e_lse:.2e} nll {e_nll:.2e} smooth {e_smooth:.2e} z {e_z:.2e} bwd fp32 "
          f"{max(v for k, v in errs.items() if k.startswith('fp32')):.2e} 16-bit {max(v for k, v in errs.items() if not k.startswith('fp32')):.2e}")
    for name, e in errs.items():
        assert e <= (1e-6 if name.startswith("fp32") else 1.0), (name, e)          # the bars of the plain test, in the units above
    assert e_lse <= 1e-6, e_lse                                  # the plain test's bar
    assert e_nll <= 1e-5, e_nll                                  # the plain test's bar
    # smooth and z sums: 4x the worst value measured over these 96 cases, rounded up to one digit (the headroom is for the unordered
    # float atomics and another machine of the pool); the constants below, profiles/ce_reg.md
    assert e_smooth <= SMOOTH_BAR, e_smooth
    assert e_z <= Z_BAR, e_z


# MEASURED (MI355X, the 96 cases above): smooth sum <= 2.18e-6 relative (4097 x 2049), z sum <= 1.76e-6 (4097 x 2049); beside them
# lse <= 1.7e-7, nll sum <= 3.4e-6, backward fp32 <= 1.6e-7 of |g| (1 + 2 zeta max|lse|), 16-bit <= 0.4991 of its unit
SMOOTH_MEASURED, SMOOTH_BAR = 2.18e-6, 9e-6                     # 4 x 2.18e-6 = 8.7e-6
Z_MEASURED, Z_BAR = 1.76e-6, 8e-6                               # 4 x 1.76e-6 = 7.03e-6


def test_a_label_past_the_vocabulary_adds_nothing_and_raises_the_flag(ops, dev):
    from open_musiclm_amd import ops as O
    for V in (41, 1089):                                         # the wave and the workgroup forward
        x, logits, labels = _ce_inputs(9, V, seed=V)
        labels[4] = V                                            # a live row becomes a row past the vocabulary
        lg, lb = logits.to(dev), labels.to(dev)
        lse = torch.full((9,), NAN, device=dev)
        sums = torch.zeros(3, device=dev)
        flag = O.index_error_flag(dev)
        flag.zero_()
        ops.ce_fwd(lg, lb, lse, sums, V, label_smoothing=0.1, z_loss=1e-2)
        assert int(flag.item()) == 4
        flag.zero_()
        want = CR.sums(x, labels)                                # (the restatement leaves such rows out)
        for g, w in zip(sums.cpu().tolist(), want):
            assert abs(g - w) <= 1e-5 * abs(w), (V, g, w)
        for dt in (torch.float32, torch.float16):
            dl = torch.full((9, (V + 8) // 8 * 8), NAN, dtype=dt, device=dev)
            ops.ce_bwd(lg, lb, lse, None, 1.0, dl, V, label_smoothing=0.1, z_loss=1e-2)
            assert bool((dl[4] == 0).all()) and bool((dl[6] == 0).all()) and float(dl[0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. zero is the old kernel
@pytest.mark.parametrize("R_,V", [(5, 65), (4097, 1025), (5, 1089), (4097, 1089)])
def test_zero_passed_to_the_new_entries_is_the_old_kernel(ops, dev, R_, V):
    x, logits, labels, (_, nll_r, smooth_r, z_r) = _shared_inputs(R_, V)
    lg, lb = logits.to(dev), labels.to(dev)
    lse_old, lse_new = torch.full((R_,), NAN, device=dev), torch.full((R_,), NAN, device=dev)
    nll_old, sums = torch.tensor([1.5], device=dev), torch.tensor(START, device=dev)
    ops.ce_fwd(lg, lb, lse_old, nll_old, V)
    _fwd_reg(lg, lb, lse_new, sums, V)
    assert torch.equal(lse_old, lse_new)
    got = sums.cpu().tolist()
    assert abs(got[0] - float(nll_old)) <= 1e-5 * abs(float(nll_old))
    for g, s, t in zip(got[1:], START[1:], (smooth_r, z_r)):      # the smooth and z sums are still written
        w = s + float(t.sum())
        assert abs(g - w) <= max(SMOOTH_BAR, Z_BAR) * abs(w), (g, w)
    ldw, ldo = ((V + 8) // 8) * 8, (V + 3 if (V + 3) % 8 else V + 5)
    gdev = torch.tensor([0.25], device=dev)
    for dt, ldd, gs in ((torch.float32, ldw, None), (torch.float32, ldo, gdev), (torch.bfloat16, ldw, gdev), (torch.float16, ldw, None),
                        (torch.float16, ldo, gdev)):
        a = torch.full((R_, ldd), NAN, dtype=dt, device=dev)
        b = torch.full((R_, ldd), NAN, dtype=dt, device=dev)
        ops.ce_bwd(lg, lb, lse_old, gs, 0.7, a, V)
        _bwd_reg(lg, lb, lse_old, gs, 0.7, b, V, 0.0, 0.0)
        assert torch.equal(a, b), (dt, ldd)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the model against the oracle
from test_ce_reg_host import EPS, EPS_SEEN, HEAD, ZETA, oracle_regularised as _oracle_regularised  # noqa: E402  (made once, shared)


def _grad_errs(model, ref, precision):
    """Every parameter gradient in the units of test_training_step_matches_reference_golden (tests/test_gpu_model.py): the largest
    deviation over max(the reference tensor's largest entry, 1e-3 of the model's largest); the analytically-zero directions apart."""
    gscale = max(float(v.abs().max()) for v in ref.values())
    out = {}
    for k, p in model.named_parameters():
        if k not in ref:
            continue
        got = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu() * grad_unscale(precision)
        out[k] = float((got.double() - ref[k].double()).abs().max() / max(float(ref[k].abs().max()), 1e-3 * gscale))
    inv = {k: out.pop(k) for k in list(out) if k.endswith("rel_pos_bias.net.3.bias") or k.endswith("relative_attention_bias.weight")}
    return out, inv


@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_regularised_training_step_matches_the_oracle(golden_dir, dev, precision, monkeypatch):
    """tiny_coarse golden, training mode, forgetful mask and dropouts off, zeta = 1e-2, on the torch preparation path and the fused
    one-launch path.  At eps = 0.1: loss within the loss bar, every parameter gradient within the bars the unregularised check holds
    them to, and the expected losses with either term left out miss the measured one by more than 10x the loss bar.  At eps = 0.5 (the
    smallest round value at which the oracle alone clears it, tests/test_ce_reg_host.py::test_each_term_is_visible_to_the_oracle): the
    same agreement, and the expected logit-head weight gradient without smoothing misses the measured one by more than 10x its bar."""
    from open_musiclm_amd import open_musiclm as M
    from test_gpu_model import build_from_golden
    z, model = build_from_golden(golden_dir, "tiny_coarse", dev, precision)
    o = _oracle_regularised(golden_dir)
    dids = [torch.from_numpy(z[f"ids.{i}"]).to(dev) for i in range(3)]
    tol = TOL[precision]
    for path in ("fused", "torch"):
        if path == "torch":
            monkeypatch.setenv("OMLM_FUSED_PREP", "0")
        for eps in (EPS, EPS_SEEN):
            want, ref = o[eps, ZETA]
            wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.],
                                                           mask_prob=0.0, label_smoothing=eps, z_loss=ZETA).train()
            model.zero_grad(set_to_none=True)
            loss, _, _ = wrapper(all_token_ids=dids, return_loss=True, return_logits=False)
            loss.backward()
            got = float(loss.detach())
            e_loss = abs(got - want) / want
            grads, inv = _grad_errs(model, ref, precision)
            worst = max(grads.items(), key=lambda kv: kv[1])
            no_eps, _ = _grad_errs(model, o[0.0, ZETA][1], precision)
            print(f"regularised step [{precision}, {path}, eps {eps}]: loss rel err {e_loss:.2e}, worst gradient {worst}, invariant "
                  f"{max(inv.values()):.2e}; head gradient against the expected one without smoothing {no_eps[HEAD]:.3e}")
            report(f"ce_reg_train[{precision},{path},{eps}]", loss=e_loss, worst_grad=worst, grads=grads, invariant=inv, head_without_smoothing=no_eps[HEAD])
            assert e_loss < tol["loss"], (path, eps, e_loss)
            assert worst[1] < tol["grad"], (path, eps, worst)
            assert all(v < tol["invariant"] for v in inv.values()), (path, eps, inv)
            # each term is seen: the expected values with a term left out miss what was measured
            assert abs(got - o[eps, 0.0][0]) > 10 * tol["loss"] * want, (path, eps)
            assert abs(got - o[0.0, ZETA][0]) > 10 * tol["loss"] * want, (path, eps)
            if eps == EPS_SEEN:
                assert no_eps[HEAD] > 10 * tol["grad"], (path, no_eps[HEAD])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. eval is plain
def test_eval_and_score_are_the_plain_cross_entropy(golden_dir, dev):
    from open_musiclm_amd import open_musiclm as M
    from test_gpu_model import build_from_golden
    z, model = build_from_golden(golden_dir, "tiny_coarse", dev, "fp16ff")
    kw = dict(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.15)
    plain = M.TokenConditionedTransformerWrapper(**kw).eval()
    reg = M.TokenConditionedTransformerWrapper(label_smoothing=EPS, z_loss=ZETA, **kw).eval()
    dids = [torch.from_numpy(z[f"ids.{i}"]).to(dev) for i in range(3)]
    with torch.no_grad():
        for pk in (dict(), dict(return_logits=False)):
            lp, gp, _ = plain(all_token_ids=dids, return_loss=True, **pk)
            lr, gr, _ = reg(all_token_ids=dids, return_loss=True, **pk)
            assert abs(float(lp) - float(lr)) <= 2e-6 * abs(float(lp)), (float(lp), float(lr))      # (the atomics' order)
            for a, b in zip(gp, gr):
                assert (a is None and b is None) or torch.equal(a, b)
        sp = plain.score(conditioning_token_ids=dids[:2], pred_token_ids=dids[2])
        sr = reg.score(conditioning_token_ids=dids[:2], pred_token_ids=dids[2])
        assert torch.equal(sp, sr)
        lt, _, _ = reg.train()(all_token_ids=dids, return_loss=True, return_logits=False)         # and training mode is not
    model.eval()
    assert abs(float(lt) - float(lp)) > 1e-3 * abs(float(lp))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. off means off
def _small(dev, precision="bf16x3"):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(1)
    return M.create_coarse_transformer(dim=64, depth=2, heads=2, ff_dropout=0.0, num_coarse_quantizers=3, num_clap_quantizers=3,
                                       clap_codebook_size=32, semantic_codebook_size=48, acoustic_codebook_size=40, precision=precision).to(dev)


NEW = ("omlm_cross_entropy_fwd_reg", "omlm_cross_entropy_bwd_reg")
OLD = ("omlm_cross_entropy_fwd", "omlm_cross_entropy_bwd")


@pytest.mark.parametrize("path", ["fused", "torch"])
def test_off_launches_what_it_always_launched(dev, path, monkeypatch):
    """The hip.call spy of tests/test_gpu_guidance.py around a training forward + backward with the forgetful mask on."""
    import sys
    from open_musiclm_amd import hip
    from open_musiclm_amd import open_musiclm as M
    model = _small(dev)
    g = torch.Generator().manual_seed(2)
    raw = [torch.randint(0, 32, (3, 2, 3), generator=g).to(dev), torch.randint(0, 48, (3, 7), generator=g).to(dev),
           torch.randint(0, 40, (3, 4, 3), generator=g).to(dev)]
    if path == "torch":
        monkeypatch.setenv("OMLM_FUSED_PREP", "0")
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    def run(weights=(0., 0., 1.), **kw):
        w = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=list(weights),
                                                 mask_prob=0.15, **kw).train()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(77)
        del names[:]
        loss, _, _ = w(all_token_ids=raw, return_loss=True, return_logits=False)
        loss.backward()
        return list(names), torch.cuda.get_rng_state(dev).clone(), float(loss.detach())
    run()                                                            # anything built on first use is built
    for mod in [m for n, m in list(sys.modules.items()) if n.startswith("open_musiclm_amd") and getattr(m, "call", None) is real]:
        monkeypatch.setattr(mod, "call", spy)
    base, rng0, l0 = run()
    assert all(n in base for n in OLD) and not any(n in base for n in NEW)
    for kw in (dict(label_smoothing=0, z_loss=0), dict(label_smoothing=0.0, z_loss=0.0)):
        got, rng, l = run(**kw)
        assert got == base and torch.equal(rng, rng0) and abs(l - l0) <= 2e-6 * abs(l0), kw
    for kw in (dict(label_smoothing=0.1), dict(z_loss=1e-2), dict(label_smoothing=0.1, z_loss=1e-2)):
        got, rng, l = run(**kw)
        assert [n for n in got if n not in NEW] == [n for n in base if n not in OLD], kw      # everything else is the same
        assert [got.count(n) for n in NEW] == [1, 1] and not any(n in got for n in OLD), kw
        assert torch.equal(rng, rng0), kw
        assert "z_loss" not in kw or abs(l - l0) > 1e-3 * abs(l0), kw          # (smoothing alone hardly moves an untrained model's loss)
    got, _, _ = run(weights=(0., 0.5, 1.), label_smoothing=0.1, z_loss=1e-2)                   # once per sequence with a positive weight
    assert [got.count(n) for n in NEW] == [2, 2] and not any(n in got for n in OLD)
    model.eval()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the captured step
@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_graphed_and_eager_micro_steps_agree_with_the_regularised_loss(dev, precision):
    """The pattern and bars of test_graphed_and_eager_micro_steps_agree_with_the_drop (tests/test_gpu_guidance.py): dim 64, depth 2,
    B = 2, three optimizer steps; the captured micro-step carries the _reg launches and the python-scalar combination of the sums."""
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.graph import GraphedForwardBackward
    from open_musiclm_amd.optimizer import get_optimizer
    B = 2
    g = torch.Generator().manual_seed(3)
    batches = [[torch.randint(0, 32, (B, 2, 3), generator=g).to(dev), torch.randint(0, 48, (B, 9), generator=g).to(dev),
                torch.randint(0, 40, (B, 6, 3), generator=g).to(dev)] for _ in range(3)]
    keys = ("clap_token_ids", "semantic_token_ids", "coarse_token_ids")

    def run(use_graph, **reg):
        torch.manual_seed(0)
        model = M.create_coarse_transformer(dim=64, depth=2, heads=2, ff_dropout=0.0, num_coarse_quantizers=3, num_clap_quantizers=3,
                                            clap_codebook_size=32, semantic_codebook_size=48, acoustic_codebook_size=40, precision=precision).to(dev)
        stage = M.CoarseStage(coarse_transformer=model, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0, **reg).train()
        opt = get_optimizer(model.parameters(), lr=3e-3, wd=0.01)
        opt.zero_grad()
        fb = GraphedForwardBackward(lambda **kw: stage(**kw, return_loss=True, return_logits=False)[0], enabled=use_graph, instances=1)

        def discard():
            opt.mark_grads_dirty()
            opt.zero_grad()
        fb.prepare(dict(zip(keys, batches[0])), after_warmup=discard)
        assert (fb.graph is not None) == use_graph, fb.capture_error
        losses = []
        for k in range(3):
            opt.zero_grad()
            loss = fb(**dict(zip(keys, batches[k])))
            opt.mark_grads_dirty()
            opt.step(max_grad_norm=0.5)
            losses.append(float(loss))
        import gc
        gc.unfreeze()
        return losses
    le = run(False, label_smoothing=0.1, z_loss=1e-2)
    lg = run(True, label_smoothing=0.1, z_loss=1e-2)
    l0 = run(False)
    print(f"graph vs eager with the regularised loss [{precision}]: eager {le} graph {lg} without {l0}")
    for a, b in zip(le, lg):
        assert abs(a - b) <= (2e-4 if precision == "bf16x3" else 5e-3) * abs(a), (le, lg)
    assert abs(le[0] - l0[0]) > 1e-3 * abs(l0[0]) and abs(lg[0] - l0[0]) > 1e-3 * abs(l0[0]), (le, lg, l0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the trainer
def test_trainer_builds_a_stage_that_carries_both_values(dev, tmp_path):
    from dataclasses import asdict
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.config import SingleStageTrainerConfig
    from open_musiclm_amd.data import SyntheticTokenDataset
    from open_musiclm_amd.trainer import SingleStageTrainer
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=128, depth=2, heads=2, num_coarse_quantizers=3, ff_dropout=0.0, precision="bf16").to(dev)
    ds = SyntheticTokenDataset("coarse", length=8, coarse_window_seconds=1, semantic_window_seconds=2)
    cfg = SingleStageTrainerConfig(stage="coarse", folder="", valid_frac=0.0, lr=3e-3, lr_warmup=0, batch_size=2, grad_accum_every=1, wd=0.01,
                                   max_grad_norm=0.5, cross_entropy_loss_weights=[0., 0., 1.], num_train_steps=2, save_results_every=1000,
                                   save_model_every=1000, save_predicted_tokens=False, save_reconstructed_wave=False,
                                   use_preprocessed_data=False, label_smoothing=0.1, z_loss=1e-4)
    again = SingleStageTrainerConfig(**asdict(cfg))
    assert (again.label_smoothing, again.z_loss) == (0.1, 1e-4)
    kw = {k: v for k, v in asdict(again).items() if k not in ("stage", "folder", "use_preprocessed_data")}
    tr = SingleStageTrainer(model, "coarse", dataset=ds, results_folder=str(tmp_path / "res"), **kw)
    w = tr.train_wrapper.transformer_wrapper
    assert (w.label_smoothing, w.z_loss) == (0.1, 1e-4) and (tr.label_smoothing, tr.z_loss) == (0.1, 1e-4)
    assert np.isfinite(tr.train_step()["loss"])
