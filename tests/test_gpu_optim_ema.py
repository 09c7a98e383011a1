"""GPU: the weight EMA of the fused optimizer step -- the kernel entry (csrc/optim_misc.hip, omlm_adamw_clip_step_ema) on both its
paths and past its grid cap, its clock and its skipped steps, FusedAdam's flat EMA buffer and its resume, the read-only twin model on
that buffer (logits, generate, a stale operand cache), and the trainer's checkpoints.  The rule is restated in optim_ema_ref.py; every
EMA value is checked against the fp64 blend of the kernel's OWN fp32 parameters, so only the blend's rounding is under test."""
import os

import numpy as np
import pytest
import torch

import optim_ema_ref as R
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_loss_optim_sampler import ADAMW_CASES, INF, NAN, _flat_bufs, _gen, _grads, _guards_ok

pytestmark = pytest.mark.gpu

HP = dict(lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01)
# (decay 0.9) d over steps 1, 2, 3: the warm-up's 2/11, 3/12, 4/13; 0 then 0.9 twice; 0 throughout (the EMA follows the weights)
MODES = {"warmup": dict(ema_update_after_step=0, ema_warmup=True), "plain": dict(ema_update_after_step=1, ema_warmup=False),
         "follow": dict(ema_update_after_step=3, ema_warmup=True)}
PAST_CAP = 4 * 4096 * 256 + 4 * 300 + 3                        # the 4096-workgroup grid takes a second trip, plus a scalar tail
KERNEL_CASES = [c + (m,) for c in ADAMW_CASES if c[0] <= 10007 for m in MODES] + \
               [(PAST_CAP, False, torch.bfloat16, True, "warmup"), (PAST_CAP, True, torch.float16, False, "plain")]


def _same_bits(a, b):
    return torch.equal(R.bits(a), R.bits(b))


def _check_ema(E, ref, P, steps, what):
    """E against the fp64 reference within optim_ema_ref.bound; returns the worst error / bound."""
    err = (E.detach().double().cpu() - ref).abs()
    bnd = R.bound(steps, P.detach(), ref)
    ratio = float((err / bnd.clamp(min=1e-300)).max())
    print(f"{what}: max |E - ref| {float(err.max()):.3e}, worst error / bound {ratio:.3f}")
    assert bool((err <= bnd).all()), (what, float(err.max()), ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel entry
@pytest.mark.parametrize("n,scalar,p16_dtype,decoupled,mode", KERNEL_CASES)
def test_ema_entry_blends_and_leaves_the_step_alone(ops, dev, n, scalar, p16_dtype, decoupled, mode):
    g = _gen(n + 2 * scalar + int(decoupled))
    p0 = torch.randn(n, generator=g)
    e0 = p0 * (1.0 + 0.05 * torch.randn(n, generator=g))
    bufs_a, p16_a = _flat_bufs(n, scalar, dev, p16_dtype, [p0, None, None, None, e0])      # the EMA entry
    bufs_b, p16_b = _flat_bufs(n, scalar, dev, p16_dtype, [p0, None, None, None])          # the entry without it
    (_, Pa), (_, Ga), (_, Ma), (_, Va), (_, E) = bufs_a
    (_, Pb), (_, Gb), (_, Mb), (_, Vb) = bufs_b
    off = 1 if scalar else 0
    nsq = torch.zeros(1, device=dev)
    ref, worst = e0.double(), 0.0
    for step, grad in enumerate(_grads(n, g, (0.3, 10.0, 0.5)), start=1):
        Ga.copy_(grad.to(dev))
        Gb.copy_(Ga)
        nsq.zero_()
        ops.sumsq_accumulate(Ga.clone(), nsq)
        kw = dict(HP, step=step, gscale=0.5, gnorm_sq=nsq, max_norm=1.0, decoupled=decoupled, zero_grad=True)
        ops.adamw_clip_step(Pb, Gb, Mb, Vb, p16_b[1] if p16_b else None, **kw)
        ops.adamw_clip_step(Pa, Ga, Ma, Va, p16_a[1] if p16_a else None, **kw, ema=E, ema_decay=0.9, **MODES[mode])
        assert _same_bits(Pa, Pb) and _same_bits(Ma, Mb) and _same_bits(Va, Vb), step       # the step itself: bit-equal to the old entry's
        assert float(Ga.abs().max()) == 0.0 and float(Gb.abs().max()) == 0.0
        if p16_a:
            assert _same_bits(p16_a[1], p16_b[1]), step
        d = R.decay_at(step, 0.9, MODES[mode]["ema_update_after_step"], MODES[mode]["ema_warmup"])
        ref = R.blend(ref, Pa, d)
        if d == 0.0:
            assert _same_bits(E, Pa), step                                                   # the EMA follows the weights bit for bit
        worst = max(worst, _check_ema(E, ref, Pa, step, f"ema_kernel[n={n},scalar={scalar},{mode}] step {step}"))
    assert mode == "follow" or not _same_bits(E, Pa)                                          # (the blend really happened)
    assert _guards_ok(bufs_a, n, off) and _guards_ok(bufs_b, n, off)                          # E's guard elements included
    if p16_a:
        c = p16_a[0].cpu().float()
        assert bool((c[:4 - off] == 7.0).all()) and bool((c[4 - off + n:] == 7.0).all())
    report(f"adamw_ema[n={n},scalar={scalar},p16={p16_dtype},decoupled={decoupled},{mode}]", worst_error_over_bound=worst)


def test_ema_entry_refuses_bad_settings_by_name(ops, dev):
    bufs, _ = _flat_bufs(8, False, dev, None, [torch.ones(8)] * 5)
    P, G, M, V, E = (b[1] for b in bufs)
    before = [t.clone() for t in (P, G, M, V, E)]
    kw = dict(HP, step=1, gscale=1.0, gnorm_sq=None, max_norm=0.0, decoupled=True, zero_grad=True, ema=E)
    for decay in (-0.5, 1.0, NAN):
        with pytest.raises(ValueError, match=r"ema_decay must be a number in \[0, 1\)"):
            ops.adamw_clip_step(P, G, M, V, None, **kw, ema_decay=decay)
    with pytest.raises(ValueError, match=r"ema_update_after_step must be an integer >= 0"):
        ops.adamw_clip_step(P, G, M, V, None, **kw, ema_decay=0.9, ema_update_after_step=-1)
    # the C entry itself refuses too (a caller that goes around ops), before any launch
    from open_musiclm_amd import hip
    args = [hip.ptr(t) for t in (P, G, M, V)] + [None, 8, 3e-3, 0.9, 0.99, 1e-8, 0.01, 1, 1.0, None, 0.0, 1, 1, 1, None, hip.ptr(E)]
    for tail, text in (((1.0, 0, 1), "ema_decay must lie in"), ((NAN, 0, 1), "ema_decay must lie in"), ((0.9, -1, 1), "ema_update_after_step must be")):
        with pytest.raises(RuntimeError, match=text):
            hip.call("omlm_adamw_clip_step_ema", *args, *tail, hip.stream_ptr())
    assert all(_same_bits(a, b) for a, b in zip(before, (P, G, M, V, E)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the clock and the skipped step
@pytest.mark.parametrize("scalar", [False, True])
def test_ema_runs_on_the_applied_step_clock_and_skips_with_the_step(ops, dev, scalar):
    """ls_state {S, good, skipped, applied = 5, S} with update_after_step 3: the step is applied step 6, so d = d(6) = 4/13, not
    d(step argument = 9) = 7/16; a non-finite norm leaves E, like P, M, V and P16, bit-unchanged and still clears G."""
    n, S = 4099, 1024.0
    g = _gen(60 + scalar)
    p0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    v0 = torch.rand(n, generator=g) * 1e-6
    e0 = p0 * (1.0 + 0.05 * torch.randn(n, generator=g))
    grad = _grads(n, g, (3.0,))[0]
    bufs, p16 = _flat_bufs(n, scalar, dev, torch.float16, [p0, grad * S, m0, v0, e0])
    (_, P), (_, G), (_, M), (_, V), (_, E) = bufs
    ls = torch.tensor([S, 1.0, 2.0, 5.0, S], device=dev)
    nsq = torch.zeros(1, device=dev)
    ops.sumsq_accumulate(G.clone(), nsq)
    kw = dict(HP, gscale=0.5, gnorm_sq=nsq, max_norm=1.0, decoupled=True, zero_grad=True, ls_state=ls, ema=E, ema_decay=0.9,
              ema_update_after_step=3, ema_warmup=True)
    ops.adamw_clip_step(P, G, M, V, p16[1], step=9, **kw)
    d6, d9 = R.decay_at(6, 0.9, 3, True), R.decay_at(9, 0.9, 3, True)
    assert d6 == R.f32(4.0 / 13.0) and d9 == R.f32(7.0 / 16.0)
    ratio = _check_ema(E, R.blend(e0, P, d6), P, 1, f"ema_clock[scalar={scalar}]")
    wrong = (E.double().cpu() - R.blend(e0, P, d9)).abs()
    assert float(wrong.max()) > 100 * float(R.bound(1, P, E).max())                          # (the two clocks are far apart at this bound)
    assert float(G.abs().max()) == 0.0 and ls.cpu().tolist() == [S, 1.0, 2.0, 5.0, S]
    for bad in (INF, NAN):
        before = [t.clone() for t in (E, P, M, V, p16[1])]
        G.copy_((grad * S).to(dev))
        nsq.fill_(bad)
        ops.adamw_clip_step(P, G, M, V, p16[1], step=10, **kw)
        assert all(_same_bits(a, b) for a, b in zip(before, (E, P, M, V, p16[1]))), bad
        assert float(G.abs().max()) == 0.0
    assert _guards_ok(bufs, n, 1 if scalar else 0)
    report(f"adamw_ema_clock[scalar={scalar}]", worst_error_over_bound=ratio)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. FusedAdam
SHAPES = [(5, 7), (3,), (16, 8), (1,), (9,), (2, 3, 4)]          # two weight-decay groups (ndim >= 2 / ndim < 2), odd sizes in 8-element granules
EMA_KW = dict(ema_decay=0.9, ema_update_after_step=2, ema_warmup=True)


def _plain_params(dev, seed=5):
    g = _gen(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]


def _step_grads(steps, seed=6):
    """Hand-written gradients: per step one tensor per parameter, alternately far above and below the clipping norm."""
    g = _gen(seed)
    return [[torch.randn(s, generator=g) * (3.0 if k % 2 == 0 else 1e-3) for s in SHAPES] for k in range(steps)]


def _feed_and_step(opt, params, grads):
    opt.zero_grad()
    for p, gr in zip(params, grads):
        p.grad.copy_(gr.to(p.device))
    opt.step(max_grad_norm=1.0, grad_scale=0.5)


def test_fused_adam_keeps_the_ema_and_leaves_the_step_alone(ops, dev):
    from open_musiclm_amd.optimizer import get_optimizer
    p_on, p_off = _plain_params(dev), _plain_params(dev)
    on, off = get_optimizer(p_on, lr=3e-3, wd=0.01, **EMA_KW), get_optimizer(p_off, lr=3e-3, wd=0.01)
    assert on.ema_enabled and not off.ema_enabled
    on.zero_grad()
    off.zero_grad()
    assert "E" not in off._flat and _same_bits(on.ema_flat, on.flat_param)                    # E starts as P
    # the parent's code path, spelled out on buffers of its own: the norm, then the old entry once per group
    f = off._flat
    Pm, Gm, Mm, Vm, P16m = (f[k].clone() for k in ("P", "G", "M", "V", "P16"))
    nsq, partials = torch.zeros(1, device=dev), torch.empty(2048, device=dev)
    ref, worst = on.flat_param.double().cpu(), 0.0
    for t, grads in enumerate(_step_grads(6), start=1):
        _feed_and_step(on, p_on, grads)
        off.zero_grad()
        for p, gr in zip(p_off, grads):
            p.grad.copy_(gr.to(dev))
        Gm.copy_(f["G"])
        off.step(max_grad_norm=1.0, grad_scale=0.5)
        nsq.zero_()
        ops.sumsq_accumulate(Gm, nsq, partials)
        for grp, (a, b) in zip(off.param_groups, f["ranges"]):
            ops.adamw_clip_step(Pm[a:b], Gm[a:b], Mm[a:b], Vm[a:b], P16m[a:b], lr=grp["lr"], beta1=grp["betas"][0], beta2=grp["betas"][1],
                                eps=grp["eps"], wd=grp["weight_decay"], step=t, gscale=0.5, gnorm_sq=nsq, max_norm=1.0,
                                decoupled=grp["decoupled"], zero_grad=True)
        for k, mine in (("P", Pm), ("M", Mm), ("V", Vm)):
            assert _same_bits(f[k], mine), (t, k)                                             # EMA off: the parent's launches, bit for bit
            assert _same_bits(on._flat[k], mine), (t, k)                                      # EMA on: the step itself is untouched
        d = R.decay_at(t, 0.9, 2, True)
        ref = R.blend(ref, on.flat_param, d)
        if d == 0.0:
            assert _same_bits(on.ema_flat, on.flat_param), t
        worst = max(worst, _check_ema(on.ema_flat, ref, on.flat_param, t, f"fused_adam_ema step {t}"))
    assert not _same_bits(on.ema_flat, on.flat_param)
    sd = on.state_dict()
    assert {k: sd["omlm_ema"][k] for k in ("decay", "update_after_step", "warmup")} == dict(decay=0.9, update_after_step=2, warmup=True)
    assert "omlm_ema" not in off.state_dict()
    for e, p, st in zip(sd["omlm_ema"]["params"], on._all_params(), sd["state"].values()):   # index order of `state`
        assert e.shape == p.shape == st["exp_avg"].shape
    report("fused_adam_ema", worst_error_over_bound=worst)


def test_fused_adam_ema_resumes_from_its_state_dict(dev, capsys):
    from open_musiclm_amd.optimizer import get_optimizer
    grads = _step_grads(5)
    p_a = _plain_params(dev)
    a = get_optimizer(p_a, lr=3e-3, wd=0.01, **EMA_KW)
    for gr in grads[:3]:
        _feed_and_step(a, p_a, gr)
    sd = a.state_dict()
    p_b = [torch.nn.Parameter(p.detach().clone()) for p in p_a]
    b = get_optimizer(p_b, lr=3e-3, wd=0.01, **EMA_KW)
    b.load_state_dict(sd)
    assert _same_bits(a.ema_flat, b.ema_flat) and not _same_bits(b.ema_flat, b.flat_param)
    # with the EMA off the key is ignored (the moments still arrive)
    p_d = [torch.nn.Parameter(p.detach().clone()) for p in p_a]
    d_ = get_optimizer(p_d, lr=3e-3, wd=0.01)
    d_.load_state_dict(sd)
    assert not d_.ema_enabled and "E" not in d_._flat and _same_bits(d_._flat["M"], a._flat["M"])
    for gr in grads[3:]:
        _feed_and_step(a, p_a, gr)
        _feed_and_step(b, p_b, gr)
    for k in ("E", "P", "M", "V"):
        assert _same_bits(a._flat[k], b._flat[k]), k
    # a state dict from before the EMA existed, loaded with the EMA on: E := P, said once
    p_c = [torch.nn.Parameter(p.detach().clone()) for p in p_a]
    c = get_optimizer(p_c, lr=3e-3, wd=0.01, **EMA_KW)
    c.zero_grad()
    c.ema_flat.add_(1.0)
    old = {k: v for k, v in sd.items() if k != "omlm_ema"}
    capsys.readouterr()
    c.load_state_dict(old)
    c.load_state_dict(old)
    assert _same_bits(c.ema_flat, c.flat_param)
    assert capsys.readouterr().out.count("carries no weight EMA") == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the twin
GEOM = dict(dim=128, depth=2, heads=2, attn_dropout=0.0, ff_dropout=0.0, num_coarse_quantizers=3, clap_codebook_size=64,
            semantic_codebook_size=64, acoustic_codebook_size=64)


def _coarse_ids(dev, seed, B=2):
    g = _gen(seed)
    return [torch.randint(0, 64, (B, 12), generator=g).to(dev), torch.randint(0, 64, (B, 9), generator=g).to(dev),
            torch.randint(0, 64, (B, 4, 3), generator=g).to(dev)]


def _fresh_from(sd, precision, dev):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(123)                                       # other initial weights: everything must come from sd
    m = M.create_coarse_transformer(**GEOM, precision=precision).to(dev)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()}, strict=True)
    return m.eval()


def _logits(model, ids):
    with torch.no_grad():
        return [None if t is None else t.clone() for t in model(all_token_ids=ids)]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_twin_serves_the_ema_to_forward_and_generate(dev, precision):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.ema import EmaTwin
    from open_musiclm_amd.optimizer import get_optimizer
    torch.manual_seed(0)
    model = M.create_coarse_transformer(**GEOM, precision=precision).to(dev)
    stage = M.CoarseStage(coarse_transformer=model, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0).train()
    opt = get_optimizer(model.parameters(), lr=3e-3, wd=0.01, ema_decay=0.5)
    opt.zero_grad()
    twin = EmaTwin(model, opt)
    keys = ("clap_token_ids", "semantic_token_ids", "coarse_token_ids")

    def train_step(seed):
        opt.zero_grad()
        loss = stage(**dict(zip(keys, _coarse_ids(dev, seed))), return_loss=True)[0]
        loss.backward()
        opt.mark_grads_dirty()
        opt.step(max_grad_norm=0.5)

    for k in range(3):
        train_step(10 + k)
    if precision == "fp16":
        assert opt.loss_scale_report()["applied_steps"] == 3
    E, P = opt.ema_flat, opt.flat_param
    assert not _same_bits(E, P)
    # state_dict: the model's keys, E's values
    sd = twin.state_dict()
    assert list(sd.keys()) == list(model.state_dict().keys())
    slot = {id(p): k for k, p in enumerate(opt._all_params())}
    for (name, mp), tp in zip(model.named_parameters(), twin.parameters()):
        o, n = opt._flat["offs"][slot[id(mp)]], opt._flat["sizes"][slot[id(mp)]]
        assert tp.data_ptr() == E.data_ptr() + 4 * o and _same_bits(sd[name], E[o:o + n].view(mp.shape)), name
        assert not tp.requires_grad and tp.grad is None and not hasattr(tp, "_omlm_bf16")
    assert not twin.training and all(p.requires_grad for p in model.parameters())
    # a FRESH model loaded from it computes what the twin computes, bit for bit
    ids = _coarse_ids(dev, 99)
    fresh = _fresh_from(sd, precision, dev)
    lt, lf, lm = _logits(twin, ids), _logits(fresh, ids), _logits(model.eval(), ids)
    model.train()
    assert all(torch.equal(a, b) for a, b in zip(lt, lf))
    assert not torch.equal(lt[-1], lm[-1])                        # (and not what the training weights compute)
    wt, wf = (M.TokenConditionedTransformerWrapper(transformer=m, unique_consecutive=False).eval() for m in (twin, fresh))
    U = torch.rand(9, 2, 65, generator=_gen(7))
    gen = lambda w: w.generate(conditioning_token_ids=ids[:2], max_time_steps=3, uniforms=U)
    out_t, out_f = gen(wt), gen(wf)
    assert out_t.shape == (2, 3, 3) and torch.equal(out_t, out_f)
    # one more step moves E under the twin: its cached operand images must go (a stale engine.prepared_weights fails here)
    train_step(20)
    lt2 = _logits(twin, ids)
    lf2 = _logits(_fresh_from(twin.state_dict(), precision, dev), ids)
    assert all(torch.equal(a, b) for a, b in zip(lt2, lf2)) and not torch.equal(lt2[-1], lt[-1])
    assert torch.equal(gen(wt), gen(M.TokenConditionedTransformerWrapper(
        transformer=_fresh_from(twin.state_dict(), precision, dev), unique_consecutive=False).eval()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the trainer
def _trainer(dev, folder, **kw):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.data import SyntheticTokenDataset
    from open_musiclm_amd.trainer import SingleStageTrainer
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=128, depth=2, heads=2, num_coarse_quantizers=3, ff_dropout=0.1, precision="bf16").to(dev)
    ds = SyntheticTokenDataset("coarse", length=8, coarse_window_seconds=1, semantic_window_seconds=2)
    return SingleStageTrainer(model, "coarse", num_train_steps=4, batch_size=2, dataset=ds, lr=3e-3, lr_warmup=0, grad_accum_every=1,
                              wd=0.01, max_grad_norm=0.5, valid_frac=0.0, save_results_every=1000, save_model_every=1,
                              results_folder=str(folder), save_predicted_tokens=False, save_reconstructed_wave=False, **kw)


def test_trainer_checkpoints_and_generates_from_the_ema(dev, tmp_path):
    from open_musiclm_amd import open_musiclm as M
    tr = _trainer(dev, tmp_path / "on", ema_decay=0.5)
    plain = _trainer(dev, tmp_path / "off")
    assert plain.ema_transformer is None and not plain.optim.ema_enabled
    logs = tr.train_step()
    assert np.isfinite(logs["loss"])
    twin = tr.ema_transformer
    assert twin is not None and twin is not tr.transformer
    # the twin is no registered submodule: the trainer's parameters and state_dict are those of a trainer without it
    twin_ids = {id(p) for p in twin.parameters()}
    twin_ptrs = {p.data_ptr() for p in twin.parameters()}
    assert not any(id(p) in twin_ids or p.data_ptr() in twin_ptrs for p in tr.parameters())
    assert list(tr.state_dict().keys()) == list(plain.state_dict().keys())
    assert len(list(tr.parameters())) == len(list(plain.parameters()))
    # the checkpoint beside the model's
    path = tmp_path / "on" / "coarse.transformer_ema.0.pt"
    assert path.exists() and (tmp_path / "on" / "coarse.transformer.0.pt").exists()
    assert not (tmp_path / "off" / "coarse.transformer_ema.0.pt").exists()
    torch.manual_seed(5)
    fresh = M.create_coarse_transformer(dim=128, depth=2, heads=2, num_coarse_quantizers=3, ff_dropout=0.1, precision="bf16").to(dev)
    fresh.load_state_dict(torch.load(str(path), map_location=dev), strict=True)
    for (k, a), b in zip(fresh.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b), k
    # generate / validate on the twin
    g = _gen(3)
    kw = dict(clap_token_ids=torch.randint(0, 1024, (2, 12), generator=g).to(dev),
              semantic_token_ids=torch.randint(0, 1024, (2, 9), generator=g).to(dev), max_time_steps=2)
    out = tr.generate(use_ema=True, **kw)
    assert out.shape == (2, 2, 3) and tr.generate(**kw).shape == (2, 2, 3)
    vl, va = tr.validate(0, use_ema=True)
    assert np.isfinite(vl) and 0.0 <= va <= 1.0 and not twin.training
    for call in (lambda: plain.generate(use_ema=True, **kw), lambda: plain.validate(0, use_ema=True)):
        with pytest.raises(ValueError, match="keeps no weight EMA"):
            call()
    # the optimizer file alone resumes the EMA; ema_path reads the twin's own file
    tr.train_step()
    E1 = tr.optim.ema_flat.clone()
    files = [str(tmp_path / "on" / f"coarse.{n}.1.pt") for n in ("transformer", "optimizer", "scheduler", "transformer_ema")]
    assert all(os.path.exists(f) for f in (files[0], files[1], files[3]))
    tr.optim.ema_flat.zero_()
    tr.load(files[0], files[1])
    assert _same_bits(tr.optim.ema_flat, E1)
    tr.optim.ema_flat.zero_()
    tr.load(files[0], files[1], ema_path=str(path))              # the EMA of step 0 over the one the optimizer file restored
    for (k, a), b in zip(fresh.state_dict().items(), tr.ema_transformer.state_dict().values()):
        assert torch.equal(a, b), k
    assert np.isfinite(tr.train_step()["loss"])
