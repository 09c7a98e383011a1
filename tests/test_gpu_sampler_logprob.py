"""GPU: the log-probabilities of the sampled id -- the LP = true instantiations of sample_kernel / sample_wide_kernel behind
omlm_sample_lp (include/omlm.h; csrc/sampler.hip), ops.sample(lp_model=, lp_sampled=), decode.SamplingLoop(logprobs=True),
generate(return_logprobs=True) and score().

Against the fp64 restatement (tests/sampler_logprob_ref.py), whose docstring derives the tolerance and the bracket that the nucleus'
fixed-point cut needs; tests/test_sampler_logprob_host.py shows the bracket is a point on more than 90 % of the rows compared here.
Everything that compares the kernels with themselves (ids with and without the pointers, stream against buffer, step_dev form, two
launches, eager against graph) is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loss_optim_sampler_ref as R
import sampler_logprob_ref as L
import sampler_stream_ref as S
import sampler_top_p_ref as P
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_model import TOL, build_from_golden

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
SEED = 0x9E3779B97F4A7C15
SENTINEL = 7.0                                          # no log-probability is positive
PS = [1.0, 0.5, 0.9, 0.999]


def _pad(x, dev, extra=9):
    """[B, V] -> [B, ld] on the device, ld > V, NaN in the padding."""
    B, V = x.shape
    out = torch.full((B, (V + 7) // 8 * 8 + extra), NAN)
    out[:, :V] = x
    return out.to(dev)


def _ids(dev, B):
    return torch.full((B,), -7, dtype=torch.long, device=dev)


def _lp(dev, *shape):
    return torch.full(shape, SENTINEL, device=dev)


def _p(p):
    return None if p >= 1.0 else p


def _sample(ops, dev, lg, V, k, T, forbid, **kw):
    out = _ids(dev, lg.shape[0])
    ops.sample(lg, out, V, k, T, forbid, **kw)
    return out


def _sample_lp(ops, dev, lg, V, k, T, forbid, **kw):
    B = lg.shape[0]
    out, pm, ps = _ids(dev, B), _lp(dev, B), _lp(dev, B)
    ops.sample(lg, out, V, k, T, forbid, lp_model=pm, lp_sampled=ps, **kw)
    return out, pm, ps


def _close(got, want, bound):
    """-inf where the restatement has -inf and nowhere else; elsewhere |got - want| <= bound.  Returns the worst excess ratio."""
    got, want = got.double(), want.double()
    dead = want == -INF
    assert torch.equal(got == -INF, dead), (got[dead != (got == -INF)][:5].tolist(), want[dead != (got == -INF)][:5].tolist())
    live = ~dead
    if not bool(live.any()):
        return 0.0
    assert bool(torch.isfinite(got[live]).all())
    return float(((got - want).abs()[live] / bound[live]).max())


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", P.COMPARE_V)
def test_logprobs_against_fp64(ops, dev, V):
    x, u = P.compare_rows(V)
    lg, ud = _pad(x, dev), u.to(dev)
    rdev = dev if V >= 1024 else torch.device("cpu")     # the restatement runs in fp64 where the rows are (the GPU for the long ones)
    xr = x.to(rdev)
    worst_m = worst_s = 0.0
    cases = loose = 0
    for k in P.compare_ks(V):
        for forbid in (False, True):
            rk = P.Ranked(xr, k, forbid)
            m = L.largest_kept(xr, forbid)
            for T in (0.4, 1.0):
                for p in PS:
                    plain = _sample(ops, dev, lg, V, k, T, forbid, top_p=_p(p), uniform=ud)
                    ids, pm, ps = _sample_lp(ops, dev, lg, V, k, T, forbid, top_p=_p(p), uniform=ud)
                    assert torch.equal(ids, plain), (V, k, forbid, T, p)
                    ids, pm, ps = ids.to(rdev), pm.to(rdev), ps.to(rdev)
                    ls = xr.double().gather(1, ids[:, None])[:, 0]
                    em = _close(pm, L.lp_model(xr, ids, forbid), L.tol(ls, m, 1.0))
                    print(f"V={V} k={k} forbid={forbid} T={T} p={p}: lp_model error / tol {em:.3f}", end="")
                    assert em <= 1.0, (V, k, forbid, T, p, em)
                    bound = L.tol(ls, m, T)
                    if p >= 1.0:
                        es = _close(ps, L.lp_sampled(xr, ids, k, T, 1.0, forbid), bound)
                    else:
                        lo, hi, same = L.bracket(xr, ids, k, T, p, forbid, ranked=rk)
                        dead = lo == -INF
                        assert torch.equal(ps == -INF, dead) and torch.equal(hi == -INF, dead)
                        live = ~dead
                        over = torch.maximum(lo - ps.double(), ps.double() - hi)[live] / bound[live]      # <= 0 inside the bracket
                        es = float(over.max()) if bool(live.any()) else 0.0
                        loose += int((~same & live).sum())
                    print(f", lp_sampled excess / tol {es:.3f}")
                    assert es <= 1.0, (V, k, forbid, T, p, es)
                    worst_m, worst_s, cases = max(worst_m, em), max(worst_s, es), cases + 1
    report(f"sampler_logprob_fp64[V={V}]", cases=cases, worst_model_over_tol=worst_m, worst_sampled_over_tol=worst_s, rows_with_a_bracket=loose)


# ---- 2. exact zeros ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 1025, 2049, 8193])
def test_one_entry_sets_give_exactly_zero(ops, dev, V):
    g = torch.Generator().manual_seed(V)
    B = 8
    x = torch.randn(B, V, generator=g) * 4
    x[1] = torch.randint(0, 4, (V,), generator=g).float()                    # ties at the maximum: one of them is kept
    lg, ud = _pad(x, dev), torch.rand(B, V, generator=g).to(dev)
    zero = torch.zeros(B, device=dev)
    forbids = (False,) if V == 1 else (False, True)
    for forbid in forbids:
        for src in (dict(uniform=ud), dict(seed=SEED, step=3)):
            for T in (0.4, 1.0):
                for p in (None, 0.9):                                        # k = 1
                    ids, pm, ps = _sample_lp(ops, dev, lg, V, 1, T, forbid, top_p=p, **src)
                    assert torch.equal(ps, zero), (V, forbid, T, p, ps.tolist())
                    assert bool((pm <= 0).all()) and bool(torch.isfinite(pm).all())
                for k in sorted({max(int(0.1 * V), 1), V}):                 # a tiny nucleus
                    ids, pm, ps = _sample_lp(ops, dev, lg, V, k, T, forbid, top_p=1e-6, **src)
                    assert torch.equal(ps, zero), (V, forbid, T, k, ps.tolist())
                    if V > 1:
                        want = R._forbid(x, forbid).argmax(1)
                        assert ids.cpu().tolist() == want.tolist()
    if V == 1:                                                               # V = 1: the model's distribution has one entry too
        ids, pm, ps = _sample_lp(ops, dev, lg, 1, 1, 1.0, False, uniform=ud)
        assert torch.equal(pm, zero) and torch.equal(ps, zero) and ids.tolist() == [0] * B
        ids, pm, ps = _sample_lp(ops, dev, lg, 1, 1, 1.0, True, uniform=ud)   # forbidden: the "id 0" rule, both -inf
        assert ids.tolist() == [0] * B and bool((pm == -INF).all()) and bool((ps == -INF).all())


# ---- 3. the counter stream against the buffer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2049, 8193])
def test_stream_form_equals_buffer_form(ops, dev, V):
    B, row0, step = 5, 3, 2
    k, T = max(int(0.1 * V), 1), 0.9
    g = torch.Generator().manual_seed(V + 1)
    U = torch.from_numpy(S.uniforms(SEED, step + 1, B, V, row0=row0)).to(dev)
    x = torch.randn(B, V, generator=g) * 4
    x[1] = torch.randint(0, 4, (V,), generator=g).float()
    lg = _pad(x, dev)
    for p in (1.0, 0.9):
        for forbid in (False, True):
            a = _sample_lp(ops, dev, lg, V, k, T, forbid, top_p=_p(p), uniform=U[step])
            b = _sample_lp(ops, dev, lg, V, k, T, forbid, top_p=_p(p), seed=SEED, step=step, row0=row0)
            for got, want in zip(b, a):
                assert torch.equal(got, want), (V, p, forbid, got.tolist(), want.tolist())
            assert bool((a[1] < 0).all()) and bool((a[2] <= 0).all())


# ---- 4. the step_dev form, with the embedding gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2049])
def test_step_dev_form_writes_its_own_row(ops, dev, V):
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    B, steps, D, row0 = 6, 2, 64, 2
    k, T = max(int(0.1 * V), 1), 0.95
    g = torch.Generator().manual_seed(V)
    U = torch.rand(steps, B, V, generator=g).to(dev)
    E = V + 3
    emb = torch.randn(E, D, generator=g).to(dev)
    for p in (1.0, 0.9):
        for rng in (False, True):
            src = dict(seed=SEED, row0=row0) if rng else dict(uniform=U)
            step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            pm, ps = _lp(dev, steps, B), _lp(dev, steps, B)
            hw, hg = (torch.full((steps, B), -7, dtype=torch.long, device=dev) for _ in range(2))
            for t in range(steps):
                lg = _pad(torch.randn(B, V, generator=g) * 4, dev)
                want, got = _ids(dev, B), _ids(dev, B)
                xw, xg = torch.full((B, D), NAN, device=dev), torch.full((B, D), NAN, device=dev)
                ops.sample(lg, want, V, k, T, True, top_p=_p(p), step_dev=step_dev, hist=hw, emb_table=emb, emb_row_offset=7, x=xw, **src)
                ops.sample(lg, got, V, k, T, True, top_p=_p(p), step_dev=step_dev, hist=hg, emb_table=emb, emb_row_offset=7, x=xg,
                           lp_model=pm, lp_sampled=ps, **src)
                assert torch.equal(got, want) and torch.equal(xg, xw) and torch.equal(xg, emb[(want + 7).clamp(0, E - 1)]), (V, p, rng, t)
                # this step's row is what the plain [B] form gives for the same draw; the later rows still hold the sentinel
                one = dict(seed=SEED, row0=row0, step=t) if rng else dict(uniform=U[t])
                ids1, pm1, ps1 = _sample_lp(ops, dev, lg, V, k, T, True, top_p=_p(p), **one)
                assert torch.equal(ids1, want) and torch.equal(pm[t], pm1) and torch.equal(ps[t], ps1), (V, p, rng, t)
                assert bool((pm[t + 1:] == SENTINEL).all()) and bool((ps[t + 1:] == SENTINEL).all())
                assert bool((pm[:t + 1] < 0).all()) and bool((ps[:t + 1] <= 0).all())
                if t < steps - 1:
                    kept = (pm[t].clone(), ps[t].clone())
                    call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())
            assert torch.equal(pm[0], kept[0]) and torch.equal(ps[0], kept[1])      # the second step left the first row alone
            assert torch.equal(hg, hw)


# ---- 5. pointers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2049])
def test_either_pointer_may_be_null(ops, dev, V):
    from open_musiclm_amd.hip import call, stream_ptr
    B = 6
    k, T = max(int(0.1 * V), 1), 0.8
    g = torch.Generator().manual_seed(V + 5)
    lg, ud = _pad(torch.randn(B, V, generator=g) * 4, dev), torch.rand(B, V, generator=g).to(dev)
    for p in (1.0, 0.9):
        ids, pm, ps = _sample_lp(ops, dev, lg, V, k, T, True, top_p=_p(p), uniform=ud)
        a, only_m = _ids(dev, B), _lp(dev, B)
        ops.sample(lg, a, V, k, T, True, top_p=_p(p), uniform=ud, lp_model=only_m)
        b, only_s = _ids(dev, B), _lp(dev, B)
        ops.sample(lg, b, V, k, T, True, top_p=_p(p), uniform=ud, lp_sampled=only_s)
        assert torch.equal(a, ids) and torch.equal(b, ids) and torch.equal(only_m, pm) and torch.equal(only_s, ps), (V, p)
        # both NULL: omlm_sample
        ld = lg.shape[1]
        c, d = _ids(dev, B), _ids(dev, B)
        for out, name, extra in ((c, "omlm_sample", ()), (d, "omlm_sample_lp", (None, None))):
            args = ops.SampleArgs(lg.data_ptr(), B, V, ld, ud.data_ptr(), 0, 0, 0, 0, None, out.data_ptr(), None, k, T, p, 1)
            call(name, ctypes.addressof(args), *extra, stream_ptr())
        assert torch.equal(c, ids) and torch.equal(d, ids), (V, p)


def test_bad_top_p_is_still_refused_by_name_before_any_launch(ops, dev):
    from open_musiclm_amd.hip import call, stream_ptr
    lg, out, pm = torch.zeros(2, 64, device=dev), _ids(dev, 2), _lp(dev, 2)
    for bad in (0.0, -1.0, 1.5, NAN):
        with pytest.raises(ValueError, match="top_p"):
            ops.sample(lg, out, 64, 8, 1.0, False, top_p=bad, seed=1, lp_model=pm)
        a = ops.SampleArgs(lg.data_ptr(), 2, 64, 64, None, 1, 0, 0, 0, None, out.data_ptr(), None, 8, 1.0, bad, 0)
        with pytest.raises(RuntimeError, match="top_p"):
            call("omlm_sample_lp", ctypes.addressof(a), pm.data_ptr(), None, stream_ptr())
    with pytest.raises(ValueError, match="lp_model"):                        # a buffer of the wrong type is refused by name too
        ops.sample(lg, out, 64, 8, 1.0, False, seed=1, lp_model=torch.zeros(2, dtype=torch.float64, device=dev))
    assert out.tolist() == [-7, -7] and pm.tolist() == [SENTINEL, SENTINEL]


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 8193])
def test_two_launches_give_the_same_bits(ops, dev, V):
    x, u = P.compare_rows(16384)
    lg, ud = _pad(x[:, :V].contiguous(), dev), u[:, :V].contiguous().to(dev)
    for p in (1.0, 0.5, 0.9):
        for k in (max(int(0.1 * V), 1), V):
            a = _sample_lp(ops, dev, lg, V, k, 0.8, True, top_p=_p(p), uniform=ud)
            b = _sample_lp(ops, dev, lg, V, k, 0.8, True, top_p=_p(p), uniform=ud)
            for got, want in zip(b, a):
                assert torch.equal(got, want), (V, p, k)


# ---- 7. generate(return_logprobs=True) -----------------------------------------------------------------------------------------------
def _tiny_coarse(golden_dir, dev, precision):
    from open_musiclm_amd import open_musiclm as M
    z = np.load(os.path.join(golden_dir, "tiny_coarse_generate.npz"))
    _, model = build_from_golden(golden_dir, "tiny_coarse", dev, precision)
    model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
    model.eval()
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    cond = [torch.from_numpy(z["cond.0"]).to(dev), torch.from_numpy(z["cond.1"]).to(dev)]
    return wrapper, cond, float(z["temperature"])


def _prefix_logits(wrapper, cond, flat):
    """[n, B, V1] fp32: transformer.last_logits of every prefix of flat [B, n], with generate's conditioning."""
    from open_musiclm_amd.utils import append_eos_id
    model = wrapper.transformer
    V1 = model.token_sequences[-1].codebook_size + 1
    condx = [append_eos_id(t.reshape(t.shape[0], -1).long(), e) for t, e in zip(cond, wrapper.eos_ids)]
    with torch.no_grad():
        return torch.stack([model.last_logits(condx + [flat[:, :j]])[:, :V1].clone() for j in range(flat.shape[1])])


def _check_against_prefix_logits(wrapper, cond, ids, lps, T, p, precision, what):
    """model against score(ids) and the fp64 log-softmax of the re-forward logits, sampled against the restatement on those logits:
    within 2 TOL[precision]["logits"] max|logit| (the bar of cached against re-forward logits; the log-sum-exp is 1-Lipschitz in the
    sup norm) + tol."""
    B, steps, Q = ids.shape
    V1 = wrapper.transformer.token_sequences[-1].codebook_size + 1
    k = max(int((1 - 0.9) * V1), 1)
    flat = ids.reshape(B, -1)
    lg = _prefix_logits(wrapper, cond, flat)                                 # [n, B, V1]
    slack = 2 * TOL[precision]["logits"] * float(lg.abs().max())
    sc = wrapper.score(conditioning_token_ids=cond, pred_token_ids=ids)
    assert sc.shape == ids.shape and sc.dtype == torch.float32
    worst = dict(model_vs_score=0.0, model=0.0, sampled=0.0)
    for j in range(flat.shape[1]):
        x, s = lg[j], flat[:, j]
        ls = x.double().gather(1, s[:, None])[:, 0]
        m = L.largest_kept(x, True)
        got_m, got_s = lps.model.reshape(B, -1)[:, j].double(), lps.sampled.reshape(B, -1)[:, j].double()
        em = float(((got_m - sc.reshape(B, -1)[:, j].double()).abs() / (slack + L.tol(ls, m, 1.0))).max())
        ef = float(((got_m - L.lp_model(x, s, True)).abs() / (slack + L.tol(ls, m, 1.0))).max())
        bound = slack + L.tol(ls, m, T)
        if p is None:
            es = float(((got_s - L.lp_sampled(x, s, k, T, 1.0, True)).abs() / bound).max())
        else:
            lo, hi, _ = L.bracket(x, s, k, T, p, True)
            es = float((torch.maximum(lo - got_s, got_s - hi) / bound).max())
        worst = dict(model_vs_score=max(worst["model_vs_score"], em), model=max(worst["model"], ef), sampled=max(worst["sampled"], es))
    print(f"{what}: slack {slack:.2e}; worst error / bound: model against score {worst['model_vs_score']:.3f}, model against fp64 "
          f"{worst['model']:.3f}, sampled {worst['sampled']:.3f}")
    report(f"generate_logprobs[{what}]", slack=slack, **worst)
    assert max(worst.values()) <= 1.0, (what, worst)


@pytest.mark.parametrize("top_p", [None, 0.9])
@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_generate_returns_logprobs(golden_dir, dev, precision, top_p):
    """The tiny golden coarse model (V1 = 41, Q = 3, B = 2), 6 time steps = 18 ids (the graph loop captures at id 3 and replays to id
    11): cached eager, cached captured graph and the re-forward route, both sources of uniforms."""
    from open_musiclm_amd import open_musiclm as M
    wrapper, cond, T = _tiny_coarse(golden_dir, dev, precision)
    steps, Q, V1 = 6, 3, 41
    U = torch.rand(steps * Q, 2, V1, generator=torch.Generator().manual_seed(11))
    for name, src in (("buffer", dict(uniforms=U)), ("counter", dict(sampler_rng="counter", sampler_seed=SEED))):
        gen = lambda **k: wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, top_p=top_p, **src, **k)  # noqa: E731
        results = {}
        for route, kw in (("cached", dict(use_cache=True)), ("graph", dict(use_cache=True, use_graph=True)), ("uncached", dict(use_cache=False))):
            plain = gen(**kw)
            ids, lps = gen(return_logprobs=True, **kw)
            assert isinstance(lps, M.LogProbs) and torch.equal(ids, plain), (route, name)
            for v in lps:
                assert v.shape == (2, steps, Q) and v.dtype == torch.float32 and v.device == ids.device
            assert bool((lps.sampled <= 0).all()) and bool((lps.model <= 0).all()) and bool(torch.isfinite(lps.model).all())
            results[route] = (ids, lps)
            _check_against_prefix_logits(wrapper, cond, ids, lps, T, top_p, precision, f"{precision},top_p={top_p},{name},{route}")
        (ia, la), (ig, lgr) = results["cached"], results["graph"]
        assert torch.equal(ia, ig) and torch.equal(la.model, lgr.model) and torch.equal(la.sampled, lgr.sampled), name
    # ids this call sampled, not the supplied ones: a primed call returns max_time_steps - first_step rows
    ids, lps = wrapper.generate(conditioning_token_ids=cond, pred_token_ids=results["cached"][0][:, :2], max_time_steps=steps, temperature=T,
                                top_p=top_p, return_logprobs=True, sampler_rng="counter", sampler_seed=SEED)
    assert ids.shape == (2, steps, Q) and lps.model.shape == (2, steps - 2, Q) and lps.sampled.shape == (2, steps - 2, Q)


@pytest.mark.parametrize("top_p", [None, 0.9])
def test_generate_returns_logprobs_over_two_decode_groups(golden_dir, dev, top_p):
    """19 samples: more than one decode call holds."""
    from open_musiclm_amd import decode
    precision = "fp16ff"
    wrapper, cond2, T = _tiny_coarse(golden_dir, dev, precision)
    B, steps, Q = 19, 3, 3
    assert decode.max_call_batch(wrapper.transformer, precision) < B
    g = torch.Generator().manual_seed(17)
    cond = [torch.randint(0, int(c.max()) + 1, (B,) + tuple(c.shape[1:]), generator=g).to(dev) for c in cond2]
    for src in (dict(uniforms=torch.rand(steps * Q, B, 41, generator=g)), dict(sampler_rng="counter", sampler_seed=SEED)):
        gen = lambda **k: wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, top_p=top_p, **src, **k)  # noqa: E731
        plain = gen()
        ids, lps = gen(return_logprobs=True)
        assert torch.equal(ids, plain) and lps.model.shape == (B, steps, Q) and lps.sampled.shape == (B, steps, Q)
        assert bool((lps.sampled <= 0).all()) and bool((lps.model <= 0).all())
        _check_against_prefix_logits(wrapper, cond, ids, lps, T, top_p, precision, f"19 samples,top_p={top_p},{'buffer' if 'uniforms' in src else 'counter'}")


def test_stages_pass_the_flag_through(golden_dir, dev):
    from open_musiclm_amd import open_musiclm as M
    wrapper, cond, T = _tiny_coarse(golden_dir, dev, "bf16x3")
    stage = M.CoarseStage(coarse_transformer=wrapper.transformer)
    kw = dict(clap_token_ids=cond[0], semantic_token_ids=cond[1], max_time_steps=2, temperature=T, sampler_rng="counter", sampler_seed=5)
    plain = stage.generate(**kw)
    ids, lps = stage.generate(return_logprobs=True, **kw)
    assert torch.equal(ids, plain) and isinstance(lps, M.LogProbs) and lps.model.shape == ids.shape


# ---- 8. score() ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
@pytest.mark.parametrize("name", ["tiny_coarse", "tiny_fine_allweights"])
def test_score_against_fp64_log_softmax_of_every_prefix(golden_dir, dev, name, precision):
    from open_musiclm_amd import open_musiclm as M
    z, model = build_from_golden(golden_dir, name, dev, precision)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    nseq = len(model.token_sequences)
    cond = [torch.from_numpy(z[f"ids.{i}"]).to(dev) for i in range(nseq - 1)]
    seq = model.token_sequences[-1]
    B, Q, V1, steps = cond[0].shape[0], seq.num_quantizers, seq.codebook_size + 1, 3
    pred = torch.randint(0, V1, (B, steps, Q), generator=torch.Generator().manual_seed(3)).to(dev)      # the eos id among them
    pred[0, 1, 0] = V1 - 1
    was_training = wrapper.training
    got = wrapper.score(conditioning_token_ids=cond, pred_token_ids=pred)
    assert got.shape == (B, steps, Q) and got.dtype == torch.float32 and got.device == pred.device and wrapper.training == was_training
    lg = _prefix_logits(wrapper, cond, pred.reshape(B, -1)).double()        # [n, B, V1]
    want = torch.log_softmax(lg, dim=-1).gather(2, pred.reshape(B, -1).t()[:, :, None])[:, :, 0].t().reshape(B, steps, Q)
    ls = lg.gather(2, pred.reshape(B, -1).t()[:, :, None])[:, :, 0].t().reshape(B, steps, Q)
    m = lg.max(dim=-1).values.t().reshape(B, steps, Q)
    bound = 2 * TOL[precision]["logits"] * float(lg.abs().max()) + L.tol(ls, m, 1.0)
    err = float(((got.double() - want).abs() / bound).max())
    print(f"score[{name},{precision}]: worst error / bound {err:.3f} (largest |error| {float((got.double() - want).abs().max()):.2e})")
    report(f"score[{name},{precision}]", worst_over_bound=err)
    assert err <= 1.0, err
    for bad in (V1, -1):
        ids = pred.clone()
        ids[1, 2, Q - 1] = bad
        with pytest.raises(ValueError, match="pred_token_ids"):
            wrapper.score(conditioning_token_ids=cond, pred_token_ids=ids)
    assert wrapper.score(conditioning_token_ids=cond, pred_token_ids=pred[:, :0]).shape == (B, 0, Q)
