"""The wide decode call on the GPU: omlm_decode_step with 17..64 samples (up to four groups of 16 carried through one launch of every
matrix-core step kernel), generate()'s routing onto it, and MusicLM.forward(fine_windows_together=True).

Every model is dim 1024 (the only width the wide route exists at) with depth 2 unless stated; prompts are 55 rows with 9 teacher-forced
ids, as in test_gpu_model.test_cached_decode_at_full_width."""
import ast
import os

import numpy as np
import pytest
import torch

from test_gpu_model import TOL, relerr, report

pytestmark = pytest.mark.gpu

V1 = 1025
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _coarse(dev, precision, heads=8):
    """One dim-1024 depth-2 coarse model per (precision, heads), shared by the tests of this file and never modified."""
    from open_musiclm_amd import open_musiclm as M
    key = (precision, heads)
    if key not in _MODELS:
        torch.manual_seed(0)
        m = M.create_coarse_transformer(dim=1024, depth=2, heads=heads, ff_dropout=0.0, num_coarse_quantizers=3, precision=precision).to(dev)
        m.eval()
        _MODELS[key] = (m, M.TokenConditionedTransformerWrapper(transformer=m, unique_consecutive=False))
    return _MODELS[key]


def _prompt(wrapper, dev, B, n=9, seed=3):
    from open_musiclm_amd.utils import append_eos_id
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(0, 1024, (B, 12, 1), generator=g), torch.randint(0, 1024, (B, 40), generator=g)]
    flat = torch.randint(0, 1024, (B, n), generator=g)
    condx = [append_eos_id(t.reshape(B, -1).long(), e) for t, e in zip(cond, wrapper.eos_ids)]
    rows = sum(t.shape[-1] + 1 for t in condx) + 1 + n
    return [t.to(dev) for t in condx], flat.to(dev), rows


def _wide_steps(model, condx, flat, rows, precision, B):
    """prefill + (n - 1) teacher-forced steps of a wide decoder: the list of [B, V1] logits (clones)."""
    from open_musiclm_amd import decode
    dec = decode.CachedDecoder(model, B, rows, precision, wide=True)
    got = [dec.prefill(condx + [flat[:, :0]])[:, :V1].clone()]
    for k in range(flat.shape[1] - 1):
        got.append(dec.step(flat[:, k].contiguous(), k)[:, :V1].clone())
    return dec, got


@pytest.mark.parametrize("precision,B,heads", [("bf16", 17, 8), ("fp16", 24, 8), ("fp16ff", 17, 8), ("fp16ff", 40, 8), ("fp16ff", 64, 8),
                                               ("bf16", 64, 16)])
def test_wide_steps_match_the_reforward(dev, precision, B, heads):
    """CachedDecoder(wide=True): prefill + 8 steps against model.last_logits of the growing sequence, worst relative error over all
    samples under the mode's own bar.  A one-sample tail (17), an eight-sample tail (24), 16 + 16 + 8 (40), a full call (64) and the
    72-tile QKV grid of 16 heads."""
    from open_musiclm_amd import decode
    model, wrapper = _coarse(dev, precision, heads)
    assert decode.supports(model, B, precision, wide=True) and not decode.supports(model, B, precision)
    condx, flat, rows = _prompt(wrapper, dev, B)
    with torch.no_grad():
        dec, got = _wide_steps(model, condx, flat, rows, precision, B)
        want = [model.last_logits(condx + [flat[:, :k]])[:, :V1].clone() for k in range(flat.shape[1])]
    assert dec.planes == (precision == "fp16ff")
    per_step = [relerr(x, y) for x, y in zip(got, want)]
    per_group = [max(relerr(x[g0:g0 + 16], y[g0:g0 + 16], floor=float(y.abs().max())) for x, y in zip(got, want)) for g0 in range(0, B, 16)]
    err = max(per_step)
    print(f"wide steps vs re-forward [{precision}, B={B}, H={heads}]: max rel err {err:.3e} per group {per_group}")
    report(f"decode_wide_vs_reforward[{precision},B={B},H={heads}]", max_rel_err=err, per_group=per_group, steps=len(got))
    assert int(dec.splitk_cnt.abs().sum()) == 0                  # every ticket counter is zero again
    assert err < TOL[precision]["logits"], (err, per_group)


def test_wide_steps_match_the_oracle(dev):
    """fp16ff, B = 40: the same loop against the CPU oracle's forward of the teacher-forced sequence, for the first and last sample of
    each group (0, 16, 31, 32, 39)."""
    from oracle import musiclm_oracle as O
    precision, B = "fp16ff", 40
    model, wrapper = _coarse(dev, precision)
    spec = O.coarse_spec(dim=1024, depth=2, heads=8)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    condx, flat, rows = _prompt(wrapper, dev, B)
    sel = [0, 16, 31, 32, 39]
    with torch.no_grad():
        _, got = _wide_steps(model, condx, flat, rows, precision, B)
        o = O.token_conditioned_forward(sd, spec, [t[sel].cpu() for t in condx] + [flat[sel].cpu()[:, :flat.shape[1] - 1]], only_final=True)[-1]
    worst = max(relerr(lg[sel], o[:, i]) for i, lg in enumerate(got))
    print(f"wide steps vs oracle [fp16ff, B=40]: max rel err {worst:.3e}")
    report("decode_wide_vs_oracle[fp16ff,B=40]", max_rel_err=worst, samples=sel)
    assert worst < TOL["fp16ff"]["logits"], worst


@pytest.mark.parametrize("precision", ["fp16", "fp16ff"])
def test_a_group_is_a_16_sample_call(dev, precision):
    """After a wide prefill at B = 40, the state of samples 16..31 goes into a CachedDecoder of 16 and that of samples 32..39 into one of
    8; all three step with the same ids.  The wide logits of those rows equal the small decoders' bit for bit over three consecutive
    steps (the scratch has been reused by then): a group takes the branches and the summation order of a call of its own sample count,
    and no partial-sum region, slab or counter is shared between groups."""
    from open_musiclm_amd import decode
    B = 40
    model, wrapper = _coarse(dev, precision)
    condx, flat, rows = _prompt(wrapper, dev, B, n=4)
    with torch.no_grad():
        wide = decode.CachedDecoder(model, B, rows, precision, wide=True)
        wide.prefill(condx + [flat[:, :0]])
        parts = []
        for b0, b1 in ((16, 32), (32, 40)):
            small = decode.CachedDecoder(model, b1 - b0, rows, precision)
            assert small.planes == wide.planes == (precision == "fp16ff")
            for l in range(wide.L):
                small.Kc[l].copy_(wide.Kc[l][b0:b1])
                small.Vc[l].copy_(wide.Vc[l][b0:b1])
                small.hist[l].copy_(wide.hist[l][b0:b1])
            small.rows = wide.rows
            small.pos_dev.copy_(wide.pos_dev)
            parts.append((b0, b1, small))
        for k in range(3):
            lw = wide.step(flat[:, k].contiguous(), k).clone()
            for b0, b1, small in parts:
                ls = small.step(flat[b0:b1, k].contiguous(), k)
                assert torch.isfinite(ls).all()
                assert torch.equal(lw[b0:b1, :V1], ls[:, :V1]), (precision, k, b0, float((lw[b0:b1, :V1] - ls[:, :V1]).abs().max()))
        for l in range(wide.L):                                 # and the state they leave behind is the same state
            for b0, b1, small in parts:
                n = wide.rows
                assert torch.equal(wide.Kc[l][b0:b1, :n], small.Kc[l][:, :n]) and torch.equal(wide.hist[l][b0:b1], small.hist[l])


def test_wide_steps_are_reproducible(dev):
    """Two identical wide runs (B = 64, fp16ff, 8 steps) give bit-identical logits at every step: the split-K slices are added in slice
    order by the last arriver, per group."""
    precision, B = "fp16ff", 64
    model, wrapper = _coarse(dev, precision)
    condx, flat, rows = _prompt(wrapper, dev, B)
    with torch.no_grad():
        _, a = _wide_steps(model, condx, flat, rows, precision, B)
        _, b = _wide_steps(model, condx, flat, rows, precision, B)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k


def _spy_decoders(monkeypatch):
    """Record (model, batch, wide) of every CachedDecoder that generate() builds."""
    from open_musiclm_amd import decode
    built = []
    orig = decode.CachedDecoder

    class Spy(orig):
        def __init__(self, model, batch, max_rows, precision, wide=False):
            built.append((model, batch, wide))
            super().__init__(model, batch, max_rows, precision, wide=wide)
    monkeypatch.setattr(decode, "CachedDecoder", Spy)
    return built


def test_generate_routes_a_large_batch_through_wide_calls(dev, monkeypatch):
    """generate() at B = 40 (fp16, injected uniforms, 3 time steps) builds ONE decoder of 40 samples; the ids have the right shape and
    range and use_graph=True returns the eager ids.  A longer run, in which the sampling loop does capture its cycles, replays them with
    the same ids as well.  B = 80 runs as 64 + 16."""
    from open_musiclm_amd import decode
    precision = "fp16"
    model, wrapper = _coarse(dev, precision)
    built = _spy_decoders(monkeypatch)
    Q = 3
    g = torch.Generator().manual_seed(21)

    def inputs(B, steps):
        cond = [torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev), torch.randint(0, 1024, (B, 40), generator=g).to(dev)]
        return dict(conditioning_token_ids=cond, max_time_steps=steps, uniforms=torch.rand(steps * Q, B, V1, generator=g))
    kw = inputs(40, 3)
    eager = wrapper.generate(**kw)
    assert [(b, w) for _, b, w in built] == [(40, True)]
    assert eager.shape == (40, 3, Q) and int(eager.min()) >= 0 and int(eager.max()) < 1024
    assert torch.equal(wrapper.generate(use_graph=True, **kw), eager)
    # 6 time steps: after one eager cycle per quantizer phase the loop captures (decode.SamplingLoop.run) -- the capture path at B > 16
    loops = []
    orig_loop = decode.SamplingLoop

    class LoopSpy(orig_loop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            loops.append(self)
    monkeypatch.setattr(decode, "SamplingLoop", LoopSpy)
    kw6 = inputs(40, 6)
    eager6 = wrapper.generate(**kw6)
    graph6 = wrapper.generate(use_graph=True, **kw6)
    assert len(loops) == 2 and len(loops[1].graphs) == Q and loops[1].use_graph, "the cycles of a 40-sample call were not captured"
    assert torch.equal(graph6, eager6)
    del built[:]
    out = wrapper.generate(**inputs(80, 2))
    assert [(b, w) for _, b, w in built] == [(64, True), (16, True)]
    assert out.shape == (80, 2, Q) and int(out.min()) >= 0 and int(out.max()) < 1024


def test_fine_windows_together_reproduces_the_golden_tokens(golden_dir, dev, monkeypatch):
    """MusicLM.forward(fine_windows_together=True) on the tiny golden stages (bf16x3, golden kwargs): the four fine windows run as ONE
    fine.generate call over 4 x 2 samples, fed the recorded uniforms of the reference's four fine calls concatenated along the batch
    axis in window order; the final [coarse | fine] ids equal the reference's bit for bit."""
    from open_musiclm_amd import open_musiclm as M
    z = np.load(os.path.join(golden_dir, "musiclm_forward.npz"))
    tiny, kw = ast.literal_eval(str(z["meta.tiny"])), ast.literal_eval(str(z["meta.kwargs"]))
    cb = dict(clap_codebook_size=32, semantic_codebook_size=48, acoustic_codebook_size=40)
    sem = M.create_semantic_transformer(**tiny, clap_codebook_size=32, semantic_codebook_size=48, precision="bf16x3")
    coarse = M.create_coarse_transformer(**tiny, num_coarse_quantizers=3, precision="bf16x3", **cb)
    fine = M.create_fine_transformer(**tiny, num_coarse_quantizers=3, num_fine_quantizers=5, clap_codebook_size=32,
                                     acoustic_codebook_size=40, precision="bf16x3")
    for pfx, m in (("sem", sem), ("coarse", coarse), ("fine", fine)):
        m.load_state_dict({k[len(f"sd.{pfx}."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"sd.{pfx}.")}, strict=True)
        m.to(dev)
    mlm = M.MusicLM(wav2vec=None, clap=None, neural_codec=None, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    n_calls = int(z["n_calls"])
    stages = [str(z[f"call.{i}.stage"]) for i in range(n_calls)]
    fine_calls = [i for i, s in enumerate(stages) if s == "fine"]
    assert len(fine_calls) == 4 and fine_calls == list(range(fine_calls[0], n_calls))
    state = dict(i=0)
    counts = dict(semantic=0, coarse=0, fine=0)

    def source(n, batch, v1):
        i = state["i"]
        if stages[i] == "fine":                  # the single stacked call: sample w * B + b draws what window w's call drew for sample b
            u = torch.cat([torch.from_numpy(z[f"call.{j}.uniforms"]) for j in fine_calls], dim=1)
        else:
            u = torch.from_numpy(z[f"call.{i}.uniforms"])
        assert u.shape == (n, batch, v1), (i, tuple(u.shape), (n, batch, v1))
        return u
    monkeypatch.setattr(M, "UNIFORM_SOURCE", source)
    for name in ("semantic", "coarse", "fine"):
        stage = getattr(mlm, name)

        def wrapped(*a, _orig=stage.generate, _name=name, **k):
            assert stages[state["i"]] == _name
            out = _orig(*a, **k)
            counts[_name] += 1
            state["i"] += 1
            return out
        monkeypatch.setattr(stage, "generate", wrapped)
    s, c, f = mlm.generate(clap_token_ids=torch.from_numpy(z["clap_ids"]).to(dev), return_tokens=True, fine_windows_together=True, **kw)
    assert counts["fine"] == 1 and counts["semantic"] + counts["coarse"] == fine_calls[0]
    fine_ref = np.concatenate([z[f"call.{j}.ids"] for j in fine_calls], axis=1)
    assert np.array_equal(f.cpu().numpy(), fine_ref)
    acoustic = torch.cat([c, f], dim=-1).cpu().numpy()
    assert np.array_equal(acoustic, z["acoustic"])


def test_fine_windows_together_takes_the_wide_route(dev, monkeypatch):
    """Three dim-1024 depth-1 stages in fp16, 4 prompts, 5 fine windows: with the flag the fine stage builds one decoder of 20 samples and
    returns ids of the sequential path's shape, in range.  With overlapping windows (step percent 0.5) the flag changes nothing: the same
    number of fine.generate calls and, from the same seed, the same ids."""
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    kw = dict(dim=1024, depth=1, heads=8, precision="fp16")
    sem = M.create_semantic_transformer(**kw).to(dev)
    coarse = M.create_coarse_transformer(num_coarse_quantizers=3, **kw).to(dev)
    fine = M.create_fine_transformer(num_coarse_quantizers=3, num_fine_quantizers=5, **kw).to(dev)
    mlm = M.MusicLM(wav2vec=None, clap=None, neural_codec=None, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    built = _spy_decoders(monkeypatch)
    calls = []
    orig = mlm.fine.generate
    monkeypatch.setattr(mlm.fine, "generate", lambda *a, **k: (calls.append(k["coarse_token_ids"].shape[0]), orig(*a, **k))[1])
    P = 4
    clap_ids = torch.randint(0, 1024, (P, 12, 1), device=dev)
    args = dict(clap_token_ids=clap_ids, output_seconds=5, semantic_window_seconds=5, coarse_window_seconds=5, fine_window_seconds=1,
                semantic_steps_per_second=2, acoustic_steps_per_second=2, return_tokens=True)

    def run(**extra):
        del built[:], calls[:]
        torch.manual_seed(7)
        out = mlm.generate(**args, **extra)
        return out, [b for m, b, _ in built if m is fine], list(calls)
    (s0, c0, f0), fine_decs0, calls0 = run()
    assert calls0 == [P] * 5 and fine_decs0 == [P] * 5
    (s1, c1, f1), fine_decs1, calls1 = run(fine_windows_together=True)
    assert calls1 == [5 * P] and fine_decs1 == [5 * P], (calls1, fine_decs1)
    assert torch.equal(s1, s0) and torch.equal(c1, c0)          # the stages before it consumed the same random stream
    assert f1.shape == f0.shape == (P, 10, 5) and int(f1.min()) >= 0 and int(f1.max()) < 1024
    (_, _, f2), _, calls2 = run(fine_sliding_window_step_percent=0.5)
    (_, _, f3), _, calls3 = run(fine_sliding_window_step_percent=0.5, fine_windows_together=True)
    assert calls3 == calls2 and len(calls2) > 1 and set(calls2) == {P}
    assert torch.equal(f3, f2)
