"""GPU: the sampler on its counter-based uniform stream (include/omlm.h; csrc/sampler.hip, the RNG = true instantiations).

The central check: a stream entry point returns, id for id, what the buffer entry point returns when it is fed the numpy restatement of
the stream (tests/sampler_stream_ref.py).  Both run the same sampler function of (logits, u) and the stream's values are exact in float32,
so equality is exact -- no near-tie allowance.  Then the law of the sampled ids on the device, generate() on every route, and the memory
the stream saves."""

import numpy as np
import pytest
import torch

import sampler_stream_ref as S
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
SEED = 0x9E3779B97F4A7C15
CHI2_15_BOUND = 15 + 6 * 30 ** 0.5                     # mean + 6 standard deviations of chi^2 with 15 degrees of freedom: 47.9


def _logits(B, V, ld, seed):
    """[B, ld] with NaN padding: random rows, row 1 heavy ties (values from a set of 4), row 2 all -inf."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 4
    x[1] = torch.randint(0, 4, (V,), generator=g).float()
    x[2] = -INF
    logits = torch.full((B, ld), NAN)
    logits[:, :V] = x
    return logits


# every instantiation and each seam: <17> to 1088, <32> to 2048, wide <4> to 4096, <16> to 16384, <64> to 65536
@pytest.mark.parametrize("V", [1, 64, 1025, 1088, 1089, 2048, 2049, 4096, 4097, 16384, 16385, 65536])
def test_stream_entry_equals_buffer_entry_fed_the_restatement(ops, dev, V):
    B, ld = 5, (V + 7) // 8 * 8 + 8
    lg = _logits(B, V, ld, 1000 + V).to(dev)
    launches = 0
    for step in (0, 7):
        for row0 in (0, 3):
            u = torch.from_numpy(S.uniforms(SEED, 1, B, V, row0=row0, t0=step)[0]).to(dev)
            for k in sorted({1, max(int(0.1 * V), 1), V}):
                for forbid in (False, True):
                    want = torch.full((B,), -7, dtype=torch.long, device=dev)
                    got = torch.full((B,), -7, dtype=torch.long, device=dev)
                    ops.sample_topk_gumbel(lg, u, want, V, k, 0.9, forbid)
                    ops.sample_topk_gumbel_rng(lg, SEED, step, row0, got, V, k, 0.9, forbid)
                    assert torch.equal(got, want), (V, step, row0, k, forbid, got.tolist(), want.tolist())
                    assert int(got.min()) >= 0 and int(got.max()) < V and int(got[2]) == 0            # the all -inf row: index 0
                    launches += 1
                    if row0 == 0:
                        # rows [3, 5) of this call are rows [0, 2) of a call that starts at global sample 3
                        tail = torch.full((2,), -7, dtype=torch.long, device=dev)
                        ops.sample_topk_gumbel_rng(lg[3:], SEED, step, 3, tail, V, k, 0.9, forbid)
                        assert torch.equal(tail, got[3:]), (V, step, k, forbid)
    # the seed matters: over 8 steps at k = V another seed moves some id
    if V >= 64:
        ids = {}
        for seed in (SEED, SEED + 1):
            outs = [torch.empty(B, dtype=torch.long, device=dev) for _ in range(8)]
            for t, o in enumerate(outs):
                ops.sample_topk_gumbel_rng(lg, seed, t, 0, o, V, V, 0.9, False)
            ids[seed] = torch.stack(outs)
        assert not torch.equal(ids[SEED], ids[SEED + 1])
    report(f"sampler_stream_equals_buffer[V={V}]", exact=True, launches=launches)


@pytest.mark.parametrize("V", [1025, 2049])
def test_stream_at_and_embed_at_equal_the_buffer_forms(ops, dev, V):
    """The graph-replayable forms: the device step counter is advanced three times through omlm_decode_advance; hist slots, out and the
    gathered x rows equal the buffer forms'."""
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    B, steps, D, ld, row0 = 6, 4, 64, V + 7, 2
    k, T = max(int(0.1 * V), 1), 0.95
    U = torch.from_numpy(S.uniforms(SEED, steps, B, V, row0=row0)).to(dev)
    lo, hi = ops.split_seed(SEED)
    E = V + 3                                                                # offset 7: the upper ids clamp to row E - 1
    emb = torch.randn(E, D, generator=torch.Generator().manual_seed(V)).to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = lambda *shape: torch.full(shape, -7, dtype=torch.long, device=dev)  # noqa: E731
    hist_b, hist_r, hist_eb, hist_er = (mk(steps, B) for _ in range(4))
    for t in range(steps):
        lg = _logits(B, V, ld, 7 * V + t).to(dev)
        out_b, out_r, out_eb, out_er = (mk(B) for _ in range(4))
        x_b = torch.full((B, D), NAN, device=dev)
        x_r = torch.full((B, D), NAN, device=dev)
        call("omlm_sample_topk_gumbel_at", ptr(lg), ptr(U), ptr(step_dev), ptr(out_b), ptr(hist_b), B, V, ld, k, T, 1, stream_ptr())
        call("omlm_sample_topk_gumbel_at_rng", ptr(lg), lo, hi, ptr(step_dev), row0, ptr(out_r), ptr(hist_r), B, V, ld, k, T, 1, stream_ptr())
        call("omlm_sample_embed_at", ptr(lg), ptr(U), ptr(step_dev), ptr(out_eb), ptr(hist_eb), B, V, ld, k, T, 1,
             ptr(emb), 7, E, ptr(x_b), D, stream_ptr())
        call("omlm_sample_embed_at_rng", ptr(lg), lo, hi, ptr(step_dev), row0, ptr(out_er), ptr(hist_er), B, V, ld, k, T, 1,
             ptr(emb), 7, E, ptr(x_r), D, stream_ptr())
        assert torch.equal(out_r, out_b) and torch.equal(out_er, out_b) and torch.equal(out_eb, out_b), (V, t)
        assert torch.equal(x_r, x_b) and torch.equal(x_r, emb[(out_b + 7).clamp(0, E - 1)]), (V, t)
        assert torch.equal(hist_r[t], out_b) and bool((hist_r[t + 1:] == -7).all()), (V, t)        # only slot *step_dev written
        if t < steps - 1:
            call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())
    assert int(step_dev.item()) == 3
    assert torch.equal(hist_r, hist_b) and torch.equal(hist_er, hist_b) and torch.equal(hist_eb, hist_b)
    assert len({tuple(r) for r in hist_b.tolist()}) == steps                   # the steps drew different ids
    report(f"sampler_stream_at_embed_at[V={V}]", exact=True)


def test_sampling_law_on_the_device(ops, dev):
    """The inputs of test_sampler_stream_host.test_sampling_law through omlm_sample_topk_gumbel_at_rng: 4096 steps of 16 rows, the ids
    follow softmax(l / T) over the 16 kept logits; chi^2_15 below mean + 6 sigma = 47.9."""
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    logits = np.float32(np.random.default_rng(0).standard_normal(64) * 2)
    k, T, steps, B = 16, 0.7, 4096, 16
    lg = torch.from_numpy(logits)[None].repeat(B, 1).contiguous().to(dev)
    lo, hi = ops.split_seed(SEED)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(B, dtype=torch.long, device=dev)
    hist = torch.full((steps, B), -7, dtype=torch.long, device=dev)
    for _ in range(steps):
        call("omlm_sample_topk_gumbel_at_rng", ptr(lg), lo, hi, ptr(step_dev), 0, ptr(out), ptr(hist), B, 64, 64, k, T, 0, stream_ptr())
        call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())
    ids = hist.cpu().numpy().ravel()
    assert int(step_dev.item()) == steps and ids.min() >= 0 and ids.max() < 64
    kept = np.zeros(64, dtype=bool)
    kept[np.argsort(-logits.astype(np.float64), kind="stable")[:k]] = True                  # no ties among 64 normal draws
    p = np.where(kept, np.exp((logits.astype(np.float64) - logits.max()) / T), 0.0)
    p /= p.sum()
    expected = p * steps * B
    counts = np.bincount(ids, minlength=64).astype(np.float64)
    assert counts[~kept].sum() == 0
    chi2 = float((((counts - expected) ** 2)[kept] / expected[kept]).sum())
    print(f"sampler stream law on the device: chi2_15 {chi2:.1f}, smallest expected count {expected[kept].min():.0f}")
    report("sampler_stream_law_device", chi2_15=chi2, bound=CHI2_15_BOUND)
    assert chi2 < CHI2_15_BOUND, chi2


def _tiny(dev, codebook, seed=0):
    """The semantic-like model of test_gpu_wide_codebook.py (dim 64, depth 1, one head, conditioning codebook 32 x 2 quantizers)."""
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(seed)
    seqs = [M.TokenSequenceInfo(32, 2, False), M.TokenSequenceInfo(codebook, 1, False)]
    model = M.TokenConditionedTransformer(token_sequences=seqs, dim=64, depth=1, heads=1, ff_dropout=0.0, precision="bf16x3").to(dev)
    return M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)


@pytest.fixture(scope="module")
def tiny2048(dev):
    wrapper = _tiny(dev, 2048)
    cond = [torch.randint(0, 32, (2, 3, 2), generator=torch.Generator().manual_seed(5)).to(dev)]
    return wrapper, cond


ROUTES = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "graph": dict(use_cache=True, use_graph=True)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_generate_on_the_stream_equals_generate_fed_the_restatement(dev, tiny2048, route):
    """V1 = 2049, B = 2, 8 ids: generate(sampler_rng="counter", sampler_seed=s) == generate(uniforms=restatement(s)), id for id, on the
    cached loop, the re-forward route and the captured-graph loop (8 ids: the graph is captured at id 1 and replayed to id 6)."""
    from open_musiclm_amd import decode
    wrapper, cond = tiny2048
    steps, V1 = 8, 2049
    assert decode.supports(wrapper.transformer, 1, prompt_rows=12)
    for s in (3, SEED):
        U = torch.from_numpy(S.uniforms(s, steps, 2, V1))
        want = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, uniforms=U, **ROUTES[route])
        got = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, sampler_rng="counter", sampler_seed=s, **ROUTES[route])
        assert got.shape == (2, steps, 1) and torch.equal(got, want), (route, s, got.tolist(), want.tolist())
        assert int(got.min()) >= 0 and int(got.max()) < 2048
    with pytest.raises(ValueError, match="counter"):
        wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, uniforms=U, sampler_rng="counter", **ROUTES[route])
    with pytest.raises(ValueError, match="sampler_rng"):
        wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, sampler_rng="philox", **ROUTES[route])


def test_ids_do_not_depend_on_how_the_batch_is_cut(ops, dev, tiny2048, monkeypatch):
    """With one sample per decode call (row0 = 0, 1) the stream gives the ids of the two-sample call.  And the loop's one sampler path
    (omlm_sample on a block built once; top_p None, no logprobs) draws the stream of the entry point that predates it: every id of the
    cut call again, through ops.sample_topk_gumbel_rng on the logits the loop sampled it from, same seed, step and row0."""
    from open_musiclm_amd import decode
    wrapper, cond = tiny2048
    whole = wrapper.generate(conditioning_token_ids=cond, max_time_steps=6, sampler_rng="counter", sampler_seed=11)
    monkeypatch.setattr(decode, "max_call_batch", lambda *a, **k: 1)
    seen, cycle = [], decode.SamplingLoop._cycle

    def recording_cycle(self, k, with_decode):
        seen.append((self, k - self.n0, self.dec.logits.clone()))
        cycle(self, k, with_decode)
    monkeypatch.setattr(decode.SamplingLoop, "_cycle", recording_cycle)
    cut = wrapper.generate(conditioning_token_ids=cond, max_time_steps=6, sampler_rng="counter", sampler_seed=11)
    assert torch.equal(cut, whole), (cut.tolist(), whole.tolist())
    assert not torch.equal(whole[0], whole[1])                                  # the samples draw from different rows of the stream
    assert sorted((loop.row0, step) for loop, step, _ in seen) == [(b, t) for b in range(2) for t in range(6)]
    out = torch.empty(1, device=dev, dtype=torch.long)
    for loop, step, logits in seen:
        assert loop.top_p == 1.0 and not loop.logprobs and loop.U is None and loop.dec.Q == 1
        ops.sample_topk_gumbel_rng(logits, 11, step, loop.row0, out, loop.dec.V1, loop.topk, loop.temperature, loop.forbid[0])
        assert torch.equal(out, loop.hist[step]), (loop.row0, step, out.tolist(), loop.hist[step].tolist())


@pytest.mark.parametrize("use_cache", [True, False])
def test_manual_seed_governs_the_stream(dev, tiny2048, use_cache):
    wrapper, cond = tiny2048
    run = lambda: wrapper.generate(conditioning_token_ids=cond, max_time_steps=6, sampler_rng="counter", use_cache=use_cache)  # noqa: E731
    torch.manual_seed(123)
    a = run()
    torch.manual_seed(123)
    b = run()
    torch.manual_seed(124)
    c = run()
    assert torch.equal(a, b) and not torch.equal(a, c), (a.tolist(), b.tolist(), c.tolist())


def test_the_stream_saves_the_uniform_buffer(dev):
    """Predicted codebook 8192 (V1 = 8193), B = 4, 128 ids: the buffer is 128 * 4 * 8193 floats = 16.8 MB; the peak of allocated bytes of
    the counter call lies below the buffer call's by at least 0.9 of that."""
    wrapper = _tiny(dev, 8192)
    cond = [torch.randint(0, 32, (4, 3, 2), generator=torch.Generator().manual_seed(6)).to(dev)]
    n_new, B, V1 = 128, 4, 8193
    buf = 4 * n_new * B * V1
    wrapper.generate(conditioning_token_ids=cond, max_time_steps=2, sampler_rng="buffer")          # anything built on first use is built
    peak = {}
    for rng in ("buffer", "counter"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ids = wrapper.generate(conditioning_token_ids=cond, max_time_steps=n_new, sampler_rng=rng, sampler_seed=1)
        torch.cuda.synchronize()
        peak[rng] = torch.cuda.max_memory_allocated()
        assert ids.shape == (B, n_new, 1) and int(ids.min()) >= 0 and int(ids.max()) < 8192
    print(f"sampler stream memory: buffer {buf} bytes, peak allocated: buffer call {peak['buffer']}, counter call {peak['counter']}")
    report("sampler_stream_memory", buffer_bytes=buf, peak_buffer=peak["buffer"], peak_counter=peak["counter"])
    assert peak["buffer"] - peak["counter"] >= 0.9 * buf, (peak, buf)
