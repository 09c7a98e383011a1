"""Per-row sampling parameters on the device: omlm_sample_rows and omlm_guide_logits_rows against the scalar entry points (product
against product: ids id for id, log-probabilities bit for bit), and generate() with one setting per row on every route."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import guidance_ref as G
import sampler_logprob_ref as L
import sampler_stream_ref as S
from test_gpu_guidance import _cond, _small, _wide
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_sampler_stream import _tiny

pytestmark = pytest.mark.gpu

NAN, INF, POISON = float("nan"), float("inf"), 12345.0
SEED = 0x9E3779B97F4A7C15
TS, PS = (0.4, 1.0, 1.7), (0.05, 0.5, 0.999, 1.0)


def _logits(B, V, ld, seed):
    """[B, ld] with NaN padding: random rows, row 1 heavy ties (values from a set of 4), row 2 all -inf."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 4
    x[1] = torch.randint(0, 4, (V,), generator=g).float()
    x[2] = -INF
    logits = torch.full((B, ld), NAN)
    logits[:, :V] = x
    return logits


def _bits(t):
    return t.contiguous().view(torch.int32)


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _f32(v, dev):
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _host(res):
    """(ids, lp_model, lp_sampled) -> three lists: the ids, and the bit patterns of the two log-probabilities."""
    return res[0].tolist(), _bits(res[1]).tolist(), _bits(res[2]).tolist()


def _run(ops, dev, lg, V, forbid, src, k=None, T=None, p=None, lp=True, **rows):
    """One ops.sample launch -> (ids, lp_model, lp_sampled); the outputs start poisoned."""
    B = lg.shape[0]
    out = torch.full((B,), -7, dtype=torch.long, device=dev)
    lpm, lps = (torch.full((B,), POISON, device=dev) for _ in range(2))
    ops.sample(lg, out, V, k, T, forbid, top_p=p, lp_model=lpm if lp else None, lp_sampled=lps if lp else None, **src, **rows)
    return out, lpm, lps


# ---- 1. the row form against the scalar form ---------------------------------------------------------------------------------------------
# every instantiation and each seam: <17> to 1088, <32> to 2048, wide <4> to 4096, <16> to 16384, <64> to 65536
@pytest.mark.parametrize("V", [64, 1025, 1088, 1089, 2048, 2049, 4097, 16385, 65536])
def test_row_form_equals_the_scalar_form_row_by_row(ops, dev, V):
    """All 36 tuples of {1, V // 10, V} x {0.4, 1.0, 1.7} x {0.05, 0.5, 0.999, 1.0} over three launches of 16 rows (top_p runs fastest:
    every launch holds rows with and without a nucleus).  Row r of a launch equals row r of the scalar launch of its tuple."""
    B, ld = 16, (V + 7) // 8 * 8 + 8
    lg = _logits(B, V, ld, 3000 + V).to(dev)
    tuples = list(itertools.product(sorted({1, max(V // 10, 1), V}), TS, PS))
    assert len(tuples) == 36
    u = torch.rand(B, V, generator=torch.Generator().manual_seed(V)).to(dev)
    launches = 0
    for src in (dict(uniform=u), dict(seed=SEED, step=5, row0=3)):
        for forbid in (False, True):
            scalar = {}
            for g in range(3):
                rows = [tuples[(16 * g + r) % 36] for r in range(B)]
                assert any(p == 1.0 for _, _, p in rows) and any(p < 1.0 for _, _, p in rows)
                arrays = dict(row_k=_i32([k for k, _, _ in rows], dev), row_temperature=_f32([T for _, T, _ in rows], dev),
                              row_top_p=_f32([p for _, _, p in rows], dev))
                res = _run(ops, dev, lg, V, forbid, src, **arrays)
                bare = _run(ops, dev, lg, V, forbid, src, lp=False, **arrays)[0]      # NULL lp pointers: the same ids
                launches += 2
                assert torch.equal(bare, res[0])
                ids, lpm, lps = _host(res)
                assert min(ids) >= 0 and max(ids) < V and ids[2] == 0             # the all -inf row: index 0
                for r, tup in enumerate(rows):
                    if tup not in scalar:
                        scalar[tup] = _host(_run(ops, dev, lg, V, forbid, src, *tup))
                        launches += 1
                    wi, wm, ws = scalar[tup]
                    assert ids[r] == wi[r], (V, forbid, list(src), r, tup, ids[r], wi[r])
                    assert lpm[r] == wm[r] and lps[r] == ws[r], (V, forbid, list(src), r, tup, res[1][r].item(), res[2][r].item())
            assert len(scalar) == 36
    report(f"sampler_rows_equal_scalar[V={V}]", exact=True, launches=launches)


# ---- 2. degenerate forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 4097])
def test_degenerate_row_forms_equal_the_scalar_call(ops, dev, V, monkeypatch):
    from open_musiclm_amd import hip
    B, ld, k, T, p = 7, V + 7, max(V // 10, 1), 0.8, 0.9
    lg = _logits(B, V, ld, 17 * V).to(dev)
    src = dict(seed=SEED, step=2, row0=1)
    want = _run(ops, dev, lg, V, True, src, k, T, p)
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))  # noqa: E731
    full = dict(row_k=_i32([k] * B, dev), row_temperature=_f32([T] * B, dev), row_top_p=_f32([p] * B, dev),
                row_seed=ops.row_tensor([SEED] * B, "seed", dev), row_sample=_i32([1 + r for r in range(B)], dev))
    # one value in every row of every array; the scalars they replace are not read
    assert same(_run(ops, dev, lg, V, True, dict(step=2), None, None, None, **full), want)
    # each array alone, the others NULL
    for name, t in full.items():
        assert same(_run(ops, dev, lg, V, True, src if name != "row_seed" else dict(step=2, row0=1), k, T, p, **{name: t}), want), name
    # top_p == 1 in every row: the call without a nucleus
    assert same(_run(ops, dev, lg, V, True, src, k, T, None, row_top_p=_f32([1.0] * B, dev)), _run(ops, dev, lg, V, True, src, k, T, None))
    # k is clamped into [1, V] on the device
    assert same(_run(ops, dev, lg, V, True, src, None, T, p, row_k=_i32([0, -5] + [k] * (B - 2), dev)),
                _run(ops, dev, lg, V, True, src, None, T, p, row_k=_i32([1, 1] + [k] * (B - 2), dev)))
    assert torch.equal(_run(ops, dev, lg, V, True, src, None, T, p, row_k=_i32([V + 9] * B, dev))[0], _run(ops, dev, lg, V, True, src, V, T, p)[0])
    # no array: omlm_sample_rows is omlm_sample_lp -- rows NULL, and a block of five NULLs
    lo, hi = ops.split_seed(SEED)
    for rows in (None, ops.SampleRowParams()):
        out = torch.full((B,), -7, dtype=torch.long, device=dev)
        lpm, lps = (torch.full((B,), POISON, device=dev) for _ in range(2))
        a = ops.SampleArgs(hip.ptr(lg), B, V, ld, None, lo, hi, 2, 1, None, hip.ptr(out), None, k, T, p, 1)
        hip.call("omlm_sample_rows", C.addressof(a), None if rows is None else C.addressof(rows), hip.ptr(lpm), hip.ptr(lps), hip.stream_ptr())
        assert same((out, lpm, lps), want)
        a.k = 0                                                         # and keeps omlm_sample_lp's checks
        with pytest.raises(RuntimeError, match="1 <= k <= V"):
            hip.call("omlm_sample_rows", C.addressof(a), None if rows is None else C.addressof(rows), hip.ptr(lpm), hip.ptr(lps), hip.stream_ptr())
    # ops.sample without row tensors names neither new entry point
    names, real = [], hip.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    _run(ops, dev, lg, V, True, src, k, T, p)
    _run(ops, dev, lg, V, True, src, k, T, p, lp=False)
    _run(ops, dev, lg, V, True, src, k, T, p, row_k=full["row_k"])
    assert names == ["omlm_sample_lp", "omlm_sample", "omlm_sample_rows"]


# ---- 3. the per-row stream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2049])
def test_per_row_stream(ops, dev, V):
    from open_musiclm_amd import hip
    B, ld, k, T, p = 6, V + 7, max(V // 10, 1), 0.9, 0.95
    lg = _logits(B, V, ld, 5 * V).to(dev)
    lg[2, :V] = torch.randn(V, generator=torch.Generator().manual_seed(2)).to(dev)        # every row live: ids that can move
    seeds = [SEED, 1, 2 ** 64 - 1, 2 ** 63, 12345, SEED ^ 1]
    samples = [0, 7, 3, 63, 1000, 5]
    rows = dict(row_seed=ops.row_tensor(seeds, "seed", dev), row_sample=_i32(samples, dev))
    got = _run(ops, dev, lg, V, False, dict(step=4), k, T, p, **rows)
    for r in range(B):
        one = _run(ops, dev, lg[r:r + 1], V, False, dict(seed=seeds[r], step=4, row0=samples[r]), k, T, p)
        assert int(got[0][r]) == int(one[0][0]) and int(_bits(got[1])[r]) == int(_bits(one[1])[0]) and \
            int(_bits(got[2])[r]) == int(_bits(one[2])[0]), (V, r)
    # the restatement of the stream: the buffer form fed u(4, sample_r, c) of seed_r
    u = torch.from_numpy(np.concatenate([S.uniforms(s, 1, 1, V, row0=b, t0=4)[0] for s, b in zip(seeds, samples)])).to(dev)
    assert torch.equal(_run(ops, dev, lg, V, False, dict(uniform=u), k, T, p)[0], got[0])
    # permuting the rows together with their parameters permutes the ids
    perm = [3, 0, 5, 1, 4, 2]
    pk, pT = [1, k, V, k, 2, 5], [0.4, 1.0, 1.7, 0.9, 0.7, 1.3]
    mk = lambda order: dict(row_k=_i32([pk[i] for i in order], dev), row_temperature=_f32([pT[i] for i in order], dev),  # noqa: E731
                            row_seed=ops.row_tensor([seeds[i] for i in order], "seed", dev), row_sample=_i32([samples[i] for i in order], dev))
    a = _run(ops, dev, lg, V, True, dict(step=1), None, None, p, **mk(range(B)))
    b = _run(ops, dev, lg[perm].contiguous(), V, True, dict(step=1), None, None, p, **mk(perm))
    assert all([x[i] for i in perm] == y for x, y in zip(_host(a), _host(b)))
    assert len(set(a[0].tolist())) > 1
    # seed / sample belong to the counter stream: refused by name with a uniform buffer, by the library and by ops.sample
    out = torch.zeros(B, dtype=torch.long, device=dev)
    for member, t in (("seed", rows["row_seed"]), ("sample", rows["row_sample"])):
        a_ = ops.SampleArgs(hip.ptr(lg), B, V, ld, hip.ptr(u), 0, 0, 0, 0, None, hip.ptr(out), None, k, T, p, 0)
        rp = ops.SampleRowParams(**{member: hip.ptr(t)})
        with pytest.raises(RuntimeError, match=f"rows->{member}.*uniform"):
            hip.call("omlm_sample_rows", C.addressof(a_), C.addressof(rp), None, None, hip.stream_ptr())
        with pytest.raises(ValueError, match=f"row_{member}"):
            ops.sample(lg, out, V, k, T, False, uniform=u, **{f"row_{member}": t})


# ---- 4. the replayable form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,stream", [(1025, False), (1025, True), (2049, True), (2049, False)])
def test_replayable_row_form(ops, dev, V, stream):
    """step_dev, hist / lp_* [steps, B] and the embedding gather with per-row arrays, three steps driven by omlm_decode_advance: every step
    equals the scalar form's of the row's tuple (run on the same counter into buffers of its own); x rows are the table rows of the ids."""
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    B, steps, D, ld = 6, 3, 64, V + 7
    tuples = [(1, 0.4, 1.0), (max(V // 10, 1), 1.0, 0.5), (V, 1.7, 0.999)]
    rows = [tuples[r % 3] for r in range(B)]
    arrays = dict(row_k=_i32([t[0] for t in rows], dev), row_temperature=_f32([t[1] for t in rows], dev), row_top_p=_f32([t[2] for t in rows], dev))
    U = torch.rand(steps, B, V, generator=torch.Generator().manual_seed(V)).to(dev)
    src = dict(seed=SEED, row0=2) if stream else dict(uniform=U)
    E = V + 3
    emb = torch.randn(E, D, generator=torch.Generator().manual_seed(V)).to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def state():
        return dict(out=torch.full((B,), -7, dtype=torch.long, device=dev), hist=torch.full((steps, B), -7, dtype=torch.long, device=dev),
                    lp_model=torch.full((steps, B), POISON, device=dev), lp_sampled=torch.full((steps, B), POISON, device=dev),
                    x=torch.full((B, D), NAN, device=dev))
    got, want = state(), {t: state() for t in tuples}
    for t in range(steps):
        lg = _logits(B, V, ld, 9 * V + t).to(dev)
        common = dict(step_dev=step_dev, emb_table=emb, emb_row_offset=7, **src)
        ops.sample(lg, got["out"], V, None, None, True, hist=got["hist"], x=got["x"], lp_model=got["lp_model"], lp_sampled=got["lp_sampled"],
                   **common, **arrays)
        for (k, T, p), w in want.items():
            ops.sample(lg, w["out"], V, k, T, True, top_p=p, hist=w["hist"], x=w["x"], lp_model=w["lp_model"], lp_sampled=w["lp_sampled"], **common)
        for r, tup in enumerate(rows):
            assert int(got["out"][r]) == int(want[tup]["out"][r]) and torch.equal(got["x"][r], want[tup]["x"][r]), (V, t, r)
        assert torch.equal(got["x"], emb[(got["out"] + 7).clamp(0, E - 1)]) and torch.equal(got["hist"][t], got["out"])
        assert bool((got["hist"][t + 1:] == -7).all()) and bool((got["lp_model"][t + 1:] == POISON).all())       # only slot *step_dev written
        if t < steps - 1:
            call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())
    assert int(step_dev.item()) == steps - 1
    for r, tup in enumerate(rows):
        for name in ("hist", "lp_model", "lp_sampled"):
            a, b = got[name][:, r], want[tup][name][:, r]
            assert torch.equal(a if name == "hist" else _bits(a), b if name == "hist" else _bits(b)), (V, r, name)
    assert len({tuple(h) for h in got["hist"].tolist()}) == steps


# ---- 5. the guide kernel with a scale per row -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [41, 1025, 1027])
def test_guide_rows_is_bit_equal_to_the_restatement(ops, dev, V):
    scales = [0.0, 0.5, 1.0, 3.0, 7.5]
    rows = len(scales)
    gen = torch.Generator().manual_seed(V)
    sd = _f32(scales, dev)
    for ld in ((V + 3) // 4 * 4 + 4, (V + 3) // 4 * 4 + 5):                # a multiple of 4 (16-byte loads) and not
        l = torch.full((rows, ld), POISON)
        n = torch.full((rows, ld), POISON)
        l[:, :V] = torch.randn(rows, V, generator=gen) * 9
        n[:, :V] = torch.randn(rows, V, generator=gen) * 9
        n[0, 0] = l[0, 0]
        want = np.stack([G.guide(l[r, :V], n[r, :V], s) for r, s in enumerate(scales)])
        ld_, nd_ = l.to(dev), n.to(dev)
        out = torch.full((rows, ld), POISON, device=dev)
        ops.guide_logits(ld_, nd_, out, V, sd)
        assert np.array_equal(out[:, :V].cpu().numpy().view(np.uint32), want.view(np.uint32)), (V, ld)
        assert bool((out[:, V:] == POISON).all()), (V, ld)                  # the columns past V are not written
        alias = ld_.clone()
        ops.guide_logits(alias, nd_, alias, V, sd)                          # out may be cond
        assert torch.equal(alias, out.where(torch.arange(ld, device=dev)[None] < V, ld_)), (V, ld)
        one = torch.full((rows, ld), POISON, device=dev)                   # and row by row the scalar entry point
        for r, s in enumerate(scales):
            ops.guide_logits(ld_[r:r + 1], nd_[r:r + 1], one[r:r + 1], V, s)
        assert torch.equal(_bits(one), _bits(out))
    with pytest.raises(ValueError, match="scale"):
        ops.guide_logits(ld_, nd_, out, V, sd[:3].contiguous())


# ---- 6. the loop, replayed ----------------------------------------------------------------------------------------------------------------
def _recording(monkeypatch):
    from open_musiclm_amd import decode
    seen, cycle = [], decode.SamplingLoop._cycle

    def recording_cycle(self, k, with_decode):
        seen.append((self, k - self.n0, self.dec.logits.clone()))
        cycle(self, k, with_decode)
    monkeypatch.setattr(decode.SamplingLoop, "_cycle", recording_cycle)
    return seen


@pytest.mark.parametrize("which", ["small", "wide"])
def test_per_row_loop_equals_a_scalar_replay(ops, dev, which, monkeypatch):
    """generate() with per-row temperature, filter_thres and top_p (then cond_scale too): every id of row r equals scalar ops.sample on the
    logits the loop sampled it from, with row r's settings and the same uniforms.  small: first-generation step kernels, P = 3; wide: the
    matrix-core route, P = 18 (the rows cross a group of 16)."""
    from open_musiclm_amd import decode
    precision = "fp16ff"
    model, wrapper = _small(dev, precision) if which == "small" else _wide(dev, precision)
    P = 3 if which == "small" else 18
    assert decode.step_route(P, *decode._geometry(model), True, wide=True) == ("gen1" if which == "small" else "dec4")
    seq = model.token_sequences[-1]
    V1, Q, steps = seq.codebook_size + 1, seq.num_quantizers, 2
    n_new = steps * Q
    settings = [(0.4, 0.0, 0.5), (1.0, 0.9, 1.0), (1.7, 0.5, 0.999)]        # (temperature, filter_thres, top_p)
    per_row = [settings[r % 3] for r in range(P)]
    kw = dict(temperature=[s[0] for s in per_row], filter_thres=[s[1] for s in per_row], top_p=[s[2] for s in per_row])
    scales = [(0.0, 1.5, 3.0)[(r // 3) % 3] for r in range(P)]
    cond = _cond(model, P, dev, seed=21)
    U = torch.rand(n_new, P, V1, generator=torch.Generator().manual_seed(6)).to(dev)
    seen = _recording(monkeypatch)
    for guided in (False, True):
        del seen[:]
        gkw = dict(cond_scale=scales) if guided else {}
        ids, lps = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, uniforms=U, return_logprobs=True, **kw, **gkw)
        assert ids.shape == (P, steps, Q) and [s for _, s, _ in seen] == list(range(n_new))
        flat, worst = ids.reshape(P, -1), 0.0
        for loop, j, logits in seen:
            assert loop.P == P and logits.shape[0] == (2 * P if guided else P)
            src = logits[:, :V1]
            if guided:
                g = np.stack([G.guide(logits[r, :V1], logits[P + r, :V1], scales[r]) for r in range(P)])
                src = torch.from_numpy(g).to(dev)
            for T, thres, p in settings:
                out = torch.empty(P, dtype=torch.long, device=dev)
                ops.sample(src.contiguous(), out, V1, max(int((1 - thres) * V1), 1), T, loop.forbid[j % Q], top_p=p, uniform=U[j])
                for r in range(P):
                    if per_row[r] == (T, thres, p):
                        assert int(flat[r, j]) == int(out[r]), (which, guided, j, r, int(flat[r, j]), int(out[r]))
            if guided:
                x = torch.from_numpy(g)
                want = G.log_softmax64(x)
                for r in range(P):
                    s = int(flat[r, j])
                    bound = L.tol(float(x[r, s]), float(x[r, :V1 - 1].max()), 1.0)
                    worst = max(worst, abs(float(lps.model.reshape(P, -1)[r, j]) - float(want[r, s])) / bound)
        if guided:
            print(f"per-row guided replay [{which}]: lp_model error / tol {worst:.3f}")
            report(f"sampler_rows_guided_replay[{which}]", lp_model_err_over_tol=worst)
            assert worst <= 1.0, worst
        assert len({tuple(r) for r in flat.tolist()}) > 1


# ---- 7. routes ----------------------------------------------------------------------------------------------------------------------------
ROUTES = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "graph": dict(use_cache=True, use_graph=True)}


@pytest.fixture(scope="module")
def tiny2048(dev):
    wrapper = _tiny(dev, 2048)
    cond = [torch.randint(0, 32, (4, 3, 2), generator=torch.Generator().manual_seed(5)).to(dev)]
    return wrapper, cond


def test_routes_agree_with_per_row_settings(dev, tiny2048):
    """V1 = 2049, bf16x3, 8 ids (the graph is captured at id 1 and replayed to id 6): the three routes give the same ids, from injected
    uniforms, from the counter stream with one seed and with a seed per row."""
    wrapper, cond4 = tiny2048
    cond = [cond4[0][:2]]
    steps = 8
    kw = dict(conditioning_token_ids=cond, max_time_steps=steps, temperature=[0.7, 1.3], filter_thres=[0.9, 0.5], top_p=[0.8, 1.0],
              return_logprobs=True)
    U = torch.rand(steps, 2, 2049, generator=torch.Generator().manual_seed(3))
    for name, src in (("uniforms", dict(uniforms=U)), ("counter", dict(sampler_rng="counter", sampler_seed=SEED)),
                      ("row seeds", dict(sampler_seed=[SEED, 77]))):
        res = {route: wrapper.generate(**kw, **src, **rk) for route, rk in ROUTES.items()}
        ids, lps = res["cached"]
        assert ids.shape == (2, steps, 1) and int(ids.min()) >= 0 and int(ids.max()) < 2048
        for route in ("uncached", "graph"):
            assert torch.equal(res[route][0], ids), (name, route, res[route][0].tolist(), ids.tolist())
        assert torch.equal(res["graph"][1].model, lps.model) and torch.equal(res["graph"][1].sampled, lps.sampled), name
        scalar = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=0.7, filter_thres=0.9, top_p=0.8,
                                  **(src if name != "row seeds" else dict(sampler_rng="counter", sampler_seed=SEED)))
        assert torch.equal(scalar[0], ids[0]), name                         # row 0 has the scalar call's settings


# ---- 8. neighbours ------------------------------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_neighbours(dev, tiny2048):
    wrapper, cond = tiny2048
    r, steps = 1, 8
    base = dict(temperature=[0.7, 1.3, 1.0, 0.5], top_p=[0.8, 0.9, 1.0, 0.6], sampler_seed=[11, 22, 33, 44])
    run = lambda **kw: wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, return_logprobs=True, **{**base, **kw})  # noqa: E731
    ids, lps = run()
    ids2, lps2 = run(temperature=[1.6, 1.3, 0.4, 1.1], top_p=[0.3, 0.9, 0.5, 1.0], sampler_seed=[5, 22, 2 ** 64 - 1, 7])      # rows != r
    assert torch.equal(ids2[r], ids[r]) and torch.equal(_bits(lps2.model[r]), _bits(lps.model[r])) and \
        torch.equal(_bits(lps2.sampled[r]), _bits(lps.sampled[r]))
    assert all(not torch.equal(ids2[i], ids[i]) for i in range(4) if i != r)
    # the row's uniforms are those of a one-sample call with its seed: alone in a call it gives the same ids (same kernels at dim 64)
    alone = wrapper.generate(conditioning_token_ids=[cond[0][r:r + 1]], max_time_steps=steps, temperature=1.3, top_p=0.9,
                             sampler_rng="counter", sampler_seed=22)
    assert torch.equal(alone[0], ids[r])
    ids3, lps3 = run(sampler_seed=[11, 23, 33, 44])                          # its own seed moves it, and nothing else
    assert not torch.equal(ids3[r], ids[r]) and not torch.equal(lps3.sampled[r], lps.sampled[r])
    assert all(torch.equal(ids3[i], ids[i]) for i in range(4) if i != r)


# ---- 9. cuts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
def test_per_row_ids_do_not_depend_on_how_the_batch_is_cut(dev, guided, monkeypatch):
    """The wide model (matrix-core steps at every call size used here): B = 6 as calls of 2, guided P = 3 as calls of one pair."""
    from open_musiclm_amd import decode
    precision = "fp16ff"
    model, wrapper = _wide(dev, precision)
    B = 3 if guided else 6
    cond = _cond(model, B, dev, n_clap=1, n_sem=9, seed=31)
    row = dict(temperature=[0.5 + 0.2 * r for r in range(B)], filter_thres=[(0.9, 0.0, 0.99)[r % 3] for r in range(B)],
               top_p=[(1.0, 0.7, 0.95)[r % 3] for r in range(B)])
    if guided:
        row["cond_scale"] = [0.0, 1.0, 2.5]
    sizes, init = [], decode.CachedDecoder.__init__

    def recording_init(self, model_, batch, *a, **k):
        sizes.append(batch)
        init(self, model_, batch, *a, **k)
    monkeypatch.setattr(decode.CachedDecoder, "__init__", recording_init)
    real = decode.max_call_batch
    for seeds in (SEED, [100 + r for r in range(B)]):
        kw = dict(conditioning_token_ids=cond, max_time_steps=2, sampler_rng="counter", sampler_seed=seeds, return_logprobs=True, **row)
        del sizes[:]
        whole, lw = wrapper.generate(**kw)
        assert sizes == [2 * B if guided else B]
        monkeypatch.setattr(decode, "max_call_batch", lambda *a, **k: 2)
        cut, lc = wrapper.generate(**kw)
        monkeypatch.setattr(decode, "max_call_batch", real)
        assert sizes[1:] == [2] * 3
        assert whole.shape == (B, 2, 3) and torch.equal(cut, whole), (cut.tolist(), whole.tolist())
        assert torch.equal(_bits(lc.model), _bits(lw.model)) and torch.equal(_bits(lc.sampled), _bits(lw.sampled))
        assert len({tuple(r) for r in whole.reshape(B, -1).tolist()}) > 1


# ---- 10. off means off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["cached", "graph", "uncached"])
def test_scalars_launch_what_they_always_launched(dev, route, monkeypatch):
    from open_musiclm_amd import decode, hip
    from open_musiclm_amd import ops as ops_
    model, wrapper = _small(dev)
    cond = _cond(model, 2, dev)
    kw = dict(conditioning_token_ids=cond, max_time_steps=6, sampler_rng="counter", sampler_seed=3, **ROUTES[route])
    wrapper.generate(**kw)                                          # anything built on first use is built
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    for mod in (hip, decode, ops_):
        monkeypatch.setattr(mod, "call", spy)
    new = {"omlm_sample_rows", "omlm_guide_logits_rows"}
    cycle_names = new | {"omlm_sample", "omlm_sample_lp", "omlm_guide_logits", "omlm_decode_twin", "omlm_decode_step", "omlm_decode_advance"}
    # ids whose cycle the spy sees, 18 ids: all of them; on the graph route the 3 eager ones, the 3 captured ones (a capture records its calls
    # once, replays make none) and the last, which is never decoded
    seen_ids = 7 if route == "graph" else 18

    def cycles(sampler, guided):
        """The parent's calls of the sampling cycle, in order: per id the sampler (behind the combine when guided); on the cached routes
        the twin copy when guided and the decode step, except after the last id."""
        one = (["omlm_guide_logits"] if guided else []) + [sampler]
        if route == "uncached":
            return one * seen_ids
        return (one + (["omlm_decode_twin"] if guided else []) + ["omlm_decode_step"]) * (seen_ids - 1) + one

    def recorded(**more):
        del names[:]
        out = wrapper.generate(**kw, **more)
        return out, list(names)
    for lp, sampler in ((False, "omlm_sample"), (True, "omlm_sample_lp")):
        lpk = dict(return_logprobs=True) if lp else {}
        same = lambda x, y: (torch.equal(x[0], y[0]) and torch.equal(_bits(x[1].model), _bits(y[1].model)) and  # noqa: E731
                             torch.equal(_bits(x[1].sampled), _bits(y[1].sampled))) if lp else torch.equal(x, y)
        want, base = recorded(**lpk)
        # the default call is pinned to the parent's cycle, and explicit numbers launch the default call: the WHOLE sequence, every route
        assert [n for n in base if n in cycle_names] == cycles(sampler, False), (route, lp)
        for numbers in (dict(temperature=1.0, filter_thres=0.9), dict(temperature=1.0, filter_thres=0.9, top_p=None, cond_scale=None),
                        dict(temperature=1, filter_thres=0.9, top_p=1, cond_scale=1), dict(top_p=1.0, cond_scale=1.0)):
            got, seq = recorded(**numbers, **lpk)
            assert seq == base and not new & set(seq), (route, lp, numbers)
            assert same(got, want), (route, lp, numbers)
        # numbers that turn the nucleus and guidance on: the scalar entry points, in the parent's guided cycle
        got, seq = recorded(temperature=0.8, filter_thres=0.5, top_p=0.7, cond_scale=3, **lpk)
        assert not new & set(seq) and [n for n in seq if n in cycle_names] == cycles(sampler, True), (route, lp)
        # the same values as one per row: the row entry points in the same places, every other call the same, and the same result
        rows, rseq = recorded(temperature=[0.8, 0.8], filter_thres=[0.5, 0.5], top_p=[0.7, 0.7], cond_scale=[3, 3], **lpk)
        swap = {sampler: "omlm_sample_rows", "omlm_guide_logits": "omlm_guide_logits_rows"}
        assert rseq == [swap.get(n, n) for n in seq], (route, lp)
        assert same(rows, got), (route, lp)


# ---- 11. pass-through ---------------------------------------------------------------------------------------------------------------------
def test_stages_and_trainer_hand_the_sequences_on(dev, tmp_path):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.data import SyntheticTokenDataset
    from open_musiclm_amd.trainer import SingleStageTrainer
    model, wrapper = _small(dev)
    cond = _cond(model, 3, dev)
    kw = dict(max_time_steps=3, temperature=[0.5, 1.0, 1.5], filter_thres=[0.9, 0.5, 0.0], top_p=[1.0, 0.6, 0.9], cond_scale=[0.0, 1.0, 3.0],
              sampler_seed=[7, 8, 9])
    want = wrapper.generate(conditioning_token_ids=cond, **kw)
    plain = wrapper.generate(conditioning_token_ids=cond, max_time_steps=3, sampler_rng="counter", sampler_seed=7)
    stage = M.CoarseStage(coarse_transformer=model)
    got = stage.generate(clap_token_ids=cond[0], semantic_token_ids=cond[1], **kw)
    assert got.shape == (3, 3, 3) and torch.equal(got, want) and not torch.equal(want, plain)
    torch.manual_seed(0)
    m2 = M.create_coarse_transformer(dim=128, depth=2, heads=2, num_coarse_quantizers=3, ff_dropout=0.1, precision="bf16").to(dev)
    ds = SyntheticTokenDataset("coarse", length=8, coarse_window_seconds=1, semantic_window_seconds=2)
    tr = SingleStageTrainer(m2, "coarse", num_train_steps=1, batch_size=2, dataset=ds, lr=3e-3, lr_warmup=0, grad_accum_every=1, wd=0.01,
                            max_grad_norm=0.5, valid_frac=0.0, save_results_every=1000, save_model_every=1000, results_folder=str(tmp_path),
                            save_predicted_tokens=False, save_reconstructed_wave=False)
    g = torch.Generator().manual_seed(3)
    clap, sem = torch.randint(0, 1024, (3, 12), generator=g).to(dev), torch.randint(0, 1024, (3, 9), generator=g).to(dev)
    out = tr.generate(clap_token_ids=clap, semantic_token_ids=sem, **kw)
    ref = tr.train_wrapper.transformer_wrapper.generate(conditioning_token_ids=[clap, sem], **kw)
    assert out.shape == (3, 3, 3) and torch.equal(out, ref)
