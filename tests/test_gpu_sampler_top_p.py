"""GPU: the sampler's nucleus (top-p) -- the NUC = true instantiations of sample_kernel / sample_wide_kernel behind omlm_sample
(include/omlm.h; csrc/sampler.hip), ops.sample, decode.SamplingLoop and generate(top_p=...).

Against the fp64 restatement (tests/sampler_top_p_ref.py), whose docstring derives the one allowance: a row whose id depends on where
inside p (1 +- 2^-16) the cut falls is left out, at most one such row per case; and the existing near-tie allowance on the Gumbel scores.
Everything that compares the kernels with each other (seams, stream against buffer, top_p = 1 against the six entry points, two
launches) is exact."""

import numpy as np
import pytest
import torch

import loss_optim_sampler_ref as R
import sampler_stream_ref as S
import sampler_top_p_ref as P
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_sampler_stream import ROUTES, _tiny

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
SEED = 0x9E3779B97F4A7C15
U_TOP = 1.0 - 2.0 ** -24                                # the largest uniform: Gumbel term ~ +16.6
PS = [0.05, 0.5, 0.9, 0.999]


def _pad(x, dev, extra=9):
    """[B, V] -> [B, ld] on the device, ld > V, NaN in the padding."""
    B, V = x.shape
    out = torch.full((B, (V + 7) // 8 * 8 + extra), NAN)
    out[:, :V] = x
    return out.to(dev)


def _ids(dev, B):
    return torch.full((B,), -7, dtype=torch.long, device=dev)


def _sample(ops, dev, lg, V, k, T, forbid, **kw):
    out = _ids(dev, lg.shape[0])
    ops.sample(lg, out, V, k, T, forbid, **kw)
    return out


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", P.COMPARE_V)
def test_nucleus_ids_against_fp64(ops, dev, V):
    x, u = P.compare_rows(V)
    B = x.shape[0]
    lg, ud = _pad(x, dev), u.to(dev)
    rdev = dev if V >= 1024 else torch.device("cpu")     # the restatement runs in fp64 where the rows are (the GPU for the long ones)
    xr, ur = x.to(rdev), u.to(rdev)
    cases = rows = near_total = amb_total = worst = 0
    for k in P.compare_ks(V):
        for forbid in (False, True):
            rk = P.Ranked(xr, k, forbid)
            for T in P.COMPARE_T:
                for p in P.COMPARE_P:
                    got = _sample(ops, dev, lg, V, k, T, forbid, top_p=p, uniform=ud).to(rdev)
                    assert int(got.min()) >= 0 and int(got.max()) < V, (V, k, forbid, T, p)
                    want = rk.sample(ur, T, p)
                    amb = rk.ambiguous_rows(ur, T, p)
                    near, i0, i1 = R.near_tie_rows(rk.scores(ur, T, p))
                    near, i0, i1 = near.to(rdev), i0.to(rdev), i1.to(rdev)
                    bad = (got != want) & ~amb & ~(near & ((got == i0) | (got == i1)))
                    assert not bool(bad.any()), (V, k, forbid, T, p, bad.nonzero().flatten().tolist()[:5], got[bad][:5].tolist(),
                                                 want[bad][:5].tolist())
                    if B > 2:
                        assert int(got[2]) == 0                              # the all -inf row
                    n_amb = int(amb.sum())
                    assert n_amb <= P.AMBIGUOUS_CAP, (V, k, forbid, T, p, n_amb)
                    worst, amb_total, near_total = max(worst, n_amb), amb_total + n_amb, near_total + int(near.sum())
                    cases, rows = cases + 1, rows + B
    print(f"top-p against fp64 at V={V}: {cases} cases, {rows} rows, ambiguous {amb_total} (worst case {worst}), near ties {near_total}")
    report(f"sampler_top_p_fp64[V={V}]", cases=cases, rows=rows, ambiguous=amb_total, near_tie_rows=near_total)
    assert near_total <= max(0.01 * rows, 1), (near_total, rows)


# ---- 2. kept-set probes with injected uniforms ---------------------------------------------------------------------------------------
def _probe(ops, dev, V, idx, vals, p, k, T=1.0, floor=-30.0):
    """One row: `vals` at the indices `idx` over a floor 30 below.  Every entry the rule drops gets the largest uniform, the kept ones
    small distinct ones: a dropped entry that the kernel keeps would win (a tied one by +16.6 against at most +0.4; a floor one is kept out
    by the 30).  Returns (id, the rule's kept indices)."""
    x = torch.full((1, V), floor)
    x[0, idx] = torch.tensor(vals)
    mask = P.nucleus_mask(x, k, T, p, False)
    kept = mask[0].nonzero().flatten().tolist()
    u = torch.full((1, V), U_TOP)
    u[0, kept] = torch.linspace(0.1, 0.5, len(kept))[torch.randperm(len(kept), generator=torch.Generator().manual_seed(V + len(kept)))]
    want = int(P.sample(x, u, k, T, p, False))
    assert want in kept
    got = int(_sample(ops, dev, _pad(x, dev), V, k, T, False, top_p=p, uniform=u.to(dev)))
    assert got == want and got in kept, (V, p, k, got, want, kept)
    return got, kept


# (V, first index of a block of ten): wave kernels across the lane-64 boundary; workgroup kernels across the boundary between the segments
# of two waves (64 NV - 1 | 64 NV: NV = 4, 16, 64) and across a lane-64 boundary inside a segment
PROBES = [(1025, 59), (1088, 123), (2048, 59), (2048, 1980), (2049, 251), (4096, 59), (4097, 1019), (16384, 2043), (16385, 4091),
          (65536, 4091), (65536, 65526)]


@pytest.mark.parametrize("V,first", PROBES)
def test_kept_set_probes_tied_block(ops, dev, V, first):
    """Ten equal top logits: p = 0.45 keeps the five lowest indices, 0.05 one, 0.51 six, 0.95 all ten (p m is far from an integer);
    with k = 4 the top-k cuts the block first and p = 0.45 of the four keeps two."""
    idx = list(range(first, first + 10))
    for p, n in ((0.45, 5), (0.05, 1), (0.51, 6), (0.95, 10)):
        for k in (10, 13, V):
            got, kept = _probe(ops, dev, V, idx, [0.0] * 10, p, k)
            assert kept == idx[:n], (V, p, k, kept)
    got, kept = _probe(ops, dev, V, idx, [0.0] * 10, 0.45, 4)
    assert kept == idx[:2]
    # the block scattered over the row (first, middle, last index among them)
    spread = sorted({0, 1, V // 3, V // 2, V // 2 + 1, V - 66, V - 65, V - 64, V - 2, V - 1})
    got, kept = _probe(ops, dev, V, spread, [0.0] * 10, 0.45, V)
    assert kept == spread[:5]


@pytest.mark.parametrize("V,first", PROBES)
def test_kept_set_probes_distinct_values(ops, dev, V, first):
    """Ten distinct values 0, -0.1, ... in an index order of their own; the cut falls halfway between the mass before the sixth and the
    mass before the seventh-ranked entry, so six are kept; and a tied pair straddling the cut."""
    idx = list(range(first, first + 10))
    order = [3, 9, 0, 6, 1, 8, 5, 2, 7, 4]                                  # rank of the value at idx[i]
    vals = [-0.1 * r for r in order]
    w = np.exp(-0.1 * np.arange(10))
    before = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    W = w.sum() + (V - 10) * np.exp(-30.0)
    for n in (1, 6, 9):
        p = float((before[n - 1] + before[n]) / 2 / W)
        for k in (10, V):
            got, kept = _probe(ops, dev, V, idx, vals, p, k)
            assert sorted(kept) == sorted(idx[i] for i in range(10) if order[i] < n), (V, n, k, kept)
    # ranks 4 and 5 share one value: the cut between them keeps the lower index of the two only
    vals2 = [-0.1 * min(r, 4) if r in (4, 5) else -0.1 * r for r in order]
    x = np.array(sorted(vals2, reverse=True))
    w2 = np.exp(x)
    p = float((w2[:4].sum() + 0.5 * w2[4]) / (w2.sum() + (V - 10) * np.exp(-30.0)))
    got, kept = _probe(ops, dev, V, idx, vals2, p, V)
    lower = min(idx[order.index(4)], idx[order.index(5)])
    assert sorted(kept) == sorted([idx[i] for i in range(10) if order[i] < 4] + [lower]), (V, kept)


# ---- 3. degenerate rows --------------------------------------------------------------------------------------------------------------
def test_degenerate_rows(ops, dev):
    one = torch.zeros(3, 1)
    for p in PS:
        assert _sample(ops, dev, _pad(one, dev), 1, 1, 1.0, True, top_p=p, uniform=torch.rand(3, 1).to(dev)).tolist() == [0, 0, 0]
        assert _sample(ops, dev, _pad(one, dev), 1, 1, 1.0, False, top_p=p, seed=SEED).tolist() == [0, 0, 0]
    for V in (1025, 2049, 8193):
        g = torch.Generator().manual_seed(V)
        x = torch.randn(8, V, generator=g)
        where = torch.randint(0, V - 1, (8,), generator=g)
        x[torch.arange(8), where] = 200.0                                    # every other weight underflows to a mass of 0
        u = torch.rand(8, V, generator=g)
        lg, ud = _pad(x, dev), u.to(dev)
        greedy = _ids(dev, 8)
        for p in PS + [1e-6]:
            for k in (max(int(0.1 * V), 1), V):
                assert _sample(ops, dev, lg, V, k, 0.7, True, top_p=p, uniform=ud).cpu().tolist() == where.tolist(), (V, p, k)
            # k = 1: the nucleus of one entry is that entry
            y = _pad(torch.randn(8, V, generator=g), dev)
            ops.sample_topk_gumbel(y, ud, greedy, V, 1, 0.7, True)
            assert torch.equal(_sample(ops, dev, y, V, 1, 0.7, True, top_p=p, uniform=ud), greedy), (V, p)


# ---- 4. seams: the same row on two kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1088, 2048, 4096, 16384])
def test_same_row_across_a_seam_gives_the_same_ids(ops, dev, V):
    """A row of V logits, and the same row with one forbidden logit appended (V + 1: the next instantiation -- at 2048 the workgroup kernel
    instead of the wave kernel): identical ids for every p, exactly.  The masses are integers, so no sum depends on who forms it."""
    g = torch.Generator().manual_seed(V)
    B = 16
    x = torch.randn(B, V, generator=g) * 3
    x[1] = torch.randint(0, 4, (V,), generator=g).float()
    x[2] = torch.randint(0, 2, (V,), generator=g).float() * 0.25
    u = torch.rand(B, V, generator=g)
    x1 = torch.cat([x, torch.full((B, 1), 50.0)], dim=1)                     # would win if it were not forbidden
    u1 = torch.cat([u, torch.full((B, 1), U_TOP)], dim=1)
    lg, lg1, ud, ud1 = _pad(x, dev), _pad(x1, dev), u.to(dev), u1.to(dev)
    for k in (7, max(int(0.1 * V), 1), V):
        for T in (0.4, 1.0):
            for p in PS + [0.3, 0.7]:
                a = _sample(ops, dev, lg, V, k, T, False, top_p=p, uniform=ud)
                b = _sample(ops, dev, lg1, V + 1, k, T, True, top_p=p, uniform=ud1)
                assert torch.equal(a, b), (V, k, T, p, a.tolist(), b.tolist())


# ---- 5. top_p = 1 through omlm_sample is each of the six entry points -----------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2049])
def test_top_p_one_equals_the_six_entry_points(ops, dev, V):
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    B, steps, D, ld, row0 = 6, 3, 64, (V + 7) // 8 * 8 + 9, 2
    k, T = max(int(0.1 * V), 1), 0.95
    g = torch.Generator().manual_seed(V)
    U = torch.rand(steps, B, V, generator=g).to(dev)
    lo, hi = ops.split_seed(SEED)
    E = V + 3
    emb = torch.randn(E, D, generator=g).to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    mk = lambda *shape: torch.full(shape, -7, dtype=torch.long, device=dev)  # noqa: E731
    hists = {n: (mk(steps, B), mk(steps, B)) for n in ("at", "at_rng", "embed", "embed_rng")}
    for t in range(steps):
        lg = _pad(torch.randn(B, V, generator=g) * 4, dev)
        for top_p in (None, 1.0):
            # plain forms
            want, got = mk(B), mk(B)
            ops.sample_topk_gumbel(lg, U[t], want, V, k, T, True)
            ops.sample(lg, got, V, k, T, True, top_p=top_p, uniform=U[t])
            assert torch.equal(got, want)
            ops.sample_topk_gumbel_rng(lg, SEED, t, row0, want, V, k, T, True)
            ops.sample(lg, got, V, k, T, True, top_p=top_p, seed=SEED, step=t, row0=row0)
            assert torch.equal(got, want)
        # replayable forms: *step_dev selects the uniforms and the hist slot
        for name, rng in (("at", False), ("at_rng", True)):
            want, got = mk(B), mk(B)
            if rng:
                call("omlm_sample_topk_gumbel_at_rng", ptr(lg), lo, hi, ptr(step_dev), row0, ptr(want), ptr(hists[name][0]), B, V, ld, k, T, 1,
                     stream_ptr())
                ops.sample(lg, got, V, k, T, True, seed=SEED, row0=row0, step_dev=step_dev, hist=hists[name][1])
            else:
                call("omlm_sample_topk_gumbel_at", ptr(lg), ptr(U), ptr(step_dev), ptr(want), ptr(hists[name][0]), B, V, ld, k, T, 1, stream_ptr())
                ops.sample(lg, got, V, k, T, True, uniform=U, step_dev=step_dev, hist=hists[name][1])
            assert torch.equal(got, want), (name, t)
        for name, rng in (("embed", False), ("embed_rng", True)):
            want, got = mk(B), mk(B)
            xw, xg = torch.full((B, D), NAN, device=dev), torch.full((B, D), NAN, device=dev)
            if rng:
                call("omlm_sample_embed_at_rng", ptr(lg), lo, hi, ptr(step_dev), row0, ptr(want), ptr(hists[name][0]), B, V, ld, k, T, 1,
                     ptr(emb), 7, E, ptr(xw), D, stream_ptr())
                ops.sample(lg, got, V, k, T, True, seed=SEED, row0=row0, step_dev=step_dev, hist=hists[name][1], emb_table=emb,
                           emb_row_offset=7, x=xg)
            else:
                call("omlm_sample_embed_at", ptr(lg), ptr(U), ptr(step_dev), ptr(want), ptr(hists[name][0]), B, V, ld, k, T, 1,
                     ptr(emb), 7, E, ptr(xw), D, stream_ptr())
                ops.sample(lg, got, V, k, T, True, uniform=U, step_dev=step_dev, hist=hists[name][1], emb_table=emb, emb_row_offset=7, x=xg)
            assert torch.equal(got, want) and torch.equal(xg, xw) and torch.equal(xg, emb[(want + 7).clamp(0, E - 1)]), (name, t)
        if t < steps - 1:
            call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())
    assert int(step_dev.item()) == steps - 1
    for name, (hw, hg) in hists.items():
        assert torch.equal(hg, hw) and int(hw.min()) >= 0, name


def test_bad_top_p_is_refused_by_name_before_any_launch(ops, dev):
    from open_musiclm_amd.hip import call, stream_ptr
    import ctypes
    lg, out = torch.zeros(2, 64, device=dev), _ids(dev, 2)
    for bad in (0.0, -1.0, 1.5, NAN):
        with pytest.raises(ValueError, match="top_p"):
            ops.sample(lg, out, 64, 8, 1.0, False, top_p=bad, seed=1)
        a = ops.SampleArgs(lg.data_ptr(), 2, 64, 64, None, 1, 0, 0, 0, None, out.data_ptr(), None, 8, 1.0, bad, 0)
        with pytest.raises(RuntimeError, match="top_p"):
            call("omlm_sample", ctypes.addressof(a), stream_ptr())
    assert out.tolist() == [-7, -7]


# ---- 6. the counter stream against the buffer, with a nucleus ------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 2048, 2049, 8193, 65536])
def test_stream_form_equals_buffer_form_with_a_nucleus(ops, dev, V):
    B, steps, D, row0 = 5, 3, 64, 3
    k, T = max(int(0.1 * V), 1), 0.9
    g = torch.Generator().manual_seed(V + 1)
    U = torch.from_numpy(S.uniforms(SEED, steps, B, V, row0=row0)).to(dev)
    emb = torch.randn(V + 3, D, generator=g).to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    hb, hr = (torch.full((steps, B), -7, dtype=torch.long, device=dev) for _ in range(2))
    for t in range(steps):
        x = torch.randn(B, V, generator=g) * 4
        x[1] = torch.randint(0, 4, (V,), generator=g).float()
        lg = _pad(x, dev)
        for p in (0.05, 0.5, 0.9):
            for forbid in (False, True):
                a = _sample(ops, dev, lg, V, k, T, forbid, top_p=p, uniform=U[t])
                b = _sample(ops, dev, lg, V, k, T, forbid, top_p=p, seed=SEED, step=t, row0=row0)
                assert torch.equal(a, b), (V, t, p, forbid, a.tolist(), b.tolist())
        a = _sample(ops, dev, lg, V, k, T, True, top_p=0.5, uniform=U, step_dev=step_dev, hist=hb)
        b = _sample(ops, dev, lg, V, k, T, True, top_p=0.5, seed=SEED, row0=row0, step_dev=step_dev, hist=hr)
        assert torch.equal(a, b) and torch.equal(hb[t], a) and torch.equal(hr[t], a) and bool((hr[t + 1:] == -7).all()), (V, t)
        xa, xb = torch.full((B, D), NAN, device=dev), torch.full((B, D), NAN, device=dev)
        ea = _sample(ops, dev, lg, V, k, T, True, top_p=0.5, uniform=U, step_dev=step_dev, emb_table=emb, emb_row_offset=1, x=xa)
        eb = _sample(ops, dev, lg, V, k, T, True, top_p=0.5, seed=SEED, row0=row0, step_dev=step_dev, emb_table=emb, emb_row_offset=1, x=xb)
        assert torch.equal(ea, a) and torch.equal(eb, a) and torch.equal(xa, xb) and torch.equal(xa, emb[a + 1]), (V, t)
        ops_call_advance(step_dev)
    assert int(step_dev.item()) == steps


def ops_call_advance(step_dev):
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    call("omlm_decode_advance", None, ptr(step_dev), stream_ptr())


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 8193])
def test_two_launches_give_the_same_ids(ops, dev, V):
    x, u = P.compare_rows(16384)
    lg, ud = _pad(x[:, :V].contiguous(), dev), u[:, :V].contiguous().to(dev)
    for p in PS:
        for k in (max(int(0.1 * V), 1), V):
            a = _sample(ops, dev, lg, V, k, 0.8, True, top_p=p, uniform=ud)
            b = _sample(ops, dev, lg, V, k, 0.8, True, top_p=p, uniform=ud)
            assert torch.equal(a, b), (V, p, k)


# ---- 8. the law on the device --------------------------------------------------------------------------------------------------------
def test_sampling_law_with_a_nucleus_on_the_device(ops, dev):
    """The 64-logit row, k = 16, T = 0.7 of the stream test; p halfway between the mass before the 6th and before the 7th of the 16 kept
    entries, so the nucleus has 6.  4096 steps x 16 rows on the counter stream: no id outside the nucleus, and chi^2 against the
    renormalised nucleus probabilities below mean + 6 sigma of its 5 degrees of freedom (5 + 6 sqrt(10) = 24.0)."""
    logits = np.float32(np.random.default_rng(0).standard_normal(64) * 2)
    k, T, steps, B, n = 16, 0.7, 4096, 16, 6
    l64 = logits.astype(np.float64)
    rank = np.argsort(-l64, kind="stable")[:k]                               # no ties among 64 normal draws
    w = np.exp((l64[rank] - l64[rank[0]]) / T)
    before = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    p = float((before[n - 1] + before[n]) / 2 / w.sum())
    nucleus = np.zeros(64, dtype=bool)
    nucleus[rank[:n]] = True
    assert P.nucleus_mask(torch.from_numpy(logits)[None], k, T, p, False)[0].numpy().tolist() == nucleus.tolist()
    lg = torch.from_numpy(logits)[None].repeat(B, 1).contiguous().to(dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(B, dtype=torch.long, device=dev)
    hist = torch.full((steps, B), -7, dtype=torch.long, device=dev)
    for _ in range(steps):
        ops.sample(lg, out, 64, k, T, False, top_p=p, seed=SEED, step_dev=step_dev, hist=hist)
        ops_call_advance(step_dev)
    ids = hist.cpu().numpy().ravel()
    assert int(step_dev.item()) == steps and ids.min() >= 0 and ids.max() < 64
    counts = np.bincount(ids, minlength=64).astype(np.float64)
    assert counts[~nucleus].sum() == 0
    prob = np.where(nucleus, np.exp((l64 - l64.max()) / T), 0.0)
    expected = prob / prob.sum() * steps * B
    chi2 = float((((counts - expected) ** 2)[nucleus] / expected[nucleus]).sum())
    bound = (n - 1) + 6 * (2 * (n - 1)) ** 0.5
    print(f"top-p law on the device: p {p:.4f}, chi2_{n - 1} {chi2:.1f} (bound {bound:.1f}), smallest expected count {expected[nucleus].min():.0f}")
    report("sampler_top_p_law_device", chi2=chi2, bound=bound, p=p)
    assert chi2 < bound, chi2


# ---- 9. generate() -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny2048(dev):
    wrapper = _tiny(dev, 2048)
    cond = [torch.randint(0, 32, (2, 3, 2), generator=torch.Generator().manual_seed(5)).to(dev)]
    return wrapper, cond


@pytest.mark.parametrize("route", list(ROUTES))
def test_generate_with_a_nucleus(dev, tiny2048, route):
    """V1 = 2049, B = 2, 8 ids on the cached loop, the re-forward route and the captured-graph loop."""
    wrapper, cond = tiny2048
    steps, V1, kw = 8, 2049, ROUTES[route]
    gen = lambda **k: wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, **kw, **k)  # noqa: E731
    for s in (3, SEED):
        U = torch.from_numpy(S.uniforms(s, steps, 2, V1))
        want = gen(top_p=0.5, uniforms=U)
        got = gen(top_p=0.5, sampler_rng="counter", sampler_seed=s)
        assert got.shape == (2, steps, 1) and torch.equal(got, want), (route, s, got.tolist(), want.tolist())
        assert int(got.min()) >= 0 and int(got.max()) < 2048
    # a nucleus of one entry is greedy decoding: k = 1 by filter_thres = 1 keeps the same first maximum
    greedy = gen(filter_thres=1.0, sampler_rng="counter", sampler_seed=5)
    assert torch.equal(gen(top_p=1e-6, sampler_rng="counter", sampler_seed=6), greedy)
    assert torch.equal(gen(top_p=1e-6, uniforms=U), greedy)
    # the nucleus changes ids; top_p = 1 and None do not
    plain = gen(uniforms=U)
    assert torch.equal(gen(top_p=1.0, uniforms=U), plain) and torch.equal(gen(top_p=None, uniforms=U), plain)
    assert torch.equal(gen(top_p=1.0, sampler_rng="counter", sampler_seed=SEED), plain)
    assert not torch.equal(want, plain), (want.tolist(), plain.tolist())
    for bad in (0, -0.1, 1.01, NAN, "0.5x"):
        with pytest.raises(ValueError, match="top_p"):
            gen(top_p=bad)


def test_generate_with_a_nucleus_on_the_wide_route(dev):
    """B = 20 on the model of test_gpu_wide_codebook.test_wide_head_cached_steps_vs_oracle (dim 1024, 8 heads, depth 1, fp16, predicted
    codebook 2048): one decode call of more than 16 samples."""
    from open_musiclm_amd import decode
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    model = M.create_semantic_transformer(dim=1024, depth=1, heads=8, semantic_codebook_size=2048, ff_dropout=0.0, precision="fp16").to(dev)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    cond = [torch.randint(0, 1024, (20, 1, 12), generator=torch.Generator().manual_seed(8)).to(dev)]
    assert decode.max_call_batch(model, "fp16") >= 20 and decode.supports(model, 1, prompt_rows=20)
    steps, V1 = 6, 2049
    gen = lambda **k: wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, **k)  # noqa: E731
    U = torch.from_numpy(S.uniforms(9, steps, 20, V1))
    want = gen(top_p=0.5, uniforms=U)
    got = gen(top_p=0.5, sampler_rng="counter", sampler_seed=9)
    assert got.shape == (20, steps, 1) and torch.equal(got, want)
    assert torch.equal(gen(top_p=1e-6), gen(filter_thres=1.0))
    plain = gen(uniforms=U)
    assert not torch.equal(want, plain) and torch.equal(gen(top_p=1.0, uniforms=U), plain)


def test_musiclm_forward_takes_top_p_per_stage(dev, monkeypatch):
    """The tiny stages of test_gpu_model.test_musiclm_hierarchical_decode_tokens: shapes as without the argument; a nucleus of one entry
    in every stage equals greedy decoding (filter_thres = 1 handed to every stage)."""
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    kw = dict(dim=64, depth=1, heads=1, precision="bf16")
    sem = M.create_semantic_transformer(**kw).to(dev)
    coarse = M.create_coarse_transformer(num_coarse_quantizers=3, **kw).to(dev)
    fine = M.create_fine_transformer(num_coarse_quantizers=3, num_fine_quantizers=5, **kw).to(dev)
    mlm = M.MusicLM(wav2vec=None, clap=None, neural_codec=None, semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    args = dict(clap_token_ids=torch.randint(0, 1024, (1, 12, 1), device=dev), output_seconds=2, semantic_window_seconds=1,
                coarse_window_seconds=1, fine_window_seconds=1, semantic_steps_per_second=10, acoustic_steps_per_second=6, return_tokens=True)
    s, c, f = mlm.forward(top_p={"semantic": 0.9, "fine": 0.5}, **args)
    assert s.shape == (1, 20, 1) and c.shape[0] == 1 and c.shape[2] == 3 and f.shape[2] == 5 and c.shape[1] == f.shape[1]
    assert int(c.max()) < 1024 and int(c.min()) >= 0
    tiny = mlm.forward(top_p={"semantic": 1e-6, "coarse": 1e-6, "fine": 1e-6}, **args)
    tiny_all = mlm.forward(top_p=1e-6, **args)
    seen = []
    for stage in (mlm.semantic, mlm.coarse, mlm.fine):
        orig = stage.generate
        monkeypatch.setattr(stage, "generate", lambda _orig=orig, **k: (seen.append(k.get("top_p")), _orig(**{**k, "filter_thres": 1.0}))[1])
    greedy = mlm.forward(**args)
    assert seen and all(p is None for p in seen)
    for a, b, g in zip(tiny, tiny_all, greedy):
        assert torch.equal(a, g) and torch.equal(b, g)
    for bad in (0, 1.5, {"fine": 0}, {"acoustic": 0.5}):
        with pytest.raises(ValueError, match="top_p"):
            mlm.forward(top_p=bad, **args)
