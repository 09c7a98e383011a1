"""GPU: the device k-means fit (csrc/kmeans_fit.hip, open_musiclm_amd/kmeans_fit.py) against the fp64 restatement tests/kmeans_fit_ref.py
on identical injected draws, and `learn_kmeans(..., device='cuda')` / `HfHubertKmeansTrainer.train(device='cuda')` end to end."""
import ast
import os

import numpy as np
import pytest
import torch

import kmeans_fit_ref as R
from rvq_cases import grid_uniform
from test_gpu_kernels import dev, ops, relerr, report  # noqa: F401  (the shared fixtures)

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -24


class Seeder:
    """device buffers of one k-means++ run through the C ABI"""

    def __init__(self, ops, dev, X, uniforms, K):
        self.ops, self.K = ops, K
        self.m, self.D = X.shape
        self.trials = uniforms.shape[1]
        self.rows = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(dev)
        self.u = torch.from_numpy(np.ascontiguousarray(uniforms, np.float32)).to(dev)
        self.closest = torch.zeros(self.m, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.centres = torch.zeros(K, self.D, device=dev)
        self.centres_T = torch.zeros(self.D, K, device=dev)
        self.chosen = torch.full((K,), -1, dtype=torch.int32, device=dev)
        self.pots = torch.zeros(K, dtype=torch.float64, device=dev)
        self.ws = torch.zeros(ops.kmeans_pp_workspace_bytes(self.m, self.trials) // 4 + 4, device=dev)

    def args(self):
        return (self.rows, self.closest, self.u, self.counter, self.centres, self.centres_T, self.chosen, self.pots, self.ws, self.K,
                self.trials)

    def seed(self):
        self.ops.kmeans_pp_seed(*self.args())
        torch.cuda.synchronize()

    def pick(self, k, closest):
        self.closest.copy_(torch.from_numpy(np.asarray(closest, np.float32)))
        self.counter.fill_(k)
        self.ops.kmeans_pp_pick(*self.args())
        torch.cuda.synchronize()


def _grid_case(m, D, K, trials, seed):
    """coordinates on the 2^-3 grid in [-2, 2]: every squared distance is a multiple of 2^-6 below 2^24 * 2^-6 (D <= 64), so the fp32
    distances, their sums in any order and the fp64 potentials are exact; duplicated rows make exact ties and rows of weight zero."""
    rng = np.random.RandomState(seed)
    X = grid_uniform(rng, (m, D), 2.0)
    X[m // 2:m // 2 + 20] = X[:20]                    # duplicates: weight zero once their twin is a centre, equal potentials as candidates
    u = R.ArrayDraws(seed).seeding_uniforms(K, trials).numpy()
    return X, u


@pytest.mark.parametrize("m,D,K,trials", [(700, 24, 32, 5), (300, 23, 8, 4), (5000, 64, 40, 11), (20000, 16, 12, 8)])
def test_pp_seeding_matches_the_restatement_exactly(ops, dev, m, D, K, trials):
    """One pick from the restatement's state and one whole seeding, on exactly representable inputs: chosen rows, potentials, the closest
    vector and both centre layouts EQUAL; a second run gives identical bytes."""
    X, u = _grid_case(m, D, K, trials, seed=m + D)
    ref = R.pp_seed(X, u, K, record=True)
    s = Seeder(ops, dev, X, u, K)
    k = K // 2
    s.pick(k, ref["record"]["closest"][k - 1])
    w = int(np.argmin(ref["record"]["pots"][k - 1]))
    assert int(s.chosen[k]) == int(ref["chosen"][k]) == int(ref["record"]["cands"][k - 1][w])
    assert float(s.pots[k]) == float(ref["pots"][k])
    assert int(s.counter) == k + 1
    want_closest = ref["record"]["closest"][k] if k + 1 < K else ref["closest"]
    assert np.array_equal(s.closest.cpu().numpy().astype(np.float64), want_closest)
    assert np.array_equal(s.centres[k].cpu().numpy(), X[ref["chosen"][k]])

    s.seed()
    got = s.chosen.cpu().numpy()
    report(f"kmeans_pp_seed_exact_{m}x{D}_K{K}_t{trials}", equal=bool((got == ref["chosen"]).all()))
    assert np.array_equal(got, ref["chosen"])
    assert np.array_equal(s.pots.cpu().numpy(), ref["pots"])
    assert np.array_equal(s.centres.cpu().numpy(), X[ref["chosen"]])
    assert np.array_equal(s.centres_T.cpu().numpy(), X[ref["chosen"]].T)
    assert np.array_equal(s.closest.cpu().numpy().astype(np.float64), ref["closest"])
    assert int(s.counter) == K
    first = (s.centres.clone(), s.closest.clone(), s.pots.clone())
    s.seed()
    assert torch.equal(first[0], s.centres) and torch.equal(first[1], s.closest) and torch.equal(first[2], s.pots)


def test_pp_picks_on_gaussian_rows(ops, dev):
    """Every pick of a seeding on its own, started from the restatement's state (its closest vector rounded to fp32, which both sides then
    use), so that one differing pick does not carry into the next.  The chosen row must equal the restatement's except where the
    restatement's two best potentials lie within fp32 rounding of each other: relative gap below 2 D 2^-24, the worst-case rounding of a
    D-term fp32 sum of squares.  Those are counted and may not exceed 1 % of the picks (tests/test_kmeans_fit_host.py checks on the CPU
    that these inputs keep the restatement itself, fp32 against fp64, under the cap)."""
    rng = np.random.RandomState(11)
    m, D, K, trials = 2000, 32, 64, 6
    X = rng.standard_normal((m, D)).astype(np.float32)
    u = R.ArrayDraws(5).seeding_uniforms(K, trials).numpy()
    ref = R.pp_seed(X, u, K, record=True)
    s = Seeder(ops, dev, X, u, K)
    near_ties, worst = 0, 0.0
    for k in range(1, K):
        closest = ref["record"]["closest"][k - 1].astype(np.float32)
        cands = R.pp_candidates(closest, u[k])
        w, pots, new_closest = R.pp_pick(X, closest, cands)
        s.pick(k, closest)
        got = int(s.chosen[k])
        assert got in cands.tolist(), (k, got, cands)                      # the inverse-CDF draw itself (fp64 on both sides)
        if got != int(cands[w]):
            two = np.sort(pots)[:2]
            gap = (two[1] - two[0]) / two[0]
            assert gap < 2 * D * F32_EPS, f"pick {k}: row {got} instead of {int(cands[w])} with potentials {pots}"
            near_ties += 1
        else:
            worst = max(worst, relerr(s.closest.cpu(), torch.from_numpy(new_closest)), abs(float(s.pots[k]) / pots[w] - 1.0))
    report("kmeans_pp_picks_gaussian", near_ties=near_ties, picks=K - 1, worst_rel=worst)
    print(f"near ties {near_ties} of {K - 1} picks, worst relative error of closest / potential {worst:.2e}")
    assert near_ties <= 0.01 * (K - 1)
    assert worst < 1e-5


def test_minibatch_step_against_the_restatement(ops, dev):
    """One step (then a second, for the device stop state): assignment in the fp32 arithmetic of oracle.kmeans_assign (which the assign
    kernel matches bit for bit), sums in fp64.  Counts equal; centres and batch inertia to 1e-5 relative (fp32 sums of <= 10^4 rows
    against fp64; the order of the atomics is the only freedom)."""
    from oracle import musiclm_oracle as O
    rng = np.random.RandomState(3)
    n, D, K, B = 5000, 48, 64, 2001
    X = rng.standard_normal((n, D)).astype(np.float32)
    C = X[rng.permutation(n)[:K]].copy()
    C[7] += 100.0                                                        # a centre that receives nothing keeps its place and count
    counts0 = rng.randint(0, 50, K).astype(np.float64)
    idx = rng.randint(0, n, (2, B))
    x = torch.from_numpy(X).to(dev)
    centres = torch.from_numpy(C).to(dev)
    centres_T = centres.t().contiguous()
    counts = torch.from_numpy(counts0.astype(np.float32)).to(dev)
    bcounts, sums = torch.zeros(K, device=dev), torch.zeros(K, D, device=dev)
    rowmin, move = torch.zeros(B, device=dev), torch.zeros(K, dtype=torch.float64, device=dev)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    alpha = min(1.0, 2.0 * B / (n + 1))
    Cr, cr = C.astype(np.float64), counts0.copy()
    stop = R.StopState(alpha, 0.0, 10)
    for step in range(2):
        cur32 = Cr.astype(np.float32) if step == 0 else centres.cpu().numpy()      # the assignment sees the kernel's own fp32 centres
        labels = O.kmeans_assign(X[idx[step]], cur32)
        if step == 1:
            Cr = cur32.astype(np.float64)
        bi, mv, mk = R.minibatch_step(X[idx[step]], Cr, cr, labels=labels)
        stop.update(bi, mv)
        ops.kmeans_minibatch_step(x, torch.from_numpy(idx[step].astype(np.int32)).to(dev), centres, centres_T, counts, bcounts, sums,
                                  rowmin, move, state, alpha, 0.0, 10)
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        live = np.arange(K) != 7                                          # the far centre would only inflate the scale of the comparison
        e_c = relerr(centres.cpu()[live], torch.from_numpy(Cr[live]))
        e_i = abs(st[2] / bi - 1.0)
        print(f"step {step}: centres rel err {e_c:.2e}, batch inertia rel err {e_i:.2e}, movement {st[3]:.6f} / {mv:.6f}")
        report(f"kmeans_minibatch_step_{step}", centres=e_c, inertia=e_i)
        assert np.array_equal(counts.cpu().numpy().astype(np.float64), cr)
        assert mk[7] == 0 and np.array_equal(centres[7].cpu().numpy(), C[7])
        assert e_c < 1e-5 and e_i < 1e-5
        assert abs(st[3] / mv - 1.0) < 1e-3
        assert torch.equal(centres_T, centres.t())
        assert int(st[4]) == step + 1 and float(bcounts.abs().sum()) == 0.0 and float(sums.abs().sum()) == 0.0
    assert abs(st[0] / stop.ewa - 1.0) < 1e-5 and st[6] == 0.0
    # a step behind a stop changes nothing
    state[6] = 1.0
    before = (centres.clone(), counts.clone(), state.clone())
    ops.kmeans_minibatch_step(x, torch.from_numpy(idx[0].astype(np.int32)).to(dev), centres, centres_T, counts, bcounts, sums, rowmin, move,
                              state, alpha, 0.0, 10)
    torch.cuda.synchronize()
    assert torch.equal(before[0], centres) and torch.equal(before[1], counts) and torch.equal(before[2], state)


@pytest.mark.parametrize("n", [1, 255, 10_000, 1_000_000])
def test_inertia_against_fp64(ops, dev, n):
    """sum over rows of the min squared distance against fp64 on the same fp32 inputs: 1e-6 relative, up to 10^6 rows."""
    rng = np.random.RandomState(n % 1000)
    D, K = 16, 32
    X = rng.standard_normal((n, D)).astype(np.float32)
    C = rng.standard_normal((K, D)).astype(np.float32)
    want = R.inertia(X, C) * n
    x, cT = torch.from_numpy(X).to(dev), torch.from_numpy(C).to(dev).t().contiguous()
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    labels = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ops.kmeans_inertia(x, cT, out, labels)
    err = abs(float(out) / want - 1.0)
    print(f"n = {n}: {float(out):.6f} against {want:.6f}, relative error {err:.2e}")
    report(f"kmeans_inertia_{n}", err=err)
    assert err < 1e-6
    idx = torch.empty(n, 1, dtype=torch.int32, device=dev)
    ops.nearest_centroid(x, cT, idx, n, D, K)
    assert torch.equal(idx[:, 0], labels)                                # the same arithmetic as the assign kernel, bit for bit


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "kmeans_fit.npz"))
    return z["features"], z["centers"], ast.literal_eval(str(z["kwargs"]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_learn_kmeans_on_the_device_reaches_the_reference_inertia(dev, golden, tmp_path, seed):
    """The whole fit on the golden features with the golden keywords: inertia_ <= 1.01 x the inertia of the reference's golden centres on
    the same rows (computed here from the .npz; where the 1 % comes from: tests/test_kmeans_fit_host.py), no empty cluster, and the dumped
    model loads through get_hubert_kmeans."""
    import joblib
    from open_musiclm_amd.hf_hubert_kmeans import FittedKmeans, get_hubert_kmeans, learn_kmeans
    feats, centres, kw = golden
    want = R.inertia(feats.astype(np.float64), centres)
    path = str(tmp_path / "km.joblib")
    km = learn_kmeans(feats, seed, path, verbose=0, device="cuda", **kw)
    print(f"seed {seed}: inertia {km.inertia_:.5f} against the reference centres' {want:.5f} (ratio {km.inertia_ / want:.5f}), "
          f"{km.n_steps_} steps, stop: {km.stop_reason_}")
    report(f"kmeans_fit_golden_seed{seed}", inertia=km.inertia_, reference=want)
    assert km.inertia_ <= 1.01 * want
    assert abs(km.inertia_ / R.inertia(feats.astype(np.float64), km.cluster_centers_.astype(np.float64)) - 1.0) < 1e-5
    assert abs(-km.score(feats) / len(feats) / km.inertia_ - 1.0) < 1e-9
    labels = km.predict(feats)
    assert labels.dtype == np.int64 and len(np.unique(labels)) == kw["n_clusters"]
    assert km.cluster_centers_.dtype == np.float32 and km.cluster_centers_.shape == centres.shape
    assert km.counts_.sum() == km.n_steps_ * kw["batch_size"]
    loaded = joblib.load(path)
    assert type(loaded) is FittedKmeans and np.array_equal(loaded.cluster_centers_, km.cluster_centers_)
    hk = get_hubert_kmeans(kmeans_path=path).to(dev)
    assert torch.equal(hk.kmeans.predict(torch.from_numpy(feats).to(dev)).cpu(), torch.from_numpy(labels))


def test_fit_is_reproducible_for_a_seed_and_an_input_kind(dev, golden, tmp_path):
    """The same seed twice, and a numpy array against a CUDA tensor: the same seeding bit for bit; the final inertia_ equal to 1e-5
    relative (the mini-batch sums go through fp32 atomics, whose order is free).  The global RNGs are not touched."""
    from open_musiclm_amd.hf_hubert_kmeans import learn_kmeans
    feats, _, kw = golden
    torch.manual_seed(123)
    np.random.seed(123)
    t_state, c_state, n_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev), np.random.get_state()[1].copy()
    a = learn_kmeans(feats, 7, str(tmp_path / "a.joblib"), verbose=0, device="cuda", **kw)
    b = learn_kmeans(feats, 7, str(tmp_path / "b.joblib"), verbose=0, device=dev, **kw)
    c = learn_kmeans(torch.from_numpy(feats).to(dev), 7, str(tmp_path / "c.joblib"), verbose=0, device="cuda", **kw)
    d = learn_kmeans(feats, 8, str(tmp_path / "d.joblib"), verbose=0, device="cuda", **kw)
    assert torch.equal(t_state, torch.get_rng_state()) and torch.equal(c_state, torch.cuda.get_rng_state(dev))
    assert np.array_equal(n_state, np.random.get_state()[1])
    for other in (b, c):
        assert np.array_equal(a.init_chosen_, other.init_chosen_) and a.best_init_ == other.best_init_
        assert np.array_equal(a.init_centers_, other.init_centers_) and np.array_equal(a.init_inertias_, other.init_inertias_)
        assert abs(a.inertia_ / other.inertia_ - 1.0) < 1e-5
    assert not np.array_equal(a.init_chosen_, d.init_chosen_)


@pytest.fixture(scope="module")
def planted():
    """The shipped dimensions on a planted mixture, and the fp64 restatement of the fit on it (a few hundred GFLOP of numpy: once)."""
    X = R.planted_mixture(60_000, 768, 1024, scale=3.0, seed=0)
    kw = dict(n_clusters=1024, batch_size=10_000, max_iter=10, n_init=2, max_no_improvement=100)
    return X, kw, R.fit(X, R.ArrayDraws(0), **kw)


# Stream-to-stream spread of the RESTATEMENT on this case, measured on the CPU with four draw streams (ArrayDraws(0..3)): inertia
# 855.74, 845.92, 862.78, 827.26 -> (max - min) / min = 4.29 % (profiles/kmeans_fit.md).  The margin is twice that.
PLANTED_MARGIN = 2 * 0.0429


def test_fit_at_the_shipped_dimensions(dev, planted):
    """768-d, K = 1024, batch_size = 10000 (n_init 2 and max_iter 10 keep it short), 60 000 rows of a planted mixture, the same injected
    draws on both sides: inertia within PLANTED_MARGIN (8.6 %, twice the restatement's own stream-to-stream spread of 4.29 %) of the
    restatement's."""
    from open_musiclm_amd.kmeans_fit import GpuMiniBatchKMeans
    X, kw, ref = planted
    km = GpuMiniBatchKMeans(seed=0, device=dev, **kw)
    km.draw_source = R.ArrayDraws(0)
    km.record_times = True
    km.fit(X)
    same = float((km.init_chosen_ == ref["init_chosen"]).mean())
    print(f"inertia {km.inertia_:.4f} against the restatement's {ref['inertia']:.4f} (ratio {km.inertia_ / ref['inertia']:.5f}); "
          f"{km.n_steps_} / {ref['n_steps']} steps; seeding picks equal to the restatement's: {same:.4f}; times (ms) {km.times_ms_}")
    report("kmeans_fit_shipped_dims", inertia_gpu=km.inertia_, restatement=ref["inertia"], picks_equal=same, **km.times_ms_)
    assert abs(km.inertia_ / ref["inertia"] - 1.0) <= PLANTED_MARGIN
    assert km.n_steps_ == ref["n_steps"]
    assert len(np.unique(km.predict(X))) > 0.9 * kw["n_clusters"]


def test_trainer_fits_on_the_device(dev, golden, tmp_path):
    """HfHubertKmeansTrainer.train(device='cuda') on a features-in dataset (with a NaN row to filter): writes a kmeans.joblib that
    get_hubert_kmeans loads and whose assign ids match predict of the fitted estimator."""
    from open_musiclm_amd.hf_hubert_kmeans import HfHubertWithKmeans, get_hubert_kmeans
    from open_musiclm_amd.kmeans_fit import GpuMiniBatchKMeans
    from open_musiclm_amd.trainer import HfHubertKmeansTrainer
    feats, _, kw = golden
    feats = feats.copy()
    feats[17, 3] = np.nan

    class Feats(torch.utils.data.Dataset):            # one "clip" = 30 frames of precomputed features
        def __len__(self): return len(feats) // 30
        def __getitem__(self, i): return torch.from_numpy(feats[30 * i:30 * (i + 1)])
    hk = HfHubertWithKmeans(hubert=None, kmeans=None, codebook_size=kw["n_clusters"])
    trainer = HfHubertKmeansTrainer(feature_extraction_num_steps=4, feature_extraction_batch_size=25, hubert_kmeans=hk, dataset=Feats(),
                                    results_folder=str(tmp_path / "km"))
    trainer.train(seed=5, verbose=0, device="cuda", **{k: v for k, v in kw.items() if k != "n_clusters"})
    km = trainer.kmeans_model
    assert isinstance(km, GpuMiniBatchKMeans) and np.isfinite(km.cluster_centers_).all() and np.isfinite(km.inertia_)
    assert km.counts_.sum() == km.n_steps_ * kw["batch_size"]
    hk2 = get_hubert_kmeans(kmeans_path=str(tmp_path / "km" / "kmeans.joblib"), normalize_embeds=False).to(dev)
    clean = torch.from_numpy(feats[30:3000].reshape(-1, 30, 16)).to(dev)
    ids = hk2.assign(clean)
    assert torch.equal(ids.reshape(-1), km.predict(clean.reshape(-1, 16)))
