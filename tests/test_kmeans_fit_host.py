"""CPU side of the device k-means fit: the fp64 restatement (tests/kmeans_fit_ref.py) against the reference's own golden fit, before anything
on the GPU is compared with the restatement; and the host logic of `learn_kmeans(..., device=...)` that needs no GPU."""
import ast
import inspect
import os

import numpy as np
import pytest
import torch

import kmeans_fit_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "kmeans_fit.npz"))
    return z["features"], z["centers"], ast.literal_eval(str(z["kwargs"]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_reaches_the_reference_inertia(golden, seed):
    """The restated rules, on the golden features with the golden keywords, land within 1 % of the inertia of the centres the REFERENCE
    fitted on the same rows (1.43206; sklearn's own seed-to-seed spread on these features is 0.08 %, the total variance 57.2, so 1 % is
    twelve times the reference's spread and far below the cost of one missed cluster)."""
    feats, centres, kw = golden
    want = R.inertia(feats.astype(np.float64), centres)
    out = R.fit(feats, R.ArrayDraws(seed), **kw)
    print(f"seed {seed}: restatement {out['inertia']:.5f}, reference centres {want:.5f}, ratio {out['inertia'] / want:.5f}, "
          f"{out['n_steps']} steps")
    assert out["inertia"] <= 1.01 * want
    assert (out["counts"] > 0).all()


def test_candidate_rule_skips_rows_of_weight_zero():
    """The inverse-CDF rule as stated: first row whose cumulative weight exceeds u * total; a row of weight zero is never drawn, u = 0
    draws the first row of positive weight, the largest u below 1 the last one."""
    closest = np.array([0.0, 2.0, 0.0, 0.0, 1.0, 1.0, 0.0])
    u = np.array([0.0, 0.49, 0.5, 0.74, 0.75, R.ONE_BELOW], np.float32)
    assert R.pp_candidates(closest, u).tolist() == [1, 1, 4, 4, 5, 5]
    assert R.pp_candidates(np.zeros(5), np.array([0.3], np.float32)).tolist() == [4]          # nothing left to draw: clipped to m - 1


def test_seeding_fp32_against_fp64_stays_under_the_near_tie_cap():
    """The GPU test compares every pick of a seeding on Gaussian rows with this restatement and tolerates a different row only where the
    restatement's two best potentials lie within fp32 rounding of each other, at most 1 % of the picks.  Checked here on the same inputs:
    the restatement with its distances in fp32 against itself in fp64 picks the same rows, pick by pick from the fp64 state."""
    rng = np.random.RandomState(11)
    m, D, K, trials = 2000, 32, 64, 6
    X = rng.standard_normal((m, D)).astype(np.float32)
    u = R.ArrayDraws(5).seeding_uniforms(K, trials).numpy()
    ref = R.pp_seed(X, u, K, record=True)
    differ = 0
    for k in range(1, K):
        closest = ref["record"]["closest"][k - 1].astype(np.float32)
        cands = R.pp_candidates(closest, u[k])
        d32 = ((X[:, None, :] - X[cands][None, :, :]) ** 2).sum(-1, dtype=np.float32)
        w32 = int(np.argmin(np.minimum(closest[:, None], d32).sum(0, dtype=np.float64)))
        w64, _, _ = R.pp_pick(X, closest, cands)
        differ += int(cands[w32] != cands[w64])
    assert differ <= 0.01 * (K - 1), differ


def test_learn_kmeans_default_is_the_host_path():
    from open_musiclm_amd.hf_hubert_kmeans import learn_kmeans
    sig = inspect.signature(learn_kmeans)
    assert sig.parameters["device"].default is None
    assert list(sig.parameters)[-1] == "device"                     # the one new keyword, after the reference's


def test_learn_kmeans_device_arguments(golden, tmp_path):
    from open_musiclm_amd.hf_hubert_kmeans import learn_kmeans
    from open_musiclm_amd.kmeans_fit import GpuMiniBatchKMeans
    feats, _, kw = golden
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        learn_kmeans(feats, 0, str(tmp_path / "a.joblib"), device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="reassignment_ratio"):
        learn_kmeans(feats, 0, str(tmp_path / "a.joblib"), device="cuda", reassignment_ratio=0.1, **kw)
    with pytest.raises(NotImplementedError, match="init"):
        learn_kmeans(feats, 0, str(tmp_path / "a.joblib"), device=torch.device("cuda"), init=np.zeros((16, 16)), **kw)
    with pytest.raises(NotImplementedError, match="reassignment_ratio"):
        GpuMiniBatchKMeans(reassignment_ratio=0.01)
    assert not (tmp_path / "a.joblib").exists()


def test_trainer_rejects_a_cpu_fit_device(golden, tmp_path):
    from open_musiclm_amd.hf_hubert_kmeans import HfHubertWithKmeans
    from open_musiclm_amd.trainer import HfHubertKmeansTrainer
    feats, _, kw = golden

    class Feats(torch.utils.data.Dataset):
        def __len__(self): return len(feats) // 30
        def __getitem__(self, i): return torch.from_numpy(feats[30 * i:30 * (i + 1)])
    hk = HfHubertWithKmeans(hubert=None, kmeans=None, codebook_size=kw["n_clusters"])
    trainer = HfHubertKmeansTrainer(feature_extraction_num_steps=2, feature_extraction_batch_size=25, hubert_kmeans=hk, dataset=Feats(),
                                    results_folder=str(tmp_path / "km"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer.train(device="cpu", verbose=0)


def test_fitted_kmeans_round_trips_without_a_gpu(golden, tmp_path):
    """What the device fit dumps is plain host data: it loads through joblib, get_hubert_kmeans and HfHubertWithKmeans on a machine
    without a GPU, and through the `open_musiclm` alias package."""
    import joblib
    import open_musiclm.kmeans_fit  # noqa: F401  (the alias package lists the new module)
    from open_musiclm.hf_hubert_kmeans import FittedKmeans as AliasFitted
    from open_musiclm_amd.hf_hubert_kmeans import FittedKmeans, HfHubertWithKmeans, get_hubert_kmeans
    assert AliasFitted is FittedKmeans
    _, centres, kw = golden
    fitted = FittedKmeans(centres, 1.25, 37, np.arange(16), seed=3, params=kw)
    path = str(tmp_path / "kmeans.joblib")
    joblib.dump(fitted, path)
    back = joblib.load(path)
    assert type(back) is FittedKmeans and back.cluster_centers_.dtype == np.float32
    assert np.array_equal(back.cluster_centers_, centres.astype(np.float32)) and back.inertia_ == 1.25 and back.n_steps_ == 37
    assert back.params == kw and back.seed == 3 and np.array_equal(back.counts_, np.arange(16, dtype=np.float32))
    for v in vars(back).values():
        assert not isinstance(v, torch.Tensor)
    hk = HfHubertWithKmeans(hubert=None, kmeans=back)
    assert hk.codebook_size == 16 and tuple(hk.kmeans.centroids.shape) == (16, 16) and hk.kmeans.centroids.device.type == "cpu"
    hk2 = get_hubert_kmeans(kmeans_path=path)
    assert torch.equal(hk2.kmeans.centroids, hk.kmeans.centroids)
