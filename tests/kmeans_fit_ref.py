"""fp64 numpy restatement of the device k-means fit (open_musiclm_amd/kmeans_fit.py, csrc/kmeans_fit.hip, include/omlm.h), consuming the
same injected draws.  Used by tests/test_kmeans_fit_host.py (CPU) and tests/test_gpu_kmeans_fit.py (GPU).  Plain test infrastructure.

Rules restated:
  * candidates of a pick: cum = cumsum(closest) in fp64, r = u * cum[-1], candidate = the first row with cum > r
    (`searchsorted(cum, r, side='right')`), clipped to m - 1: a row of weight zero is never drawn;
  * pick 0 is row min(floor(u[0, 0] * m), m - 1);
  * the candidate with the lowest potential sum_i min(closest_i, d_i) wins (ties: first);
  * mini-batch step: counts_k += m_k; c_k += (sum_k - m_k c_k) / counts_k; batch inertia with the centres before the update;
  * stopping: sklearn's _mini_batch_convergence (first step ignored, ewa with alpha = min(1, 2 B / (n + 1)), tol, max_no_improvement).
Distances are the expanded form |x|^2 + |c|^2 - 2 x.c in fp64, clipped at 0 (exact on the 2^-3 grid inputs of the equality tests)."""
import math

import numpy as np
import torch

ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


class ArrayDraws:
    """A draw source for GpuMiniBatchKMeans.draw_source and for `fit` below: numpy streams keyed by (seed, kind, call / step), so the
    kernels and the restatement read identical draws whatever the chunking of the batches."""

    def __init__(self, seed):
        self.seed = int(seed)
        self.calls = {"rows": 0, "uniforms": 0, "random": 0}

    def _rs(self, kind, i):
        return np.random.RandomState([self.seed, kind, i])

    def _next(self, what):
        self.calls[what] += 1
        return self.calls[what] - 1

    def init_rows(self, n, m):
        return torch.from_numpy(self._rs(1, self._next("rows")).randint(0, n, m).astype(np.int64))

    def seeding_uniforms(self, K, trials):
        u = self._rs(2, self._next("uniforms")).random_sample((K, trials)).astype(np.float32)
        return torch.from_numpy(np.minimum(u, np.float32(ONE_BELOW)))

    def random_rows(self, m, K):
        return torch.from_numpy(self._rs(4, self._next("random")).permutation(m)[:K].astype(np.int64))

    def batch_indices(self, step0, nsteps, B, n):
        return torch.from_numpy(np.stack([self._rs(3, step0 + s).randint(0, n, B) for s in range(nsteps)]).astype(np.int64))


def sqdist(X, C, x2=None):
    X = np.asarray(X, np.float64)
    C = np.asarray(C, np.float64)
    if x2 is None:
        x2 = (X * X).sum(1)
    return np.maximum(x2[:, None] + (C * C).sum(1)[None, :] - 2.0 * (X @ C.T), 0.0)


def pp_candidates(closest, u):
    """closest [m], u [trials] (float32 draws) -> candidate rows [trials]."""
    cum = np.cumsum(np.asarray(closest, np.float64))
    r = np.asarray(u, np.float32).astype(np.float64) * cum[-1]
    return np.minimum(np.searchsorted(cum, r, side="right"), len(cum) - 1).astype(np.int64)


def pp_pick(X, closest, cands, x2=None):
    """-> winner slot, potentials [trials], new closest [m]."""
    dmin = np.minimum(np.asarray(closest, np.float64)[:, None], sqdist(X, np.asarray(X, np.float64)[cands], x2))
    pots = dmin.sum(0)
    w = int(np.argmin(pots))
    return w, pots, dmin[:, w]


def pp_seed(X, uniforms, K, record=False):
    """Greedy k-means++ on the rows X [m, D] with the draws uniforms [K, trials].  -> dict(chosen [K], centres [K, D], pots [K]) and,
    with `record`, the state before every pick k >= 1: closest vectors, candidate lists and potentials."""
    X = np.asarray(X, np.float64)
    u = np.asarray(uniforms, np.float32)
    m = X.shape[0]
    x2 = (X * X).sum(1)
    c0 = min(int(np.float64(u[0, 0]) * m), m - 1)
    closest = sqdist(X, X[c0:c0 + 1], x2)[:, 0]
    chosen, pots = [c0], [closest.sum()]
    rec = {"closest": [], "cands": [], "pots": []}
    for k in range(1, K):
        cands = pp_candidates(closest, u[k])
        w, p, new_closest = pp_pick(X, closest, cands, x2)
        if record:
            rec["closest"].append(closest.copy())
            rec["cands"].append(cands)
            rec["pots"].append(p)
        closest = new_closest
        chosen.append(int(cands[w]))
        pots.append(p[w])
    out = {"chosen": np.array(chosen), "centres": X[chosen].copy(), "pots": np.array(pots), "closest": closest}
    if record:
        out["record"] = rec
    return out


def assign(X, C, x2=None):
    d = sqdist(X, C, x2)
    lab = d.argmin(1)
    return lab, d[np.arange(len(lab)), lab]


def inertia(X, C, chunk=8192):
    """mean over the rows of the min squared distance"""
    tot = 0.0
    for i in range(0, len(X), chunk):
        tot += assign(X[i:i + chunk], C)[1].sum()
    return tot / len(X)


def minibatch_step(rows, C, counts, labels=None):
    """One step on the gathered rows [B, D]; C [K, D] and counts [K] are updated in place.  `labels` may be supplied (the GPU test passes
    the fp32 assignment of oracle.kmeans_assign); the sums are fp64 either way.  -> batch inertia (mean), squared movement, m_k."""
    rows = np.asarray(rows, np.float64)
    K = C.shape[0]
    if labels is None:
        labels, dmin = assign(rows, C)
    else:
        diff = rows - C[labels]
        dmin = (diff * diff).sum(1)
    order = np.argsort(labels, kind="stable")
    mk = np.bincount(labels, minlength=K).astype(np.float64)
    nz = np.nonzero(mk)[0]
    starts = np.concatenate([[0], np.cumsum(mk[nz]).astype(np.int64)[:-1]])
    sums = np.add.reduceat(rows[order], starts, axis=0)
    counts[nz] += mk[nz]
    new = C[nz] + (sums - mk[nz, None] * C[nz]) / counts[nz, None]
    move = float(((new - C[nz]) ** 2).sum())
    C[nz] = new
    return float(dmin.mean()), move, mk


class StopState:
    """sklearn's _mini_batch_convergence, as csrc/kmeans_fit.hip keeps it on the device."""

    def __init__(self, alpha, tol_abs, max_no_improvement):
        self.alpha, self.tol_abs, self.mni = alpha, tol_abs, int(max_no_improvement or 0)
        self.ewa = self.ewa_min = None
        self.no_improvement = self.step = 0
        self.stopped = 0

    def update(self, batch_inertia, move):
        self.step += 1
        if self.step == 1:
            return 0
        self.ewa = batch_inertia if self.ewa is None else self.ewa * (1.0 - self.alpha) + batch_inertia * self.alpha
        if self.tol_abs > 0 and move <= self.tol_abs:
            self.stopped = 2
            return 2
        if self.ewa_min is None or self.ewa < self.ewa_min:
            self.ewa_min, self.no_improvement = self.ewa, 0
        else:
            self.no_improvement += 1
        if self.mni > 0 and self.no_improvement >= self.mni:
            self.stopped = 1
        return self.stopped


def fit(X, draws, n_clusters, batch_size, max_iter, n_init, max_no_improvement=100, tol=0.0, init="k-means++", **_ignored):
    """The whole fit, steps 1-4 of open_musiclm_amd/kmeans_fit.py, in fp64 with the draws of `draws` (an ArrayDraws)."""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    K = n_clusters
    B = min(batch_size, n)
    init_size = 3 * B
    if init_size < K:
        init_size = 3 * K
    init_size = min(init_size, n)
    trials = 2 + int(math.log(K))

    def subset():
        return X if init_size == n else X[draws.init_rows(n, init_size).numpy()]

    Xv = subset()
    seeds, scores, chosen = [], [], []
    for _ in range(n_init):
        sub = subset()
        if init == "k-means++":
            s = pp_seed(sub, draws.seeding_uniforms(K, trials).numpy(), K)
            c, ch = s["centres"], s["chosen"]
        else:
            ch = draws.random_rows(init_size, K).numpy()
            c = sub[ch].copy()
        seeds.append(c)
        chosen.append(ch)
        scores.append(inertia(Xv, c))
    best = int(np.argmin(scores))
    C = seeds[best].copy()
    init_centres = C.copy()
    counts = np.zeros(K)
    n_steps = (max_iter * n) // B
    stop = StopState(min(1.0, 2.0 * B / (n + 1)), float(X.var(0).mean()) * tol if tol > 0 else 0.0, max_no_improvement)
    step = 0
    while step < n_steps and not stop.stopped:
        idx = draws.batch_indices(step, 1, B, n).numpy()[0]
        bi, mv, _ = minibatch_step(X[idx], C, counts)
        stop.update(bi, mv)
        step += 1
    return {"centres": C, "inertia": inertia(X, C), "n_steps": stop.step, "counts": counts, "best_init": best,
            "init_inertias": np.array(scores), "init_chosen": np.array(chosen), "init_centres": init_centres, "stopped": stop.stopped}


def planted_mixture(n, D, K, scale=3.0, seed=0):
    """n rows of a planted mixture: K Gaussian centres of scale `scale`, unit noise (fp32)."""
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((K, D)) * scale
    return (centres[rng.randint(0, K, n)] + rng.standard_normal((n, D))).astype(np.float32)
