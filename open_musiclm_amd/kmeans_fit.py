"""MiniBatchKMeans fitted on the device (csrc/kmeans_fit.hip): what `learn_kmeans(..., device='cuda')` runs instead of sklearn on the host.

The rules are the published ones of sklearn's MiniBatchKMeans (the reference's estimator, hf_hubert_kmeans.py:95-118); the random stream
is this module's own, so the centres are not sklearn's (the default, `device=None`, keeps sklearn and its bit-exact golden test).

1. Seeding.  `n_init` times: `init_size = 3 * batch_size` rows (`3 * K` where that is below K; all rows where n is smaller) drawn with
   replacement, greedy k-means++ on them with `2 + floor(ln K)` trials per pick (`omlm_kmeans_pp_seed`: one C call queues the K picks,
   no host round trip).  Every seeding is scored by its inertia on ONE validation draw of `init_size` rows; the lowest wins (ties: first).
2. Mini-batch loop.  `(max_iter * n) // batch_size` steps; each draws `batch_size` row indices with replacement and runs
   `omlm_kmeans_minibatch_step` (assign in the arithmetic of `omlm_nearest_centroid`, running-mean update).
3. Stopping.  sklearn's two rules live in the kernel's device state; a step that finds the stop flag set changes nothing.  The host
   queues `CHECK_EVERY` = 16 steps and then looks at the flag once, so the loop pays one synchronisation per 16 steps and the result
   does not depend on that number (`n_steps_` is the step at which the rule fired).
4. `inertia_`: mean squared distance of ALL rows to their centre (`omlm_kmeans_inertia`, fp64 accumulator).

Draws come from `draw_source` (test hook, like `ResidualVQCodebooks.init_pick_source`): an object with
`init_rows(n, m) -> int64 [m]`, `seeding_uniforms(K, trials) -> float32 [K, trials] in [0, 1)`, `random_rows(m, K) -> int64 [K]` and
`batch_indices(step0, nsteps, B, n) -> int64 [nsteps, B]`, called in this order: the validation rows, then per seeding its rows and its
uniforms (or `random_rows` for `init='random'`), then the batches in chunks of 16 steps.  Default: a `torch.Generator` on the device
seeded with `seed`; the global RNGs are not touched."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip, ops

CHECK_EVERY = 16


class TorchDraws:
    """The default draw source: one device generator seeded with `seed`."""

    def __init__(self, seed: int, device: torch.device):
        self.device = device
        self.g = torch.Generator(device=device)
        self.g.manual_seed(int(seed))

    def init_rows(self, n, m):
        return torch.randint(0, n, (m,), generator=self.g, device=self.device)

    def seeding_uniforms(self, K, trials):
        return torch.rand(K, trials, generator=self.g, device=self.device, dtype=torch.float32)

    def random_rows(self, m, K):
        return torch.randperm(m, generator=self.g, device=self.device)[:K]

    def batch_indices(self, step0, nsteps, B, n):
        return torch.randint(0, n, (nsteps, B), generator=self.g, device=self.device)


def check_fit_arguments(init, reassignment_ratio):
    """The parts of MiniBatchKMeans the device fit does not implement raise, naming the argument."""
    if not (isinstance(init, str) and init in ("k-means++", "random")):
        shown = init if isinstance(init, str) else type(init).__name__
        raise NotImplementedError(f"init={shown!r}: the device k-means fit implements init='k-means++' and init='random'")
    if reassignment_ratio != 0.0:
        raise NotImplementedError(f"reassignment_ratio={reassignment_ratio!r}: the device k-means fit implements reassignment_ratio=0.0 "
                                  "(what the reference passes)")


def require_cuda_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"open_musiclm_amd: the k-means fit was asked to run on {dev}; it only runs on an MI355X through "
                           "libomlm_hip.so (no CPU fallback). Pass device='cuda', or device=None for sklearn on the host.")
    return dev


class GpuMiniBatchKMeans:
    def __init__(self, n_clusters=1024, init="k-means++", max_iter=100, batch_size=10000, tol=0.0, max_no_improvement=100, n_init=20,
                 reassignment_ratio=0.0, seed=0, device="cuda", verbose=0):
        check_fit_arguments(init, reassignment_ratio)
        self.device = require_cuda_device(device)
        self.n_clusters, self.init, self.max_iter, self.batch_size = int(n_clusters), init, int(max_iter), int(batch_size)
        self.tol, self.max_no_improvement, self.n_init = float(tol), max_no_improvement, int(n_init)
        self.reassignment_ratio, self.seed, self.verbose = reassignment_ratio, int(seed), verbose
        self.draw_source = None                  # test hook (module docstring); None: TorchDraws(seed, device)
        self.record_times = False                # tools/kmeans_fit_probe.py: HIP events around the three phases -> times_ms_
        self._cT = None

    # ---- helpers ------------------------------------------------------------------------------------------------------------
    def _rows(self, x, what="feat") -> torch.Tensor:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        hip.require_gpu(x, what)
        if x.dtype != torch.float32 or x.dim() != 2:
            raise ValueError(f"{what} must be [n, D] fp32, got {tuple(x.shape)} {x.dtype}")
        return x.contiguous()

    def _centres_T(self) -> torch.Tensor:
        if self._cT is None:
            c = torch.from_numpy(self.cluster_centers_).to(self.device)
            self._cT = c.t().contiguous()
        return self._cT

    # ---- fit ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def fit(self, feat):
        dev = self.device
        with torch.cuda.device(dev):
            return self._fit(self._rows(feat))

    def _fit(self, x):
        dev = self.device
        n, D = x.shape
        K = self.n_clusters
        if n < K:
            raise ValueError(f"n_samples={n} should be >= n_clusters={K}")
        B = min(self.batch_size, n)
        init_size = 3 * B
        if init_size < K:
            init_size = 3 * K
        init_size = min(init_size, n)
        trials = 2 + int(math.log(K))
        draws = self.draw_source if self.draw_source is not None else TorchDraws(self.seed, dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.record_times else None

        def subset():
            if init_size == n:
                return x
            return x.index_select(0, draws.init_rows(n, init_size).to(dev))

        if ev:
            ev[0].record()
        # 1. seedings, each scored on the one validation draw
        xv = subset()
        m = init_size
        cand_c = torch.empty(self.n_init, K, D, device=dev)
        cand_cT = torch.empty(self.n_init, D, K, device=dev)
        chosen = torch.zeros(self.n_init, K, dtype=torch.int32, device=dev)
        pots = torch.zeros(self.n_init, K, dtype=torch.float64, device=dev)
        init_inertia = torch.zeros(self.n_init, dtype=torch.float64, device=dev)
        closest = torch.empty(m, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.kmeans_pp_workspace_bytes(m, trials) // 4 + 4, dtype=torch.float32, device=dev)
        for j in range(self.n_init):
            sub = subset()
            if self.init == "k-means++":
                u = draws.seeding_uniforms(K, trials).to(device=dev, dtype=torch.float32).contiguous()
                ops.kmeans_pp_seed(sub, closest, u, counter, cand_c[j], cand_cT[j], chosen[j], pots[j], ws, K, trials)
            else:
                pick = draws.random_rows(m, K).to(dev)
                chosen[j].copy_(pick)
                cand_c[j].copy_(sub.index_select(0, pick))
                cand_cT[j].copy_(cand_c[j].t())
            ops.kmeans_inertia(xv, cand_cT[j], init_inertia[j:j + 1])
            del sub
        best = int(torch.argmin(init_inertia))                      # first minimum; the one host look of the seeding phase
        self.best_init_ = best
        self.init_inertias_ = (init_inertia / m).cpu().numpy()
        self.init_chosen_ = chosen.cpu().numpy()
        self.init_centers_ = cand_c[best].cpu().numpy()
        centres = cand_c[best].clone()
        centres_T = cand_cT[best].clone()
        del cand_c, cand_cT, xv, ws
        if ev:
            ev[1].record()

        # 2. + 3. mini-batch loop, stopping rules on the device
        n_steps = (self.max_iter * n) // B
        alpha = min(1.0, 2.0 * B / (n + 1))
        tol_abs = float(x.var(dim=0, unbiased=False).mean()) * self.tol if self.tol > 0 else 0.0
        mni = int(self.max_no_improvement) if self.max_no_improvement is not None else 0
        state = torch.zeros(8, dtype=torch.float64, device=dev)
        counts = torch.zeros(K, device=dev)
        bcounts = torch.zeros(K, device=dev)
        sums = torch.zeros(K, D, device=dev)
        rowmin = torch.empty(B, device=dev)
        move_partial = torch.zeros(K, dtype=torch.float64, device=dev)
        step = 0
        while step < n_steps:
            c = min(CHECK_EVERY, n_steps - step)
            idx = draws.batch_indices(step, c, B, n).to(device=dev, dtype=torch.int32).contiguous()
            for s in range(c):
                ops.kmeans_minibatch_step(x, idx[s], centres, centres_T, counts, bcounts, sums, rowmin, move_partial, state, alpha, tol_abs,
                                          mni)
            step += c
            if float(state[6]) != 0.0:
                break
        st = state.cpu().numpy()
        self.n_steps_ = int(st[4])
        self.n_iter_ = int(math.ceil(self.n_steps_ * B / n))
        self.stop_reason_ = {0: "max_iter", 1: "max_no_improvement", 2: "tol"}[int(st[6])]
        self.ewa_inertia_ = float(st[0])
        if ev:
            ev[2].record()

        # 4. inertia over all rows
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        ops.kmeans_inertia(x, centres_T, total)
        self.inertia_ = float(total) / n
        if ev:
            ev[3].record()
            torch.cuda.synchronize(dev)
            self.times_ms_ = {"seeding": ev[0].elapsed_time(ev[1]), "loop": ev[1].elapsed_time(ev[2]), "inertia": ev[2].elapsed_time(ev[3])}
        self.cluster_centers_ = centres.cpu().numpy()
        self.counts_ = counts.cpu().numpy()
        self.n_features_in_ = D
        self._cT = centres_T
        if self.verbose:
            print(f"kmeans fit on {dev}: {self.n_steps_} / {n_steps} steps ({self.stop_reason_}), inertia {self.inertia_:.5f}")
        return self

    # ---- sklearn's read side ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, x):
        """Nearest centre of every row, through ops.nearest_centroid (the arithmetic of KmeansAssigner.predict).  numpy in -> numpy int64
        out; a CUDA tensor in -> an int64 tensor on its device."""
        as_numpy = isinstance(x, np.ndarray)
        with torch.cuda.device(self.device):
            xt = self._rows(x, "x")
            cT = self._centres_T()
            idx = torch.empty(xt.shape[0], 1, dtype=torch.int32, device=xt.device)
            ops.nearest_centroid(xt, cT, idx, xt.shape[0], xt.shape[1], cT.shape[1])
        out = idx[:, 0].long()
        return out.cpu().numpy() if as_numpy else out

    @torch.no_grad()
    def score(self, x) -> float:
        """sklearn's meaning: minus the SUM of squared distances of the rows to their nearest centre."""
        with torch.cuda.device(self.device):
            xt = self._rows(x, "x")
            total = torch.zeros(1, dtype=torch.float64, device=xt.device)
            ops.kmeans_inertia(xt, self._centres_T(), total)
            return -float(total)

    def fitted(self):
        """Plain host data for joblib (hf_hubert_kmeans.FittedKmeans): what get_hubert_kmeans / HfHubertWithKmeans read."""
        from .hf_hubert_kmeans import FittedKmeans
        return FittedKmeans(self.cluster_centers_, self.inertia_, self.n_steps_, self.counts_, seed=self.seed,
                            params=dict(n_clusters=self.n_clusters, init=self.init, max_iter=self.max_iter, batch_size=self.batch_size,
                                        tol=self.tol, max_no_improvement=self.max_no_improvement, n_init=self.n_init,
                                        reassignment_ratio=self.reassignment_ratio))
