"""What the per-quantizer metrics cost (profiles/ce_metrics.md).
1. The two launches of csrc/ce_metrics.hip and the existing omlm_cross_entropy_fwd on the same buffers in the same process: R = 32 x 901
   rows (the coarse bench step's predicted sequence), V1 = 1025 / 2049 / 8193, device events around ITERS back-to-back launches.
2. The coarse training step (dim 1024, depth 6, 8 heads, Q = 3, V1 = 1025, ff_dropout 0.1, the captured micro-step + the fused optimizer
   step -- bench.py's configuration) without and with the metrics buffer, one process, two models of the same seed, arms alternating.
env: PREC (fp16ff), BATCH (32), REPS (5), STEPS (5), ITERS (50), STEP (1; 0 skips part 2), JSON (unset: nothing is written)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from open_musiclm_amd import open_musiclm as M  # noqa: E402
from open_musiclm_amd import ops  # noqa: E402
from open_musiclm_amd.data import SyntheticTokenDataset  # noqa: E402
from open_musiclm_amd.graph import GraphedForwardBackward  # noqa: E402
from open_musiclm_amd.optimizer import get_optimizer  # noqa: E402

dev = torch.device("cuda:0")
prec, B = os.environ.get("PREC", "fp16ff"), int(os.environ.get("BATCH", 32))
reps, steps, iters = int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 5)), int(os.environ.get("ITERS", 50))
result = {"precision": prec, "batch": B, "kernels": {}, "step_ms": {}}


def timed(fn):
    """us per call: device events around `iters` launches, best and median of 5 windows after a warm-up"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / iters)
    out.sort()
    return out[0], out[2]


n, Q = 901, 3
R = 32 * n
print(f"## the launches alone, R = {R} rows, {iters} launches per window (us per launch: best / median of 5 windows)")
print("| V1 | logits MB | omlm_cross_entropy_fwd | omlm_ce_metrics | omlm_ce_metrics_bins | metrics GB/s (best) |")
print("|---|---|---|---|---|---|")
for V1 in (1025, 2049, 8193):
    ld = (V1 + 7) // 8 * 8
    g = torch.Generator(device=dev).manual_seed(V1)
    logits = torch.randn(R, ld, device=dev, generator=g)
    labels = torch.randint(0, V1, (R,), device=dev, generator=g, dtype=torch.int32)
    lse, nll_sum = torch.empty(R, device=dev), torch.zeros(1, device=dev)
    nll, rank, ent = torch.empty(R, device=dev), torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, device=dev)
    bins = torch.zeros(Q + 1, 5, dtype=torch.float64, device=dev)
    k = ops.default_metrics_top_k(V1)
    t_fwd = timed(lambda: ops.ce_fwd(logits, labels, lse, nll_sum, V1))
    t_row = timed(lambda: ops.ce_metrics(logits, labels, V1, row_nll=nll, row_rank=rank, row_entropy=ent))
    t_bin = timed(lambda: ops.ce_metrics_bins(nll, rank, ent, labels, n, Q, V1, k, bins))
    mb = R * V1 * 4 / 1e6
    print(f"| {V1} | {mb:.0f} | {t_fwd[0]:.1f} / {t_fwd[1]:.1f} | {t_row[0]:.1f} / {t_row[1]:.1f} | {t_bin[0]:.1f} / {t_bin[1]:.1f} | {mb / 1e3 / (t_row[0] * 1e-6):.0f} |")
    result["kernels"][V1] = dict(ce_fwd_us=t_fwd, ce_metrics_us=t_row, ce_metrics_bins_us=t_bin)
    del logits

if os.environ.get("STEP", "1") != "0":
    keys = ("clap_token_ids", "semantic_token_ids", "coarse_token_ids")
    ds = SyntheticTokenDataset("coarse", length=1 << 20, seed=1234)
    batches = []
    for i in range(4):
        items = [ds[i * B + j] for j in range(B)]
        batches.append([torch.cat([it[f] for it in items], 0).to(dev) for f in range(3)])

    class Arm:
        def __init__(self, with_metrics):
            torch.manual_seed(0)
            self.model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, attn_dropout=0.0, ff_dropout=0.1, num_coarse_quantizers=3,
                                                     precision=prec).to(dev)
            self.stage = M.CoarseStage(coarse_transformer=self.model, cross_entropy_loss_weights=[0., 0., 1.]).train()
            self.metrics = self.stage.transformer_wrapper.new_metrics() if with_metrics else None
            mkw = dict(return_metrics=self.metrics) if with_metrics else {}
            self.optim = get_optimizer(self.model.parameters(), lr=3e-4, wd=0.01)
            self.fb = GraphedForwardBackward(lambda **kw: self.stage(**kw, return_loss=True, return_logits=False, **mkw)[0])
            self.optim.zero_grad()

            def discard():
                self.optim.mark_grads_dirty()
                self.optim.zero_grad()
            self.fb.prepare(dict(zip(keys, batches[0])), after_warmup=discard)
            assert self.fb.graph is not None, self.fb.capture_error
            self.k = 0

        def run(self, count):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(count):
                self.optim.zero_grad()
                loss = self.fb(**dict(zip(keys, batches[self.k % len(batches)])))
                self.optim.mark_grads_dirty()
                self.optim.step(max_grad_norm=0.5)
                self.k += 1
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t) / count, float(loss)

    arms = {"without": Arm(False), "with quantizer metrics": Arm(True)}
    for a in arms.values():
        a.run(3)
    ms = {k: [] for k in arms}
    last = {}
    for _ in range(reps):
        for k, a in arms.items():
            t, last[k] = a.run(steps)
            ms[k].append(t)
    print(f"\n## coarse training step ({prec}, B = {B}, captured micro-step + optimizer step, {reps} alternating samples of {steps} steps), ms per step")
    print("| arm | best | median | worst | samples/s (best) | last loss |")
    print("|---|---|---|---|---|---|")
    for k, v in ms.items():
        v = sorted(v)
        print(f"| {k} | {v[0]:.2f} | {v[len(v) // 2]:.2f} | {v[-1]:.2f} | {B * 1e3 / v[0]:.1f} | {last[k]:.4f} |")
    d = arms["with quantizer metrics"].metrics.to_dict("train_")
    print("\nper-quantizer means of the last arm's accumulated steps: " +
          ", ".join(f"{k} {d[k]:.4f}" for k in sorted(d) if k.startswith("train_loss_") or k.startswith("train_entropy_")))
    result["step_ms"] = ms
if os.environ.get("JSON"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["JSON"])), exist_ok=True)
    json.dump(result, open(os.environ["JSON"], "w"), indent=1)
