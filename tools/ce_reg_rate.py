"""What label smoothing and z-loss cost in the training step (profiles/ce_reg.md): the coarse bench step (dim 1024, depth 6, 8 heads, Q = 3,
V1 = 1025, B x 1116 rows, ff_dropout 0.1, the captured micro-step + the fused optimizer step -- bench.py's own configuration, which is not
to change) at (label_smoothing, z_loss) = (0, 0) against (0.1, 1e-4), one process, two models of the same seed, arms alternating.
env: PREC (fp16ff), BATCH (32), REPS (5), STEPS (5 optimizer steps per sample), JSON (unset: nothing is written).  Prints the table."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from open_musiclm_amd import open_musiclm as M  # noqa: E402
from open_musiclm_amd.data import SyntheticTokenDataset  # noqa: E402
from open_musiclm_amd.graph import GraphedForwardBackward  # noqa: E402
from open_musiclm_amd.optimizer import get_optimizer  # noqa: E402

dev = torch.device("cuda:0")
prec, B = os.environ.get("PREC", "fp16ff"), int(os.environ.get("BATCH", 32))
reps, steps = int(os.environ.get("REPS", 5)), int(os.environ.get("STEPS", 5))
keys = ("clap_token_ids", "semantic_token_ids", "coarse_token_ids")
ds = SyntheticTokenDataset("coarse", length=1 << 20, seed=1234)
batches = []
for i in range(4):
    items = [ds[i * B + j] for j in range(B)]
    batches.append([torch.cat([it[f] for it in items], 0).to(dev) for f in range(3)])


class Arm:
    def __init__(self, eps, zeta):
        torch.manual_seed(0)
        self.model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, attn_dropout=0.0, ff_dropout=0.1, num_coarse_quantizers=3,
                                                 precision=prec).to(dev)
        self.stage = M.CoarseStage(coarse_transformer=self.model, cross_entropy_loss_weights=[0., 0., 1.], label_smoothing=eps, z_loss=zeta).train()
        self.optim = get_optimizer(self.model.parameters(), lr=3e-4, wd=0.01)
        self.fb = GraphedForwardBackward(lambda **kw: self.stage(**kw, return_loss=True, return_logits=False)[0])
        self.optim.zero_grad()

        def discard():
            self.optim.mark_grads_dirty()
            self.optim.zero_grad()
        self.fb.prepare(dict(zip(keys, batches[0])), after_warmup=discard)
        assert self.fb.graph is not None, self.fb.capture_error
        self.k = 0

    def run(self, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            self.optim.zero_grad()
            loss = self.fb(**dict(zip(keys, batches[self.k % len(batches)])))
            self.optim.mark_grads_dirty()
            self.optim.step(max_grad_norm=0.5)
            self.k += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n, float(loss)


arms = {(0.0, 0.0): Arm(0.0, 0.0), (0.1, 1e-4): Arm(0.1, 1e-4)}
for a in arms.values():
    a.run(3)
ms = {k: [] for k in arms}
last = {}
for _ in range(reps):
    for k, a in arms.items():
        t, last[k] = a.run(steps)
        ms[k].append(t)
print(f"## coarse training step ({prec}, B = {B}, captured micro-step + optimizer step, {reps} alternating samples of {steps} steps), ms per step")
print("| (label_smoothing, z_loss) | best | median | worst | samples/s (best) | last loss |")
print("|---|---|---|---|---|---|")
for k, v in ms.items():
    v = sorted(v)
    print(f"| {k} | {v[0]:.2f} | {v[len(v) // 2]:.2f} | {v[-1]:.2f} | {B * 1e3 / v[0]:.1f} | {last[k]:.4f} |")
if os.environ.get("JSON"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["JSON"])), exist_ok=True)
    json.dump({"precision": prec, "batch": B, "ms": {str(k): v for k, v in ms.items()}}, open(os.environ["JSON"], "w"), indent=1)
