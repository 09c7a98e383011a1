"""What classifier-free guidance costs (profiles/sampler_guidance.md), at the coarse geometry (dim 1024, depth 6, 8 heads, Q = 3, V1 = 1025,
12 CLAP + 199 semantic ids of prompt), one process, arms alternating:
  1. decode: per-id time of the KV-cached sampling loop (prefill differenced out: two generate calls of different lengths) for a guided
     call of P prompts against (a) an unguided call of P samples -- what the user pays -- and (b) an unguided call of 2P samples -- the
     same step work, so the difference is the two added launches;
  2. the two new kernels alone: N launches captured into one graph and replayed, device-event time over N -- the kernel and the queue's
     gap to the next one, without the host's launch cost (eager back-to-back launches from Python measure the host: 11 - 13 us each);
  3. the coarse training micro-step (forward + backward on the one-launch batch preparation) at null_cond_prob 0 against 0.15.
env: PREC (fp16ff), REPS (5), PS ("1,8,32"), SCALE (3.0), JSON (unset: nothing is written; a path: every sample of the run as JSON).  Prints the tables."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from open_musiclm_amd import open_musiclm as M  # noqa: E402
from open_musiclm_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
prec, reps = os.environ.get("PREC", "fp16ff"), int(os.environ.get("REPS", 5))
PS = [int(p) for p in os.environ.get("PS", "1,8,32").split(",")]
scale = float(os.environ.get("SCALE", 3.0))
torch.manual_seed(0)
model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, ff_dropout=0.0, precision=prec).to(dev)
stage = M.CoarseStage(coarse_transformer=model).eval()
short, long_ = 8, 72
result = {"precision": prec, "reps": reps, "scale": scale, "decode": {}, "kernels": {}, "train": {}}


def prompts(B):
    g = torch.Generator().manual_seed(99)
    return dict(clap_token_ids=torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev),
                semantic_token_ids=torch.randint(0, 1024, (B, 199), generator=g).to(dev), use_cache=True, sampler_rng="counter", sampler_seed=7)


def call(n, kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    stage.generate(max_time_steps=n, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t


print(f"## decode ({prec}, cond_scale {scale}, {reps} alternating repeats, us per id step = (t[{long_} time steps] - t[{short}]) / {(long_ - short) * 3} ids)")
print("| P | arm | us / step: best | median | worst | ids/s (best) |")
print("|---|---|---|---|---|---|")
for P in PS:
    arms = {"guided P": (P, dict(prompts(P), cond_scale=scale)), "unguided P": (P, prompts(P)), "unguided 2P": (2 * P, prompts(2 * P))}
    for _, kw in arms.values():
        call(2, kw)                                                    # every shape of the timed window has run once
    us = {name: [] for name in arms}
    for _ in range(reps):
        for name, (_, kw) in arms.items():
            ts, tl = call(short, kw), call(long_, kw)
            us[name].append(1e6 * (tl - ts) / ((long_ - short) * 3))
    result["decode"][P] = {}
    for name, (ids_per_step, _) in arms.items():
        v = sorted(us[name])
        result["decode"][P][name] = dict(us_per_step=v, ids_per_step=ids_per_step, ids_per_s_best=ids_per_step * 1e6 / v[0])
        print(f"| {P} | {name} | {v[0]:.1f} | {v[len(v) // 2]:.1f} | {v[-1]:.1f} | {ids_per_step * 1e6 / v[0]:.0f} |")

print("\n## the two kernels alone (N = 500 launches captured in one graph, device events around 4 replays, us per launch)")
print("| P | omlm_guide_logits [P, 1025] ld 1032 | omlm_decode_twin P ids + [P, 1024] |")
print("|---|---|---|")
N = 500
for P in PS:
    lg = torch.randn(2 * P, 1032, device=dev)
    out = torch.empty(P, 1032, device=dev)
    ids = torch.zeros(2 * P, dtype=torch.long, device=dev)
    x = torch.randn(2 * P, 1024, device=dev)
    row = {}
    lc, ln, ic, it, xc, xt = lg[:P], lg[P:], ids[:P], ids[P:], x[:P], x[P:]
    for name, fn in (("guide", lambda: ops.guide_logits(lc, ln, out, 1025, scale)), ("twin", lambda: ops.decode_twin(ic, it, xc, xt))):
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(N):
                fn()
        graph.replay()
        best = None
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            t = 1e3 * a.elapsed_time(b) / (4 * N)
            best = t if best is None else min(best, t)
        row[name] = best
    result["kernels"][P] = row
    print(f"| {P} | {row['guide']:.2f} | {row['twin']:.2f} |")

print("\n## coarse training micro-step (forward + backward, B = 4, N = 1116 rows, one-launch batch preparation), ms")
B, n_coarse = 4, 300
g = torch.Generator().manual_seed(5)
batch = [torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev), torch.randint(0, 1024, (B, 199), generator=g).to(dev),
         torch.randint(0, 1024, (B, n_coarse, 3), generator=g).to(dev)]
wrappers = {p: M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.],
                                                    mask_prob=0.15, null_cond_prob=p).train() for p in (0., 0.15)}


def micro(w, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        model.zero_grad(set_to_none=True)
        w(all_token_ids=batch, return_loss=True, return_logits=False)[0].backward()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n


for w in wrappers.values():
    micro(w, 3)
ms = {p: [] for p in wrappers}
for _ in range(reps):
    for p, w in wrappers.items():
        ms[p].append(micro(w, 10))
print("| null_cond_prob | best | median | worst |")
print("|---|---|---|---|")
for p, v in ms.items():
    v = sorted(v)
    result["train"][p] = v
    print(f"| {p} | {v[0]:.2f} | {v[len(v) // 2]:.2f} | {v[-1]:.2f} |")
model.eval()
if os.environ.get("JSON"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["JSON"])), exist_ok=True)
    json.dump(result, open(os.environ["JSON"], "w"), indent=1)
