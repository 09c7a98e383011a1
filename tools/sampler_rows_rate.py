"""What per-row sampling parameters cost and buy (profiles/sampler_rows.md), one process, arms alternating:
  1. launch: omlm_sample_rows (arrays for k, temperature and top_p, one value in every row: the same work) against omlm_sample_lp with
     those values as scalars -- nucleus and both log-probabilities on, buffer and counter stream.  The method of
     tools/sampler_top_p_rate.py: batches of BATCH launches captured once and replayed between two device events, median and quartiles
     over NBATCH batches, the table taken REPS times -- the scalar form's own rounds give the spread the row form is judged against;
  2. end to end: generate() at the coarse geometry (dim 1024, depth 6, 8 heads, Q = 3, V1 = 1025, 12 CLAP + 199 semantic ids of prompt),
     STEPS time steps = 3 STEPS ids per row, B = 64 unguided and P = 32 guided: a call with numbers against a call with a distinct
     temperature, filter_thres, top_p (and cond_scale) in every row, whole-call wall time, ids/s = rows * ids / time;
  3. the headline: N = 8 settings as ONE call of 64 rows with per-row values against 8 calls of 8 rows with numbers.
env: PREC (fp16ff), BATCH (20), NBATCH (20), REPS (2), STEPS (750), PARTS ("1,2,3")."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from open_musiclm_amd import open_musiclm as M  # noqa: E402
from open_musiclm_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
prec = os.environ.get("PREC", "fp16ff")
BATCH, NBATCH, REPS = (int(os.environ.get(n, d)) for n, d in (("BATCH", 20), ("NBATCH", 20), ("REPS", 2)))
STEPS = int(os.environ.get("STEPS", 750))
PARTS = os.environ.get("PARTS", "1,2,3").split(",")
g = torch.Generator().manual_seed(0)


def batch(fn):
    def eager():
        for i in range(BATCH):
            fn(i)
    eager()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    return graph.replay


def timed(run):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / BATCH                      # us per launch


def cell(x):
    q = statistics.quantiles(x, n=4)
    return f"{statistics.median(x):.2f} [{q[0]:.2f}, {q[2]:.2f}]"


if "1" in PARTS:
    print(f"## 1. launch, us (median [quartiles] over {NBATCH} replays of {BATCH} captured launches; top_p 0.9, k = V / 10, T = 1, both log-probabilities)")
    for rep in range(REPS):
        for V in (1025, 2049, 8193):
            for B in (1, 64):
                ld = (V + 7) // 8 * 8
                logits = (torch.randn(B, ld, generator=g) * 4).to(dev)
                u = torch.rand(B, V, generator=g).to(dev)
                out = torch.empty(B, dtype=torch.long, device=dev)
                lpm, lps = torch.empty(B, device=dev), torch.empty(B, device=dev)
                k = max(int(0.1 * V), 1)
                rows = dict(row_k=torch.full((B,), k, dtype=torch.int32, device=dev), row_temperature=torch.ones(B, device=dev),
                            row_top_p=torch.full((B,), 0.9, device=dev))
                lp = dict(lp_model=lpm, lp_sampled=lps)
                runs = {
                    "buffer scalar": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=0.9, uniform=u, **lp),
                    "buffer rows": lambda i: ops.sample(logits, out, V, None, None, True, uniform=u, **lp, **rows),
                    "counter scalar": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=0.9, seed=12345, step=i, **lp),
                    "counter rows": lambda i: ops.sample(logits, out, V, None, None, True, seed=12345, step=i, **lp, **rows),
                }
                runs = {n: batch(f) for n, f in runs.items()}
                for _ in range(3):
                    for f in runs.values():
                        timed(f)
                t = {n: [] for n in runs}
                for _ in range(NBATCH):
                    for n, f in runs.items():
                        t[n].append(timed(f))
                med = {n: statistics.median(v) for n, v in t.items()}
                print(f"rep={rep} V={V} B={B}: " + "  ".join(f"{n} {cell(v)}" for n, v in t.items()) +
                      f"  rows - scalar: buffer {med['buffer rows'] - med['buffer scalar']:+.2f} counter {med['counter rows'] - med['counter scalar']:+.2f}",
                      flush=True)

if "2" in PARTS or "3" in PARTS:
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, ff_dropout=0.0, precision=prec).to(dev)
    stage = M.CoarseStage(coarse_transformer=model).eval()

    def prompts(B, b0=0):
        gp = torch.Generator().manual_seed(99)
        clap, sem = torch.randint(0, 1024, (64, 12, 1), generator=gp), torch.randint(0, 1024, (64, 199), generator=gp)
        return dict(clap_token_ids=clap[b0:b0 + B].to(dev), semantic_token_ids=sem[b0:b0 + B].to(dev), use_cache=True, sampler_rng="counter")

    def call(kw, steps=STEPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        stage.generate(max_time_steps=steps, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def spread(B):
        return dict(temperature=[0.5 + r / B for r in range(B)], filter_thres=[0.5 + 0.49 * r / B for r in range(B)],
                    top_p=[0.5 + 0.5 * (r + 1) / B for r in range(B)])

if "2" in PARTS:
    print(f"\n## 2. generate() end to end ({prec}, {3 * STEPS} ids per row, whole call, {REPS + 1} alternating repeats)")
    print("| arm | rows | s: best | median | worst | ids/s (best) |")
    print("|---|---|---|---|---|---|")
    arms = {
        "unguided, numbers": (64, dict(prompts(64), sampler_seed=7, temperature=0.95, filter_thres=0.9, top_p=0.9)),
        "unguided, per row": (64, dict(prompts(64), sampler_seed=7, **spread(64))),
        "guided P = 32, numbers": (32, dict(prompts(32), sampler_seed=7, temperature=0.95, filter_thres=0.9, top_p=0.9, cond_scale=3.0)),
        "guided P = 32, per row": (32, dict(prompts(32), sampler_seed=7, cond_scale=[0.5 + 0.2 * r for r in range(32)], **spread(32))),
    }
    for _, kw in arms.values():
        call(kw, 2)
    ts = {n: [] for n in arms}
    for _ in range(REPS + 1):
        for n, (_, kw) in arms.items():
            ts[n].append(call(kw))
    for n, (rows_, _) in arms.items():
        v = sorted(ts[n])
        print(f"| {n} | {rows_} | {v[0]:.3f} | {v[len(v) // 2]:.3f} | {v[-1]:.3f} | {rows_ * 3 * STEPS / v[0]:.0f} |", flush=True)

if "3" in PARTS:
    print(f"\n## 3. eight settings over 64 prompts ({prec}, {3 * STEPS} ids per row): one call of 64 rows against eight calls of 8 rows")
    settings = [(0.6 + 0.1 * i, 0.9 - 0.05 * i, 1.0 - 0.05 * i) for i in range(8)]          # (temperature, filter_thres, top_p)
    one = dict(prompts(64), sampler_seed=7, temperature=[settings[r // 8][0] for r in range(64)],
               filter_thres=[settings[r // 8][1] for r in range(64)], top_p=[settings[r // 8][2] for r in range(64)])
    eight = [dict(prompts(8, 8 * i), sampler_seed=7 + i, temperature=s[0], filter_thres=s[1], top_p=s[2]) for i, s in enumerate(settings)]
    call(one, 2)
    call(eight[0], 2)
    t1, t8 = [], []
    for _ in range(REPS):
        t1.append(call(one))
        t8.append(sum(call(kw) for kw in eight))
    ids = 64 * 3 * STEPS
    print("| arm | s: best | worst | ids/s (best) |")
    print("|---|---|---|---|")
    print(f"| one call, 64 rows, per-row values | {min(t1):.3f} | {max(t1):.3f} | {ids / min(t1):.0f} |")
    print(f"| eight calls, 8 rows each, numbers | {min(t8):.3f} | {max(t8):.3f} | {ids / min(t8):.0f} |")
    print(f"ratio (eight calls / one call, best times): {min(t8) / min(t1):.2f}")
