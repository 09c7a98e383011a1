"""Launch time of the sampler with and without the log-probabilities of the sampled id (omlm_sample_lp against omlm_sample), buffer and
counter stream, with and without a nucleus, alternating in one process: the method of tools/sampler_top_p_rate.py.  Per shape and top_p
four callables -- ops.sample on the buffer and on the stream, and the same two with lp_model= and lp_sampled= -- take turns, one batch of
BATCH back-to-back launches each between two device events; the figure is the median (and quartiles) of the per-launch time over NBATCH
batches after a warm-up, and the whole table is taken REPS times.  MODE=graph (default): each batch is captured once and replayed, so the
host's launch path is out; MODE=eager: what a caller that issues launches sees.
env: MODE (graph), BATCH (20), NBATCH (20), REPS (2), PS (1,0.9), BS (1,64), VS (1025,2049,8193,65536).  k = max(int(0.1 V), 1), T = 1,
forbid_last, N(0, 16) logits."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import ops

dev = torch.device("cuda:0")
BATCH = int(os.environ.get("BATCH", 20)); NBATCH = int(os.environ.get("NBATCH", 20)); REPS = int(os.environ.get("REPS", 2))
MODE = os.environ.get("MODE", "graph")
PS = [float(p) for p in os.environ.get("PS", "1,0.9").split(",")]
BS = [int(b) for b in os.environ.get("BS", "1,64").split(",")]
VS = [int(v) for v in os.environ.get("VS", "1025,2049,8193,65536").split(",")]
g = torch.Generator().manual_seed(0)


def batch(fn):
    """The BATCH launches as a callable: eager, or one replay of their capture."""
    def eager():
        for i in range(BATCH):
            fn(i)
    if MODE != "graph":
        return eager
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


for rep in range(REPS):
    for V in VS:
        for B in BS:
            for p in PS:
                ld = (V + 7) // 8 * 8
                logits = (torch.randn(B, ld, generator=g) * 4).to(dev)
                u = torch.rand(B, V, generator=g).to(dev)
                out = torch.empty(B, dtype=torch.long, device=dev)
                pm, ps = torch.empty(B, device=dev), torch.empty(B, device=dev)
                k = max(int(0.1 * V), 1)
                tp = None if p >= 1 else p
                runs = {
                    "buffer": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=tp, uniform=u),
                    "buffer+lp": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=tp, uniform=u, lp_model=pm, lp_sampled=ps),
                    "counter": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=tp, seed=12345, step=i),
                    "counter+lp": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=tp, seed=12345, step=i, lp_model=pm, lp_sampled=ps),
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
                print(f"mode={MODE} rep={rep} top_p={p} V={V} B={B} launches={BATCH * NBATCH} us: " + "  ".join(f"{n} {cell(v)}" for n, v in t.items()) +
                      f"  added buffer {med['buffer+lp'] - med['buffer']:.2f} counter {med['counter+lp'] - med['counter']:.2f}", flush=True)
