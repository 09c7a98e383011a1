"""Launch time of the sampler with and without the nucleus (top-p), buffer and counter stream, alternating in one process: the method of
tools/sampler_stream_rate.py.  Per shape four callables -- omlm_sample_topk_gumbel / omlm_sample_topk_gumbel_rng (the parent's launches:
the yardstick, measured in this same run) and omlm_sample with top_p = TOP_P on the buffer and on the stream -- take turns, one batch of BATCH
back-to-back launches each between two device events; the figure is the median (and quartiles) of the per-launch time over NBATCH batches
after a warm-up, and the whole table is taken REPS times.  MODE=graph (default): each batch is captured once and replayed, so the host's
launch path (about 9 us, which hides every kernel shorter than that) is out; MODE=eager: what a caller that issues launches sees.
env: MODE (graph), BATCH (20), NBATCH (20), REPS (2), TOP_P (0.9), BS (1,16,64).  k = max(int(0.1 V), 1), T = 1, forbid_last, N(0, 16) logits."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import ops

dev = torch.device("cuda:0")
BATCH = int(os.environ.get("BATCH", 20)); NBATCH = int(os.environ.get("NBATCH", 20)); REPS = int(os.environ.get("REPS", 2))
MODE = os.environ.get("MODE", "graph"); TOP_P = float(os.environ.get("TOP_P", 0.9))
BS = [int(b) for b in os.environ.get("BS", "1,16,64").split(",")]
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
    for V in (1025, 2049, 8193, 65536):
        for B in BS:
            ld = (V + 7) // 8 * 8
            logits = (torch.randn(B, ld, generator=g) * 4).to(dev)
            u = torch.rand(B, V, generator=g).to(dev)
            out = torch.empty(B, dtype=torch.long, device=dev)
            k = max(int(0.1 * V), 1)
            runs = {
                "buffer": lambda i: ops.sample_topk_gumbel(logits, u, out, V, k, 1.0, True),
                "buffer+p": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=TOP_P, uniform=u),
                "counter": lambda i: ops.sample_topk_gumbel_rng(logits, 12345, i, 0, out, V, k, 1.0, True),
                "counter+p": lambda i: ops.sample(logits, out, V, k, 1.0, True, top_p=TOP_P, seed=12345, step=i),
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
            print(f"mode={MODE} rep={rep} top_p={TOP_P} V={V} B={B} launches={BATCH * NBATCH} us: " + "  ".join(f"{n} {cell(v)}" for n, v in t.items()) +
                  f"  ratio buffer {med['buffer+p'] / med['buffer']:.2f} counter {med['counter+p'] / med['counter']:.2f}", flush=True)
