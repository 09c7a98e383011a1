"""Launch time of the sampler's buffer and counter entry points (omlm_sample_topk_gumbel / omlm_sample_topk_gumbel_rng), alternating in
one process.  Device events around batches of BATCH back-to-back launches; per shape the median (and quartiles) of the per-launch time
over NBATCH batches of each entry point after a warm-up, the whole table REPS times (the spread between repetitions is the yardstick).
MODE=eager: what a caller that issues launches back to back sees (it includes the host's launch path, about 9 us per launch, which hides
any kernel shorter than that); MODE=graph: the BATCH launches are captured once and each batch is one replay, so the host is out and the
figure is kernel time plus the dispatch gap between dependent kernels.
env: MODE (eager), BATCH (10), NBATCH (40), REPS (3).  k = max(int(0.1 V), 1), T = 1, forbid_last."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import ops

dev = torch.device("cuda:0")
BATCH = int(os.environ.get("BATCH", 10)); NBATCH = int(os.environ.get("NBATCH", 40)); REPS = int(os.environ.get("REPS", 3))
MODE = os.environ.get("MODE", "eager")
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


def quart(x):
    q = statistics.quantiles(x, n=4)
    return statistics.median(x), q[0], q[2]


for rep in range(REPS):
    for V in (1025, 2049, 8193, 65536):
        for B in (1, 16, 64):
            ld = (V + 7) // 8 * 8
            logits = (torch.randn(B, ld, generator=g) * 4).to(dev)
            u = torch.rand(B, V, generator=g).to(dev)
            out = torch.empty(B, dtype=torch.long, device=dev)
            k = max(int(0.1 * V), 1)
            buf = lambda i: ops.sample_topk_gumbel(logits, u, out, V, k, 1.0, True)                     # noqa: E731
            cnt = lambda i: ops.sample_topk_gumbel_rng(logits, 12345, i, 0, out, V, k, 1.0, True)       # noqa: E731
            buf, cnt = batch(buf), batch(cnt)
            for _ in range(3):
                timed(buf), timed(cnt)
            tb, tc = [], []
            for _ in range(NBATCH):
                tb.append(timed(buf))
                tc.append(timed(cnt))
            (mb, b1, b3), (mc, c1, c3) = quart(tb), quart(tc)
            print(f"mode={MODE} rep={rep} V={V} B={B} launches={BATCH * NBATCH}: buffer {mb:.2f} us [{b1:.2f}, {b3:.2f}]  counter {mc:.2f} us [{c1:.2f}, {c3:.2f}]  "
                  f"counter - buffer {mc - mb:+.2f} us", flush=True)
