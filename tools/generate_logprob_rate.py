"""Per-step time of the KV-cached sampling loop with and without return_logprobs, alternating in one process: the set-up and the
differencing of tools/generate_top_p_rate.py (coarse stage dim 1024, depth 6, 8 heads, V1 = 1025; two `generate` calls of 10 and 110 time
steps x 3 quantizers, (t_long - t_short) / extra ids, so the prefill is out).  Per B the best of REPS pairs for each setting, and every pair.
LOGPROBS=0 measures the call without the flag alone and never names it: that form also runs on a tree from before the flag, which is how
the unflagged call is compared with its parent (PYTHONPATH pointing at that tree, same process set-up, same machine).
env: BS (1,64), PREC (fp16ff), REPS (3), TOP_P (unset: none), LOGPROBS (1), OMLM_TREE (unset: this tree; else the root to import from)."""
import os, sys, time
sys.path.insert(0, os.environ.get("OMLM_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import open_musiclm as M

dev = torch.device("cuda:0")
prec = os.environ.get("PREC", "fp16ff"); reps = int(os.environ.get("REPS", 3))
TOP_P = float(os.environ["TOP_P"]) if os.environ.get("TOP_P") else None
FLAGS = (False, True) if os.environ.get("LOGPROBS", "1") != "0" else (False,)
BS = [int(b) for b in os.environ.get("BS", "1,64").split(",")]
torch.manual_seed(0)
model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, precision=prec).to(dev)
stage = M.CoarseStage(coarse_transformer=model).eval()
short, long_ = 10, 110
print(f"tree {os.path.dirname(os.path.dirname(os.path.abspath(M.__file__)))}", flush=True)

for B in BS:
    g = torch.Generator().manual_seed(99)
    kw = dict(clap_token_ids=torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev),
              semantic_token_ids=torch.randint(0, 1024, (B, 199), generator=g).to(dev), use_cache=True)
    if TOP_P is not None:
        kw["top_p"] = TOP_P

    def run(n, flag):
        extra = dict(return_logprobs=True) if flag else {}
        torch.cuda.synchronize(); t = time.perf_counter()
        stage.generate(max_time_steps=n, **extra, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for f in FLAGS:
        run(2, f)
    us = {f: [] for f in FLAGS}
    for _ in range(reps):
        for f in FLAGS:
            ts, tl = run(short, f), run(long_, f)
            us[f].append(1e6 * (tl - ts) / ((long_ - short) * 3))
    for f in FLAGS:
        best = min(us[f])
        print(f"B={B} {prec} top_p={TOP_P} return_logprobs={f}: {best:.1f} us/step -> {B * 1e6 / best:.0f} ids/s "
              f"(all {', '.join(f'{v:.1f}' for v in us[f])})", flush=True)
