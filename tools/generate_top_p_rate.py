"""Per-step time of the KV-cached sampling loop with and without the nucleus (top_p = TOP_P against None), alternating in one process:
the set-up and the differencing of tools/decode_rate.py (coarse stage dim 1024, depth 6, 8 heads; two `generate` calls of 10 and 110 time
steps x 3 quantizers, (t_long - t_short) / extra ids, so the prefill is out).  Per B the best of REPS pairs for each setting, and every pair.
env: BS (1,16,64), PREC (fp16ff), REPS (3), TOP_P (0.9), SAMPLER_RNG (unset: generate()'s default)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import open_musiclm as M

dev = torch.device("cuda:0")
prec = os.environ.get("PREC", "fp16ff"); reps = int(os.environ.get("REPS", 3)); TOP_P = float(os.environ.get("TOP_P", 0.9))
BS = [int(b) for b in os.environ.get("BS", "1,16,64").split(",")]
torch.manual_seed(0)
model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, precision=prec).to(dev)
stage = M.CoarseStage(coarse_transformer=model).eval()
short, long_ = 10, 110

for B in BS:
    g = torch.Generator().manual_seed(99)
    kw = dict(clap_token_ids=torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev),
              semantic_token_ids=torch.randint(0, 1024, (B, 199), generator=g).to(dev), use_cache=True)
    if os.environ.get("SAMPLER_RNG"):
        kw["sampler_rng"] = os.environ["SAMPLER_RNG"]

    def run(n, top_p):
        torch.cuda.synchronize(); t = time.perf_counter()
        stage.generate(max_time_steps=n, top_p=top_p, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    for p in (None, TOP_P):
        run(2, p)
    us = {None: [], TOP_P: []}
    for _ in range(reps):
        for p in (None, TOP_P):
            ts, tl = run(short, p), run(long_, p)
            us[p].append(1e6 * (tl - ts) / ((long_ - short) * 3))
    for p in (None, TOP_P):
        best = min(us[p])
        print(f"B={B} {prec} top_p={p} sampler_rng={os.environ.get('SAMPLER_RNG', 'default')}: {best:.1f} us/step -> {B * 1e6 / best:.0f} ids/s "
              f"(all {', '.join(f'{v:.1f}' for v in us[p])})", flush=True)
