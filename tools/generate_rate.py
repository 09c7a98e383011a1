"""ids/s and peak allocated bytes of CoarseStage.generate (dim 1024, depth 6, 8 heads, 3 coarse quantizers) on the two uniform sources,
alternating in one process.  env: B (64), CODEBOOK (1024: V1 = 1025), STEPS (750 time steps x 3 quantizers = 2250 ids), PREC (fp16ff),
REPS (2).  The peak statistics are reset before each call; the time is a host clock around device synchronises (prefill included)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import open_musiclm as M

dev = torch.device("cuda:0")
B = int(os.environ.get("B", 64)); C = int(os.environ.get("CODEBOOK", 1024)); steps = int(os.environ.get("STEPS", 750))
prec = os.environ.get("PREC", "fp16ff"); reps = int(os.environ.get("REPS", 2))
torch.manual_seed(0)
model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, acoustic_codebook_size=C, precision=prec).to(dev)
stage = M.CoarseStage(coarse_transformer=model).eval()
g = torch.Generator().manual_seed(99)
kw = dict(clap_token_ids=torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev),
          semantic_token_ids=torch.randint(0, 1024, (B, 199), generator=g).to(dev), use_cache=True)
stage.generate(max_time_steps=2, sampler_rng="buffer", **kw)
stage.generate(max_time_steps=2, sampler_rng="counter", **kw)
for rep in range(reps):
    for rng in ("buffer", "counter"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        ids = stage.generate(max_time_steps=steps, sampler_rng=rng, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        n = ids.shape[1] * ids.shape[2]
        print(f"rep={rep} B={B} V1={C + 1} {prec} ids={n} sampler_rng={rng}: {dt:.3f} s -> {B * n / dt:.0f} ids/s, peak allocated "
              f"{torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB (uniform buffer {4 * n * B * (C + 1) / 2 ** 20:.0f} MiB)", flush=True)
