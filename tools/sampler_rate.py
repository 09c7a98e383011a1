"""Microseconds per sampler call (B in 1, 16, 64) and per cached decode step with its sampler (dim 1024, depth 6, fp16ff, B in 1, 16) at the
given row widths V1, for the library OMLM_LIB_PATH names (A/B against another build) or the package's own.  One JSON line per figure, also
appended to --out.  profiles/sampler_wide.md holds a run."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tag", required=True)
ap.add_argument("--what", choices=["sampler", "step"], required=True)
ap.add_argument("--widths", type=int, nargs="+", required=True)
ap.add_argument("--out", required=True)
a = ap.parse_args()
from open_musiclm_amd import decode, hip, ops
from open_musiclm_amd import open_musiclm as M
hip.lib()
dev = torch.device("cuda:0")
out = open(a.out, "a")


def emit(**kw):
    kw["tag"] = a.tag
    out.write(json.dumps(kw) + "\n"); out.flush()
    print(json.dumps(kw), flush=True)


def time_calls(fn, calls, reps):
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return us


if a.what == "sampler":
    g = torch.Generator().manual_seed(1)
    for V1 in a.widths:
        for B in (1, 16, 64):
            ld = (V1 + 7) // 8 * 8
            lg = torch.zeros(B, ld)
            lg[:, :V1] = torch.randn(B, V1, generator=g) * 4
            lg, u = lg.to(dev), torch.rand(B, V1, generator=g).to(dev)
            o = torch.zeros(B, dtype=torch.long, device=dev)
            k = max(int(0.1 * V1), 1)
            us = time_calls(lambda: ops.sample_topk_gumbel(lg, u, o, V1, k, 1.0, True), 500, 7)
            emit(what="sampler_us_per_call", V1=V1, B=B, median=statistics.median(us), lo=min(us), hi=max(us), ids=o[:4].tolist())
else:
    n_new = 256
    for V1 in a.widths:
        torch.manual_seed(0)
        model = M.create_semantic_transformer(dim=1024, depth=6, heads=8, semantic_codebook_size=V1 - 1, ff_dropout=0.0, precision="fp16ff").to(dev)
        model.eval()
        g = torch.Generator().manual_seed(2)
        for B in (1, 16):
            cond = torch.cat((torch.randint(0, 1024, (B, 12), generator=g), torch.full((B, 1), 1024)), dim=1).to(dev)
            empty = torch.empty(B, 0, dtype=torch.long, device=dev)
            U = torch.rand(n_new, B, V1, generator=g).to(dev)
            k = max(int(0.1 * V1), 1)
            us = []
            with torch.no_grad():
                for rep in range(6):
                    dec = decode.CachedDecoder(model, B, 14 + 1 + n_new + 1, "fp16ff", wide=True)
                    last = dec.prefill([cond, empty])
                    loop = decode.SamplingLoop(dec, last, U, 0, n_new, k, 1.0, [True], use_graph=False)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ids = loop.run()
                    torch.cuda.synchronize()
                    if rep:                                   # the first pass warms every kernel up
                        us.append((time.perf_counter() - t0) * 1e6 / n_new)
            emit(what="decode_step_us_per_id", V1=V1, B=B, median=statistics.median(us), lo=min(us), hi=max(us), ids=ids[:3, 0].tolist())
