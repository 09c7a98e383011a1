"""Attention timing past 4096 positions: forward and backward of one layer by HIP events, in us and in us per 1e9 live (query, key, head)
triples (B H N (N + 1) / 2: the key mask is not counted).

usage: tools/attn_long_probe.py [B H N ...]          default: 2 8 4096  2 8 8192  2 8 16384  32 8 1116
       DTYPE=fp16|bf16 (default fp16), REPS (default 5)

The events bracket the library calls, so the backward figure is the dQ kernel, the d(bias) reduction and the dK / dV kernel (with its slot
reduction past N = 4096) together; their split is read from a kernel trace of the same run:
       rocprofv3 --kernel-trace --stats -d <dir> -- python tools/attn_long_probe.py ...
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import ops

dev = torch.device("cuda:0")
DT = torch.float16 if os.environ.get("DTYPE", "fp16") == "fp16" else torch.bfloat16
REPS = int(os.environ.get("REPS", "5"))
args = [int(a) for a in sys.argv[1:]] or [2, 8, 4096, 2, 8, 8192, 2, 8, 16384, 32, 8, 1116]
assert len(args) % 3 == 0, __doc__


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


for B, H, N in zip(args[0::3], args[1::3], args[2::3]):
    g = torch.Generator().manual_seed(0)
    M = B * N
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    q = unit(torch.randn(B, N, H, 64, generator=g)).reshape(M, H * 64).to(dev).to(DT)
    k = unit(torch.randn(M, 64, generator=g)).to(dev).to(DT)
    v = torch.randn(M, 64, generator=g).to(dev).to(DT)
    ld = (H + 7) // 8 * 8
    bias = torch.zeros(N, ld)
    bias[:, :H] = torch.randn(N, H, generator=g) * 0.1
    bias = bias.to(dev)
    mask = (torch.rand(B, N, generator=g) > 0.15).to(torch.uint8).to(dev)
    mask[:, 0] = 1
    out, lse = torch.empty_like(q), torch.empty(B, H, N, device=dev)
    dout = torch.randn(M, H * 64, generator=g).to(dev).to(DT)
    delta = torch.empty(B, H, N, device=dev)
    dq, dk, dv = torch.empty(M, H * 64, device=dev), torch.empty(M, 64, device=dev), torch.empty(M, 64, device=dev)
    dbias = torch.zeros(N, ld, device=dev)
    ab = ops.AttnBias(bias, N, H, dev, qk_bound=1.0, half=DT == torch.float16)      # the fixed-reference forward, as the model runs it
    triples = B * H * N * (N + 1) / 2 / 1e9
    tf = timed(lambda: ops.attn_fwd(q, k, v, ab, mask, out, lse, B, N, H, 8.0))
    tb = timed(lambda: ops.attn_bwd(q, k, v, ab, mask, out, dout, lse, delta, dq, dk, dv, dbias, B, N, H, 8.0))
    print(f"B {B:3d} H {H:2d} N {N:6d} {str(DT)[6:]:8s} fwd {tf:10.1f} us {tf / triples:8.1f} us/Gtriple   bwd {tb:10.1f} us {tb / triples:8.1f} us/Gtriple"
          f"   checksum {float(out.float().abs().sum()):.6e}", flush=True)
    del q, k, v, out, dout, dq, dk, dv
