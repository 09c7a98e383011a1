"""One full-width training step past 4096 positions, eagerly: coarse musiclm_small geometry (dim 1024, 8 heads, depth 6), B = 2,
N = 8200 (683 semantic + 2500 x 3 coarse ids), forward + backward + optimizer step in "fp16ff" and in "bf16" from the same weights and ids.
Prints each leg's loss, gradient norm proxy and time, and the relative difference of the two losses (bar: test_gpu_model.TOL["bf16"]["logits"]).

usage: tools/long_step_probe.py [B [semantic_steps [coarse_steps]]]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from open_musiclm_amd import open_musiclm as M
from open_musiclm_amd.optimizer import get_optimizer

B, S, Cs = (int(a) for a in (sys.argv[1:] + ["2", "683", "2500"][len(sys.argv) - 1:])[:3])
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1234)
ids = [torch.randint(0, 1024, (B, 1, 12), generator=g), torch.randint(0, 1024, (B, S), generator=g), torch.randint(0, 1024, (B, Cs, 3), generator=g)]
losses = {}
for precision in ("fp16ff", "bf16"):
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, attn_dropout=0.0, ff_dropout=0.0, num_coarse_quantizers=3,
                                        precision=precision).to(dev)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.],
                                                   mask_prob=0.0)
    wrapper.train()
    optim = get_optimizer(model.parameters(), lr=3e-4, wd=0.01)
    optim.zero_grad()
    w0 = model.transformer.layers[0][2].w_in.weight.detach().clone()
    torch.cuda.synchronize()
    t0 = time.time()
    loss, _, _ = wrapper(all_token_ids=[t.to(dev) for t in ids], return_loss=True)
    loss.backward()
    optim.mark_grads_dirty()
    optim.step(max_grad_norm=0.5, grad_scale=1.0)
    torch.cuda.synchronize()
    dt = time.time() - t0
    gq = model.transformer.layers[5][0].to_q.weight.grad
    moved = float((model.transformer.layers[0][2].w_in.weight.detach() - w0).abs().max())
    N = 12 + S + 3 * Cs + 5
    losses[precision] = float(loss)
    print(f"{precision:7s} B {B} N {N} loss {float(loss):.6f} finite {bool(torch.isfinite(loss))} grads finite "
          f"{all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)} |dWq5|max {float(gq.abs().max()):.3e} "
          f"weights moved {moved:.3e} step {dt:.2f} s peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    del model, wrapper, optim
    torch.cuda.empty_cache()
rel = abs(losses["fp16ff"] - losses["bf16"]) / abs(losses["bf16"])
print(f"loss fp16ff vs bf16: rel diff {rel:.2e} (bar 1.2e-2)")
sys.exit(0 if rel < 1.2e-2 and all(l == l for l in losses.values()) else 1)
