"""numpy / torch restatement of classifier-free guidance on the condition as include/omlm.h states it (no GPU, no library), used by
tests/test_guidance_host.py (CPU) and tests/test_gpu_guidance.py (GPU).

  * the null condition: raw id -1 - codebook (p mod Q) at position p of token sequence 0 -- -1 after the per-quantizer offset, the zero
    row of every embedding path (`null_raw_ids`, `null_twin`);
  * the guide rule in float32 with exactly three roundings, in this order: d = l - n; m = s * d; g = n + m (`guide`).  numpy rounds every
    float32 operation to float32, so the result is the kernel's bit for bit;
  * the training drop on the outputs of TokenConditionedTransformerWrapper._prepare (`apply_drop`): sample b with u_b < p gets the null
    raw ids at the condition's id positions and key mask 1 there before the forgetful mask is ANDed in; its appended eos and everything
    else stay;
  * `factor(s)` = |s| + |1 - s|: g is the linear combination s l + (1 - s) n of two rows, so an error bound e on each row's entries
    gives factor(s) e on g's.
"""
import numpy as np
import torch


def null_raw_ids(codebook: int, Q: int, n: int) -> torch.Tensor:
    """[n] int64."""
    p = torch.arange(n, dtype=torch.long)
    return -1 - codebook * (p % Q) if Q > 1 else torch.full((n,), -1, dtype=torch.long)


def null_twin(cond_flat: torch.Tensor, codebook: int, Q: int, n_ids: int) -> torch.Tensor:
    """cond_flat [B, L] (n_ids id positions, then possibly an eos) -> the same with the id positions replaced by the null raw ids."""
    out = cond_flat.clone()
    out[:, :n_ids] = null_raw_ids(codebook, Q, n_ids).to(cond_flat.device)
    return out


def guide(cond, null, s) -> np.ndarray:
    """float32 arrays (or tensors) of one shape -> g = null + (s * (cond - null)), each operation rounded to float32."""
    l = np.ascontiguousarray(cond.detach().cpu().numpy() if isinstance(cond, torch.Tensor) else cond, dtype=np.float32)
    n = np.ascontiguousarray(null.detach().cpu().numpy() if isinstance(null, torch.Tensor) else null, dtype=np.float32)
    s = np.float32(s)
    with np.errstate(all="ignore"):
        d = np.subtract(l, n, dtype=np.float32)
        m = np.multiply(s, d, dtype=np.float32)
        return np.add(n, m, dtype=np.float32)


def guide64(cond, null, s) -> torch.Tensor:
    """The same combination in fp64 (the oracle side)."""
    return null.double() + float(s) * (cond.double() - null.double())


def factor(s) -> float:
    return abs(float(s)) + abs(1.0 - float(s))


def log_softmax64(g) -> torch.Tensor:
    g = torch.as_tensor(g).double()
    return torch.log_softmax(g, dim=-1)


def apply_drop(ids0, mask, forget, u, p, codebook: int, Q: int, n_ids: int):
    """ids0 [B, L] and mask [B, N] as _prepare returns them WITHOUT the drop (mask already ANDed with `forget`, or forget None), u [B]
    float32, p the drop probability (compared in float32) -> (ids0, mask) with the drop: u_b < p."""
    dropped = torch.as_tensor(np.asarray(u.detach().cpu().numpy(), dtype=np.float32) < np.float32(p)).to(ids0.device)
    out = torch.where(dropped[:, None], null_twin(ids0, codebook, Q, n_ids), ids0)
    m = mask.clone()
    live = torch.ones_like(m[:, 1:1 + n_ids]) if forget is None else forget[:, 1:1 + n_ids].to(m.device)
    m[:, 1:1 + n_ids] = torch.where(dropped[:, None], live, m[:, 1:1 + n_ids])
    return out, m, dropped
