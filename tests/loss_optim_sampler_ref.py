"""Plain fp64 restatements of the fused sampler's kept-set rule and of the fp16 loss-scale state machine, used by
tests/test_gpu_loss_optim_sampler.py (GPU) and tests/test_sampler_ref_host.py (CPU).

Sampler (csrc/sampler.hip, sample_kernel): with `forbid_last` the last logit is -inf first; every entry strictly above the k-th
largest value is kept, and of the entries equal to it the LOWEST indices are kept until k entries are kept; the id is the first maximum of
l / T - log(-log(u + 1e-20) + 1e-20) over the kept entries (index 0 when every kept entry is -inf, as torch.argmax of an all -inf row)."""
import torch


def _forbid(logits: torch.Tensor, forbid_last: bool) -> torch.Tensor:
    x = logits.double().clone()
    if forbid_last:
        x[:, -1] = float("-inf")
    return x


def kept_mask(logits: torch.Tensor, k: int, forbid_last: bool) -> torch.Tensor:
    """[B, V] bool: the entries the sampler keeps (the rule in the module docstring)."""
    x = _forbid(logits, forbid_last)
    B, V = x.shape
    kth = x.sort(dim=1, descending=True).values[:, k - 1:k]           # the k-th largest value of each row
    gt = x > kth
    eq = x == kth
    n_eq_keep = k - gt.sum(1, keepdim=True)
    rank = eq.long().cumsum(1) - 1                                      # rank of an equal entry among the equal entries, by index
    return gt | (eq & (rank < n_eq_keep))


def gumbel_scores(logits: torch.Tensor, uniform: torch.Tensor, k: int, temperature: float, forbid_last: bool) -> torch.Tensor:
    """[B, V] fp64: l / T + Gumbel(u) on the kept entries, -inf elsewhere."""
    x = _forbid(logits, forbid_last)
    g = -torch.log(-torch.log(uniform.double() + 1e-20) + 1e-20)
    w = x / temperature + g
    return torch.where(kept_mask(logits, k, forbid_last), w, torch.full_like(w, float("-inf")))


def sample(logits, uniform, k, temperature, forbid_last):
    """[B] int64 ids: the first maximum of gumbel_scores (torch.argmax returns the first maximum)."""
    return gumbel_scores(logits, uniform, k, temperature, forbid_last).argmax(dim=1)


def near_tie_rows(scores: torch.Tensor, rel: float = 1e-5):
    """Rows whose best and second-best kept scores are within rel * max(1, |best|): there an fp32 logf may order them either way.
    Returns (mask [B], best index [B], second index [B])."""
    top = scores.topk(2, dim=1) if scores.shape[1] > 1 else None
    if top is None:
        z = torch.zeros(scores.shape[0], dtype=torch.long)
        return torch.zeros(scores.shape[0], dtype=torch.bool), z, z
    v, i = top
    finite = torch.isfinite(v[:, 1])
    near = finite & ((v[:, 0] - v[:, 1]) <= rel * v[:, 0].abs().clamp(min=1.0))
    return near, i[:, 0], i[:, 1]


def loss_scale_update(state, finite: bool, growth: float, backoff: float, interval: int, smin: float, smax: float):
    """One omlm_loss_scale_update on the 5-slot state {scale, good steps, skipped steps, applied steps, scale of the last step}
    (GradScaler's rule with clamps).  Returns the new state as a list of Python floats."""
    s = [float(x) for x in state]
    s[4] = s[0]
    if not finite:
        s[0] = max(s[0] * backoff, smin)
        s[1] = 0.0
        s[2] += 1.0
    else:
        s[3] += 1.0
        s[1] += 1.0
        if interval > 0 and s[1] >= interval:
            s[0] = min(s[0] * growth, smax)
            s[1] = 0.0
    return s
