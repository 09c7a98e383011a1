"""Plain fp64 restatement of the regularised cross-entropy row rule of include/omlm.h (label smoothing eps, z-loss zeta) and of its
gradient, used by tests/test_ce_reg_host.py (CPU, against torch) and tests/test_gpu_ce_reg.py (GPU, against the kernels).  No package
import: torch only.

A live row (label y in [0, V)) with logits l[0..V), lse = log sum_c exp l[c], p = exp(l - lse):
    nll = lse - l[y]        smooth = lse - (1 / V) sum_c l[c]        z = lse^2
    row loss = (1 - eps) nll + eps smooth + zeta z
    d row loss / d l[c] = p[c] (1 + 2 zeta lse) - (1 - eps) [c == y] - eps / V
Rows whose label is negative (ignore_index) or >= V add nothing and get zero gradients."""
import torch


def live_rows(labels: torch.Tensor, V: int) -> torch.Tensor:
    return (labels >= 0) & (labels < V)


def row_terms(logits: torch.Tensor, labels: torch.Tensor):
    """logits [R, V] (any float type), labels [R] (any int type) -> (lse, nll, smooth, z), fp64 [R] each; nll / smooth / z are 0 on rows
    that are not live."""
    x = logits.double()
    V = x.shape[1]
    live = live_rows(labels, V)
    lse = torch.logsumexp(x, 1)
    own = x.gather(1, labels.long().clamp(0, V - 1)[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    nll = torch.where(live, lse - own, zero)
    smooth = torch.where(live, lse - x.sum(1) / V, zero)
    z = torch.where(live, lse * lse, zero)
    return lse, nll, smooth, z


def sums(logits, labels):
    """(NLL, S, Z): the three sums over the live rows, Python floats."""
    _, nll, smooth, z = row_terms(logits, labels)
    return float(nll.sum()), float(smooth.sum()), float(z.sum())


def loss_sum(logits, labels, eps: float, zeta: float) -> float:
    n, s, z = sums(logits, labels)
    return (1.0 - eps) * n + eps * s + zeta * z


def grad(logits: torch.Tensor, labels: torch.Tensor, eps: float, zeta: float, lse: torch.Tensor = None) -> torch.Tensor:
    """fp64 [R, V]: d (sum of row losses) / d logits.  `lse` (fp64 [R]): a log-sum-exp to use in place of the exact one (the backward
    kernel's own input)."""
    x = logits.double()
    R, V = x.shape
    live = live_rows(labels, V)
    if lse is None:
        lse = torch.logsumexp(x, 1)
    lse = lse.double()
    g = torch.exp(x - lse[:, None]) * (1.0 + 2.0 * zeta * lse)[:, None] - eps / V
    rows = torch.arange(R)[live]
    g[rows, labels[live].long()] -= 1.0 - eps
    g[~live] = 0.0
    return g
