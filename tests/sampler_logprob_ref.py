"""fp64 restatement of the two log-probabilities of a sampled id stated in include/omlm.h, used by tests/test_gpu_sampler_logprob.py (GPU)
and tests/test_sampler_logprob_host.py (CPU); built on sampler_top_p_ref.Ranked (its nucleus_mask, and loss_optim_sampler_ref.kept_mask
for top_p = 1).

For a row of V logits l_c, forbid_last, k, T > 0, 0 < p <= 1 and the id s the sampler returned:
  lp_model   = l_s - log sum_{c < V} exp(l_c)             (T = 1, all V entries, the last one even when it is forbidden);
  lp_sampled = l_s / T - log sum_{c in N} exp(l_c / T)    (N: the top-k kept set, cut to the nucleus when p < 1, last logit -inf if forbidden).
A -inf logit contributes 0; when the largest kept logit is -inf (the "id 0" rule) both are -inf; a one-entry N gives exactly 0.

The tolerance of the kernels' fp32 values against these: tol(l_s, m, T) = 2e-5 + 8 2^-24 (|l_s| + |m|) / T.
  - the roundings of l / T, of the subtraction and of m / T are each at most 1 ulp of the larger operand: the second term, with a factor 2
    to spare;
  - a sum of at most 65536 non-negative fp32 terms formed as at most 64 serial adds per lane plus at most 10 tree levels has a relative
    error of at most 74 2^-24 ~ 4.4e-6, the same absolute error after the logarithm;
  - expf and logf cost a few ulp each;
  together below 1e-5: the constant is twice that.

The kernels cut the nucleus in 2^40 fixed point, so their set N lies between N- (cut at p (1 - DELTA)) and N+ (cut at p (1 + DELTA)),
which are nested: lo = l_s / T - lse(N+) <= lp_sampled <= hi = l_s / T - lse(N- with s) (`bracket`).  All functions take tensors on any
device."""
import torch

import loss_optim_sampler_ref as R
import sampler_top_p_ref as P

DELTA = P.DELTA
NEG = float("-inf")


def tol(l_s, m, temperature):
    """Elementwise on tensors (or floats): the bound derived above."""
    return 2e-5 + 8 * 2.0 ** -24 * (abs(l_s) + abs(m)) / temperature


def _lse(x):
    """log-sum-exp over dim 1 in fp64; -inf for a row of -inf (no NaN)."""
    m = x.max(dim=1, keepdim=True).values
    ok = torch.isfinite(m)
    s = torch.exp(x - torch.where(ok, m, torch.zeros_like(m))).sum(dim=1)
    return torch.where(ok[:, 0], m[:, 0] + torch.log(s), torch.full_like(s, NEG))


def largest_kept(logits, forbid_last):
    """[B] fp64: m, the largest kept logit -- the row maximum after the last logit is forbidden (top-k and nucleus both keep it)."""
    return R._forbid(logits, forbid_last).max(dim=1).values


def lp_model(logits, ids, forbid_last=False):
    """[B] fp64.  forbid_last only decides the -inf rule (m = -inf): the sum runs over all V entries either way."""
    x = logits.double()
    ls = x.gather(1, ids.long()[:, None])[:, 0]
    out = ls - _lse(x)
    dead = ~torch.isfinite(largest_kept(logits, forbid_last))
    return torch.where(dead | (ls == NEG), torch.full_like(out, NEG), out)


def kept_set(logits, k, temperature, p, forbid_last, ranked=None):
    """[B, V] bool: N."""
    if p >= 1.0:
        return R.kept_mask(logits, k, forbid_last)
    return (ranked or P.Ranked(logits, k, forbid_last)).nucleus_mask(temperature, p)


def lp_sampled(logits, ids, k, temperature, p, forbid_last, mask=None):
    """[B] fp64; `mask` ([B, V] bool) replaces N (the bracket's sets)."""
    x = R._forbid(logits, forbid_last)
    if mask is None:
        mask = kept_set(logits, k, temperature, p, forbid_last)
    ls = x.gather(1, ids.long()[:, None])[:, 0]
    out = ls / temperature - _lse(torch.where(mask, x / temperature, torch.full_like(x, NEG)))
    dead = ~torch.isfinite(x.max(dim=1).values)
    return torch.where(dead | (ls == NEG), torch.full_like(out, NEG), out)


def bracket(logits, ids, k, temperature, p, forbid_last, ranked=None, delta=DELTA):
    """(lo, hi, same): lp_sampled on N+ and on N- with s added, [B] fp64 each (lo <= hi), and [B] bool N- == N+."""
    rk = ranked or P.Ranked(logits, k, forbid_last)
    n_minus, n_plus = rk.nucleus_mask(temperature, p * (1 - delta)), rk.nucleus_mask(temperature, min(p * (1 + delta), 1.0))
    with_s = n_minus.clone()
    with_s.scatter_(1, ids.long()[:, None], True)
    lo = lp_sampled(logits, ids, k, temperature, p, forbid_last, mask=n_plus)
    hi = lp_sampled(logits, ids, k, temperature, p, forbid_last, mask=with_s)
    return lo, hi, (n_minus == n_plus).all(dim=1)
