"""fp64 restatement of the sampler's nucleus (top-p) rule stated in include/omlm.h, used by tests/test_gpu_sampler_top_p.py (GPU) and
tests/test_sampler_top_p_host.py (CPU); built on loss_optim_sampler_ref.kept_mask.

For a row of V logits, forbid_last, k, T > 0 and 0 < p < 1:
  1. the last logit becomes -inf if forbidden;
  2. S = the top-k kept set (strictly above the k-th value, then the lowest indices among the equals);
  3. m = the largest logit in S; if m is -inf the id is 0.  Otherwise w_c = exp((l_c - m) / T) for c in S (0 for -inf), W = sum of w_c;
  4. rank S by logit descending, then index ascending: c is in the nucleus iff the mass of the entries ranked strictly before it is < p W;
  5. the id is the first maximum of l_c / T - log(-log(u_c + 1e-20) + 1e-20) over the nucleus.

The kernels form the masses in 2^40 fixed point from fp32 weights, so their cut may sit anywhere within p (1 +- DELTA) of this one:
the truncation is at most n 2^-40 <= 2^-24 of W (W >= 1), the fp32 argument of the exponential contributes at most
(sum of w |a|) 2^-23 <= ln(n) 2^-23 W ~ 1.3e-6 W, expf a few ulp: together below 2^-18, and DELTA = 2^-16.  The nuclei are nested in p, so
where the cuts p (1 - DELTA) and p (1 + DELTA) give one id, every cut in between gives it; `ambiguous_rows` marks the other rows.

All functions take tensors on any device (the GPU test runs them on the GPU in fp64) and share one sort per (logits, k, forbid_last):
`Ranked`."""
import torch

import loss_optim_sampler_ref as R

DELTA = 2.0 ** -16


class Ranked:
    """A batch of rows with S formed and ranked (steps 1, 2 and the order of step 4): what does not depend on T, p or u."""

    def __init__(self, logits: torch.Tensor, k: int, forbid_last: bool):
        self.x = R._forbid(logits, forbid_last)                              # fp64
        self.S = R.kept_mask(logits, k, forbid_last)
        xs = torch.where(self.S, self.x, torch.full_like(self.x, float("-inf")))
        # descending by logit, ascending by index among equals (stable); entries outside S sort as -inf and are masked out again below
        self.sorted, self.order = torch.sort(xs, dim=1, descending=True, stable=True)

    def nucleus_mask(self, temperature: float, p: float) -> torch.Tensor:
        """[B, V] bool: the nucleus (a row whose m is -inf keeps S: its id is 0 either way)."""
        m = self.sorted[:, :1]
        ok = torch.isfinite(m)
        w = torch.where(ok, torch.exp((self.sorted - torch.where(ok, m, torch.zeros_like(m))) / temperature), torch.zeros_like(self.sorted))
        before = torch.cumsum(w, dim=1) - w
        ins = (before < p * w.sum(dim=1, keepdim=True)) | ~ok
        mask = torch.zeros_like(self.S).scatter_(1, self.order, ins)
        return mask & self.S

    def scores(self, uniform: torch.Tensor, temperature: float, p: float) -> torch.Tensor:
        """[B, V] fp64: l / T + Gumbel(u) on the nucleus, -inf elsewhere."""
        g = -torch.log(-torch.log(uniform.double() + 1e-20) + 1e-20)
        w = self.x / temperature + g
        return torch.where(self.nucleus_mask(temperature, p), w, torch.full_like(w, float("-inf")))

    def sample(self, uniform, temperature, p):
        return self.scores(uniform, temperature, p).argmax(dim=1)            # the first maximum

    def ambiguous_rows(self, uniform, temperature, p, delta=DELTA):
        """[B] bool: rows whose id differs between the cuts p (1 - delta) and p (1 + delta)."""
        return self.sample(uniform, temperature, p * (1 - delta)) != self.sample(uniform, temperature, p * (1 + delta))


def nucleus_mask(logits, k, temperature, p, forbid_last):
    return Ranked(logits, k, forbid_last).nucleus_mask(temperature, p)


def scores(logits, uniform, k, temperature, p, forbid_last):
    return Ranked(logits, k, forbid_last).scores(uniform, temperature, p)


def sample(logits, uniform, k, temperature, p, forbid_last):
    """[B] int64 ids."""
    return Ranked(logits, k, forbid_last).sample(uniform, temperature, p)


def ambiguous_rows(logits, uniform, k, temperature, p, forbid_last, delta=DELTA):
    return Ranked(logits, k, forbid_last).ambiguous_rows(uniform, temperature, p, delta)


# ---- the inputs of the comparison against the kernels (the GPU test runs them; the host test bounds their ambiguous rows) -------------
COMPARE_V = [1, 2, 64, 1025, 1088, 1089, 2048, 2049, 4096, 4097, 16384, 16385, 65536]      # every instantiation and seam
COMPARE_P = [0.05, 0.5, 0.9, 0.999]
COMPARE_T = [0.4, 1.0]
AMBIGUOUS_CAP = 1                                     # rows per case (a case: up to 64 rows at one V, k, p, T, forbid_last)


def compare_rows(V):
    """(logits [B, V], uniform [B, V]) float32 on the CPU: B = 64 (16 at V = 65536); even rows N(0, 1), odd rows N(0, 16) logits, row 1
    heavy ties (values from a set of 4), row 2 all -inf."""
    B = 16 if V >= 65536 else 64
    g = torch.Generator().manual_seed(4000 + V)
    x = torch.randn(B, V, generator=g)
    x[1::2] *= 4
    x[1] = torch.randint(0, 4, (V,), generator=g).float()
    x[2] = float("-inf")
    u = torch.rand(B, V, generator=g)
    return x, u


def compare_ks(V):
    return sorted({1, max(int(0.1 * V), 1), V})
