"""GPU: the workgroup-wide sampler (csrc/sampler.hip, sample_wide_kernel) that serves rows of 2048 < V <= 65536 logits -- the same
function of (logits, uniforms, k, T, forbid_last) as the wave kernel, checked against the fp64 restatement in loss_optim_sampler_ref.py
with the recipes of test_gpu_loss_optim_sampler.py, and against the wave kernel itself.

Widths: 2049 is the first width on the wide route (4 slots per lane, 9 waves), 4097 the first with 16 slots, 16385 the first with 64
slots, 65536 the last width the sampler takes (64 slots, 16 waves).  A wave owns 64 * slots contiguous indices: segments of 256 entries
at V = 2049 and of 4096 at V = 65536."""

import pytest
import torch

import loss_optim_sampler_ref as R
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_loss_optim_sampler import _check_ids, _gen, _probe_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
B = 16
SEGMENT = {2049: 256, 65536: 4096}               # indices one wave owns (64 lanes x slots per lane)


@pytest.mark.parametrize("V", [2049, 2050, 4097, 16385, 65536])
def test_wide_sampler_random_rows_against_fp64(ops, dev, V):
    """The recipe of test_sampler_random_rows_against_fp64 with 16 rows: ids equal the fp64 reference's, except on rows whose best two
    reference scores lie within 1e-5 relative (one of the two); such rows are fewer than 1 % (the reference alone: 0 of 384 per V)."""
    g = _gen(V)
    ld = V + 5
    ks = sorted({k for k in (1, 2, max(int(0.1 * V), 1), V) if k <= V})
    rows = near = 0
    for k in ks:
        for T in (0.5, 1.0, 2.0):
            for forbid in (False, True):
                x = torch.randn(B, V, generator=g) * 4
                x[1:4] = torch.randint(0, 6, (3, V), generator=g).float()                    # integer rows: ties at the threshold
                for r, n_inf in ((4, V // 10), (5, min(V, V - k + (k + 1) // 2)), (6, V)):  # -inf entries; more than V - k; all
                    x[r, torch.randperm(V, generator=g)[:n_inf]] = -INF
                logits = torch.full((B, ld), NAN)
                logits[:, :V] = x
                u = torch.rand(B, V, generator=g)
                out = torch.full((B,), -7, dtype=torch.long, device=dev)
                ops.sample_topk_gumbel(logits.to(dev), u.to(dev), out, V, k, T, forbid)
                near += _check_ids(out.cpu(), x, u, k, T, forbid)
                rows += B
    report(f"sampler_wide_random[V={V}]", rows=rows, near_tie_rows=near)
    assert near < 0.01 * rows, (near, rows)


def _boundary_pair(V, k, b, g):
    """Two equal rows of integer logits whose k-th value (4) is tied, with the LAST kept tied entry at index b - 1 and the FIRST dropped one
    at index b.  Row 0 puts u = 1 - 2^-24 on b - 1 (the id must be b - 1), row 1 on b (the id must not be b)."""
    x = torch.randint(0, 4, (V,), generator=g).float()
    x[torch.randperm(V, generator=g)[:k // 2]] = 5.0
    x[b - 1] = x[b] = 4.0
    n5 = int((x == 5.0).sum())
    free = (x[:b - 1] != 5.0).nonzero().flatten()
    x[free[torch.randperm(len(free), generator=g)[:k - n5 - 1]]] = 4.0                     # with b - 1: exactly k - n5 fours up to b - 1
    later = b + 1 + torch.randperm(V - b - 1, generator=g)[:V // 5]
    x[later[x[later] != 5.0]] = 4.0                                                       # more dropped fours behind b
    x = x.repeat(2, 1)
    u = 0.01 + 0.98 * torch.rand(2, V, generator=g)
    u[0, b - 1] = u[1, b] = 1.0 - 2.0 ** -24
    keep = R.kept_mask(x, k, False)
    assert bool(keep[0, b - 1]) and not bool(keep[0, b]) and float(x[0].sort(descending=True).values[k - 1]) == 4.0   # the construction works
    return x, u


@pytest.mark.parametrize("V", [2049, 65536])
@pytest.mark.parametrize("exact", [False, True])
def test_wide_sampler_kept_set_probes(ops, dev, V, exact):
    """test_sampler_kept_set_probes at the wide widths, plus one pair of rows whose last kept and first dropped tied entries are index
    neighbours on either side of a wave's segment boundary (a multiple of 64 too): the offset scan over the waves decides the id."""
    g = _gen(V + exact)
    b = 4 * SEGMENT[V] if V == 2049 else 5 * SEGMENT[V]
    assert b % 64 == 0 and b % SEGMENT[V] == 0
    for k in (max(int(0.1 * V), 1), 2 * max(int(0.1 * V), 1) + 1):
        for T in (0.5, 1.0, 2.0):
            x, u, probes = _probe_rows(V, k, exact, g)
            want = R.sample(x, u, k, T, False)
            even = torch.arange(len(probes)) % 2 == 0
            assert torch.equal(want[even], probes[even]) and not bool((want[~even] == probes[~even]).any())     # the probe works
            out = torch.empty(len(probes), dtype=torch.long, device=dev)
            ops.sample_topk_gumbel(x.to(dev), u.to(dev), out, V, k, T, False)
            got = out.cpu()
            assert torch.equal(got[even], probes[even]), (k, T, got[even], probes[even])        # the last kept tied index is kept
            assert not bool((got[~even] == probes[~even]).any()), (k, T)                          # the first dropped one is dropped
            _check_ids(got, x, u, k, T, False)
        xb, ub = _boundary_pair(V, k, b, g)
        out = torch.empty(2, dtype=torch.long, device=dev)
        ops.sample_topk_gumbel(xb.to(dev), ub.to(dev), out, V, k, 1.0, False)
        got = out.cpu()
        assert int(got[0]) == b - 1 and int(got[1]) != b, (k, b, got)
        _check_ids(got, xb, ub, k, 1.0, False)
    report(f"sampler_wide_probes[V={V},exact={exact}]", exact=True)


@pytest.mark.parametrize("k", [1, 204, 2048])
def test_wide_and_wave_kernels_are_one_function(ops, dev, k):
    """Rows of 2048 logits through the wave kernel (V = 2048) and, with a forbidden 2049th column appended, through the workgroup kernel
    (V = 2049, forbid_last): the same fp32 expression and the same tie rule, so identical ids -- no near-tie allowance."""
    g = _gen(7 + k)
    for T in (0.5, 1.0, 2.0):
        x = torch.randn(B, 2048, generator=g) * 4
        x[1:4] = torch.randint(0, 6, (3, 2048), generator=g).float()
        x[4, torch.randperm(2048, generator=g)[:1900]] = -INF
        u = torch.rand(B, 2049, generator=g)
        xa = torch.cat((x, torch.randn(B, 1, generator=g) * 4 + 20.0), dim=1)                 # a finite last column that would win if it were kept
        a = torch.full((B,), -7, dtype=torch.long, device=dev)
        bb = torch.full((B,), -7, dtype=torch.long, device=dev)
        ops.sample_topk_gumbel(xa.to(dev), u.to(dev), a, 2049, k, T, True)
        ops.sample_topk_gumbel(x.to(dev), u[:, :2048].contiguous().to(dev), bb, 2048, k, T, False)
        assert torch.equal(a, bb), (k, T, a.tolist(), bb.tolist())
        assert bool(((a >= 0) & (a < 2048)).all())
    report(f"sampler_wide_equals_wave[k={k}]", exact=True)


def test_wide_sampler_at_and_embed_at(ops, dev):
    """test_sampler_at_and_embed_at at V = 4097: only slot step_dev[0] of hist is written; the gathered row is the clamped table row."""
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    V = 4097
    g = _gen(V + 3)
    Bq, steps, D, ld = 6, 5, 128, V + 7
    k, T = max(int(0.1 * V), 1), 0.95
    x = torch.randn(Bq, V, generator=g) * 4
    logits = torch.full((Bq, ld), NAN)
    logits[:, :V] = x
    U = torch.rand(steps, Bq, V, generator=g)
    lg, Ud = logits.to(dev), U.to(dev)
    step_dev = torch.tensor([3], dtype=torch.int32, device=dev)
    plain = torch.empty(Bq, dtype=torch.long, device=dev)
    ops.sample_topk_gumbel(lg, Ud[3].contiguous(), plain, V, k, T, True)
    _check_ids(plain.cpu(), x, U[3], k, T, True)
    out = torch.full((Bq,), -7, dtype=torch.long, device=dev)
    hist = torch.full((steps, Bq), -7, dtype=torch.long, device=dev)
    call("omlm_sample_topk_gumbel_at", ptr(lg), ptr(Ud), ptr(step_dev), ptr(out), ptr(hist), Bq, V, ld, k, T, 1, stream_ptr())
    h = hist.cpu()
    assert torch.equal(out, plain) and torch.equal(h[3], plain.cpu())
    assert bool((h[torch.arange(steps) != 3] == -7).all())                 # only slot 3 written
    E = 2 * V
    emb = torch.randn(E, D, generator=g).to(dev)
    for offset in (7, -V, E - V // 2):                                      # inside; every row clamped to 0; upper rows clamped to E - 1
        out.fill_(-7)
        hist.fill_(-7)
        xo = torch.full((Bq, D), NAN, device=dev)
        call("omlm_sample_embed_at", ptr(lg), ptr(Ud), ptr(step_dev), ptr(out), ptr(hist), Bq, V, ld, k, T, 1,
             ptr(emb), offset, E, ptr(xo), D, stream_ptr())
        assert torch.equal(out, plain) and torch.equal(hist[3], plain)
        r = (plain + offset).clamp(0, E - 1)
        assert torch.equal(xo, emb[r])                                      # a copy of the clamped row: bit-equal
    report(f"sampler_wide_at_embed_at[V={V}]", exact=True)


def test_wide_sampler_limit(ops, dev):
    """V = 65537 is refused before any launch, by the Python wrapper (ValueError) and by the C entry point: both name the limit and
    leave the output buffer as it was."""
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    V = 65537
    assert ops.SAMPLER_MAX_V == 65536
    logits = torch.zeros(2, V, device=dev)
    u = torch.full((2, V), 0.5, device=dev)
    out = torch.full((2,), -7, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="65536"):
        ops.sample_topk_gumbel(logits, u, out, V, 10, 1.0, True)
    with pytest.raises(RuntimeError, match="65536"):
        call("omlm_sample_topk_gumbel", ptr(logits), ptr(u), ptr(out), 2, V, V, 10, 1.0, 1, stream_ptr())
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7, -7]
    ops.sample_topk_gumbel(logits[:, :65536].contiguous(), u[:, :65536].contiguous(), out, 65536, 10, 1.0, True)      # the limit itself samples
    assert bool(((out >= 0) & (out < 65535)).all())
