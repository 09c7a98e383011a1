"""GPU: the kernels at both ends of a training step and of a sampled token -- cross-entropy (csrc/embed_ce.hip), the token
gather, the top-k Gumbel sampler (csrc/sampler.hip), the Adam/AdamW step with its loss-scale machine and the grad-norm reduction (csrc/optim_misc.hip),
and FusedAdam end to end -- against fp64 torch on the CPU, on every route their launchers pick (wave / workgroup kernels, 16-byte /
element paths, <17> / <32> sampler slots) and past their grid caps.  Every bar sits next to its check with its reason; every measured
error goes to the kernel report through test_gpu_kernels.report()."""

import pytest
import torch

import loss_optim_sampler_ref as R
from test_gpu_kernels import dev, ops, relerr, report  # noqa: F401  (the shared fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    """x as the fp32 the kernel's C ABI receives (lr, betas, eps, wd are `float` arguments)."""
    return float(torch.tensor(x, dtype=torch.float32))


def _ulp(x, dtype):
    """Spacing of `dtype` at |x| (fp64 tensor): 2^(floor(log2 |x|) - mantissa bits), subnormal spacing below the normal range."""
    fi = torch.finfo(dtype)
    mant = {torch.bfloat16: 7, torch.float16: 10}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp(min=fi.tiny)))
    return torch.exp2(e - mant)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. cross-entropy
# V = 1088 is the widest row of the wave-per-row forward (64 lanes x 17 slots); 1089 and 2049 take the workgroup kernel.  R = 4097 is one
# row past a full trip of both forward grids (1024 x 4 rows, 4096 workgroups); 35712 = B * N of the coarse bench step.
CE_SHAPES = [(R_, V) for R_ in (1, 3, 4097) for V in (1, 63, 64, 1025, 1088, 1089, 2049)] + [(35712, 1025), (35712, 1089)]


def _ce_inputs(R_, V, seed):
    g = _gen(seed)
    ld = (V + 8) // 8 * 8                                        # > V (a NaN pad the kernels must never read), ld % 4 == 0
    x = torch.randn(R_, V, generator=g)
    kind = torch.arange(R_) % 5
    x[kind == 1] *= 30                                           # wide rows: lse far from the maximum's neighbours
    dom = (kind == 2).nonzero().flatten()
    x[dom, torch.randint(0, V, (len(dom),), generator=g)] += 80  # one dominant logit: softmax ~ one-hot
    eq = (kind == 3).nonzero().flatten()
    x[eq] = torch.rand(len(eq), 1, generator=g) * 4 - 2          # all-equal rows: softmax = 1 / V
    logits = torch.full((R_, ld), NAN)
    logits[:, :V] = x
    labels = torch.randint(0, V, (R_,), generator=g, dtype=torch.int32)
    r = torch.arange(R_)
    labels[r % 11 == 3] = 0
    labels[r % 11 == 5] = V - 1
    labels[r % 7 == 6] = -1                                      # ignore_index rows
    if R_ >= 4 and V > 1:
        labels[dom[:len(dom) // 2]] = x[dom[:len(dom) // 2]].argmax(1).int()      # label on the dominant logit (loss ~ 0)
    return x, logits, labels


@pytest.mark.parametrize("R_,V", CE_SHAPES)
def test_cross_entropy_routes_against_fp64(ops, dev, R_, V):
    x, logits, labels = _ce_inputs(R_, V, seed=R_ * 31 + V)
    lg, lb = logits.to(dev), labels.to(dev)
    lse = torch.full((R_,), NAN, device=dev)
    nll = torch.tensor([1.5], device=dev)                        # nll_sum ACCUMULATES onto what is there
    ops.ce_fwd(lg, lb, lse, nll, V)
    x64 = x.double()
    lse_ref = torch.logsumexp(x64, 1)
    lse_got = lse.cpu().double()
    e_lse = float(((lse_got - lse_ref).abs() / lse_ref.abs().clamp(min=1.0)).max())
    live = labels >= 0
    own = x64.gather(1, labels.clamp(min=0).long()[:, None])[:, 0]
    nll_ref = 1.5 + float((lse_ref - own)[live].sum())
    e_nll = abs(float(nll) - nll_ref) / abs(nll_ref)
    # backward: every route of the launcher.  The reference takes the kernel's own row_lse (an input of ce_bwd, checked above), so
    # this check sees the backward alone: dl = coef * g * (exp(l - lse) - onehot)
    p64 = torch.exp(x64 - lse_got[:, None])
    p64[torch.arange(R_)[live], labels[live].long()] -= 1.0
    p64[~live] = 0.0
    ldw = ((V + 8) // 8) * 8                                     # ldd % 8 == 0 + 16-byte aligned buffers: the 16-bit wave kernel
    ldo = V + 3 if (V + 3) % 8 else V + 5                        # ldd % 8 != 0: the element-wise fallback
    gdev = torch.tensor([0.25], device=dev)
    variants = [("fp32", torch.float32, ldw, 0, None, 3.0), ("fp32_gs", torch.float32, ldo, 0, gdev, 0.7)]
    for dt, nm in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        variants += [(f"{nm}_wave", dt, ldw, 0, gdev, 3.0), (f"{nm}_wave_nogs", dt, ldw, 0, None, 0.7),
                     (f"{nm}_odd_ldd", dt, ldo, 0, gdev, 0.7), (f"{nm}_offset", dt, ldw, 1, None, 3.0)]
    errs = {}
    for name, dt, ldd, off, gs, coef in variants:
        gtot = coef * (0.25 if gs is not None else 1.0)
        buf = torch.full((R_ * ldd + 8,), NAN, dtype=dt, device=dev)
        dl = buf[off:off + R_ * ldd].view(R_, ldd)               # off = 1: a 2- or 4-byte misaligned view -> the fallback kernel
        ops.ce_bwd(lg, lb, lse, gs, coef, dl, V)
        got = dl.cpu()
        assert bool((got[:, V:] == 0).all()), name               # pad columns [V, ldd) written as exact zeros
        assert bool((got[~live] == 0).all()), name               # ignored rows: exact zeros
        if off:
            assert bool(torch.isnan(buf[:off].cpu()).all()) and bool(torch.isnan(buf[off + R_ * ldd:].cpu()).all()), name
        ref = gtot * p64
        d = (got[:, :V].double() - ref).abs()
        if dt == torch.float32:
            errs[name] = float(d.max()) / gtot                  # |err| / |g|
        else:
            errs[name] = float((d / (_ulp(ref, dt) + 1e-5 * gtot)).max())     # |err| / (1 ulp at |ref| + 1e-5 |g|)
    # the one-off all-ignored batch: nothing is added, every gradient is zero
    if R_ == 3:
        lb_none = torch.full((R_,), -1, dtype=torch.int32, device=dev)
        nll2 = torch.tensor([2.25], device=dev)
        ops.ce_fwd(lg, lb_none, lse, nll2, V)
        dl = torch.full((R_, ldw), NAN, dtype=torch.bfloat16, device=dev)
        ops.ce_bwd(lg, lb_none, lse, gdev, 3.0, dl, V)
        assert float(nll2) == 2.25 and bool((dl == 0).all())
    report(f"ce[{R_}x{V}]", lse_rel=e_lse, nll_rel=e_nll, **{f"bwd_{k}": v for k, v in errs.items()})
    for name, e in errs.items():
        # fp32: one __expf per element, stored once: measured <= 1.0e-7 |g|, bar 1e-6 |g|.  16-bit: the store rounds once (RNE): measured
        # <= 0.5 of (1 ulp at |ref| + 1e-5 |g|), bar 1
        assert e <= (1e-6 if name.startswith("fp32") else 1.0), (name, e)
    assert e_lse <= 1e-6, e_lse                                  # __expf / __logf + an fp32 sum of <= 2049 terms: measured <= 1.7e-7
    assert e_nll <= 1e-5, e_nll                                  # fp32 per-row terms + float atomics over <= 35712 rows: measured <= 3.2e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. token gather: 4 sequences, B * N = 18630 rows (> the 16384-workgroup cap: a second trip), D up to 1280 (> 256 float4 per row)
@pytest.mark.parametrize("D", [64, 1024, 1280])
@pytest.mark.parametrize("with_pos", [False, True])
def test_embed_gather_wide(ops, dev, D, with_pos):
    g = _gen(D + 7 * with_pos)
    B, lens, rows = 6, [700, 1, 800, 1600], [40, 17, 33, 25]
    N = sum(l + 1 for l in lens)
    assert B * N > 16384
    seg = torch.cat([torch.full((l + 1,), s, dtype=torch.int32) for s, l in enumerate(lens)])
    posidx = torch.cat([torch.arange(l + 1, dtype=torch.int32) for l in lens])
    ids = torch.empty(B, N, dtype=torch.int32)
    o = 0
    for s, l in enumerate(lens):
        ids[:, o] = -2                                           # start token
        ids[:, o + 1:o + 1 + l] = torch.randint(0, rows[s], (B, l), generator=g, dtype=torch.int32)
        o += l + 1
    ids[torch.rand(B, N, generator=g) < 0.05] = -1               # pads (start tokens included: a pad there is a pad)
    ids[:, 0] = -2
    tables = [torch.randn(r, D, generator=g) for r in rows]
    starts = [torch.randn(D, generator=g) for _ in rows]
    pos = [torch.randn(l + 1, D, generator=g) for l in lens] if with_pos else None
    out = torch.full((B, N, D), NAN, device=dev)
    to = lambda ts: [t.to(dev) for t in ts] if ts is not None else None
    ids_d, seg_d, pos_d = ids.to(dev), seg.to(dev), posidx.to(dev)
    ops.embed_fwd(ids_d, seg_d, pos_d, to(tables), to(starts), to(pos), out)
    ref = torch.zeros(B, N, D)
    for s in range(len(lens)):
        cols = (seg == s).nonzero().flatten()
        i = ids[:, cols].long()
        blk = torch.zeros(B, len(cols), D)
        blk[i >= 0] = tables[s][i[i >= 0]]
        blk[i == -2] = starts[s]
        if with_pos:
            pr = pos[s][posidx[cols].long()].expand(B, -1, -1)
            blk = torch.where((i != -2)[..., None], blk + pr, blk)          # pads and ids get their position row, start tokens do not
        ref[:, cols] = blk
    assert torch.equal(out.cpu(), ref)                          # a copy plus one fp32 add: the same bits as the fp32 restatement
    dx = torch.randn(B, N, D, generator=g)
    dt = [torch.zeros(r, D, device=dev) for r in rows]
    dsr = [torch.zeros(D, device=dev) for _ in rows]
    dp = [torch.zeros(l + 1, D, device=dev) for l in lens] if with_pos else None
    ops.embed_bwd(ids_d, seg_d, pos_d, dt, dsr, dp, dx.to(dev), 0.1)
    e = 0.0
    for s in range(len(lens)):
        cols = (seg == s).nonzero().flatten()
        i = ids[:, cols].reshape(-1).long()
        gx = 0.1 * dx[:, cols].reshape(-1, D).double()
        rt = torch.zeros(rows[s], D, dtype=torch.float64).index_add_(0, i[i >= 0], gx[i >= 0])
        rs = gx[i == -2].sum(0)
        e = max(e, relerr(dt[s].cpu(), rt), relerr(dsr[s].cpu(), rs))
        if with_pos:
            pi = posidx[cols].long().repeat(B)
            rp = torch.zeros(lens[s] + 1, D, dtype=torch.float64).index_add_(0, pi[i != -2], gx[i != -2])
            e = max(e, relerr(dp[s].cpu(), rp))
    report(f"embed_wide[D={D},pos={with_pos}]", bwd=e)
    assert e <= 1e-5, e                                          # fp32 atomics, <= ~700 adds per row: measured <= 9.1e-7


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. sampler: V = 1088 is the widest row of sample_kernel<17>; 1089 and 2048 take <32>
SAMPLER_V = [1, 64, 65, 1025, 1088, 1089, 2048]


def _check_ids(got, logits, u, k, T, forbid):
    """Exact ids, except rows where the reference's best two scores are within 1e-5 relative (fp32 logf may order those either way:
    there the id must be one of the two).  Returns the number of such rows."""
    sc = R.gumbel_scores(logits, u, k, T, forbid)
    want = sc.argmax(1)
    near, i0, i1 = R.near_tie_rows(sc)
    bad = (got != want) & ~(near & ((got == i0) | (got == i1)))
    assert not bool(bad.any()), (k, T, forbid, bad.nonzero().flatten().tolist()[:5], got[bad][:5], want[bad][:5])
    return int(near.sum())


@pytest.mark.parametrize("V", SAMPLER_V)
def test_sampler_random_rows_against_fp64(ops, dev, V):
    g = _gen(V)
    B, ld = 40, V + 5
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
    report(f"sampler_random[V={V}]", rows=rows, near_tie_rows=near)
    assert near < 0.01 * rows, (near, rows)


def _probe_rows(V, k, exact, g, nrows=8):
    """Integer logits in 0..5 with heavy ties at the k-th value.  exact: exactly k entries are 5 (the descent can stop on a threshold
    that cuts exactly k keys); else k // 2 entries are 5 and the k-th value (4) is shared by ~V / 5 entries.  Even rows put u = 1 - 2^-24
    (Gumbel term ~ +16.6; every other u is in [0.01, 0.99], so at most +4.6) on the LAST kept entry of the k-th value, odd rows on the
    FIRST dropped entry at or below it: the kept set decides the id."""
    x = torch.randint(0, 5, (nrows, V), generator=g).float()
    n5 = k if exact else k // 2
    for r in range(nrows):
        x[r, torch.randperm(V, generator=g)[:n5]] = 5.0
    u = 0.01 + 0.98 * torch.rand(nrows, V, generator=g)
    keep = R.kept_mask(x, k, False)
    probes = []
    for r in range(nrows):
        kth = float(x[r].sort(descending=True).values[k - 1])
        kept_eq = (keep[r] & (x[r] == kth)).nonzero().flatten()
        if r % 2 == 0:
            p = int(kept_eq[-1])
        else:
            below = kth if not exact else float(x[r][x[r] < kth].max())
            p = int((~keep[r] & (x[r] == below)).nonzero().flatten()[0])
        u[r, p] = 1.0 - 2.0 ** -24
        probes.append(p)
    return x, u, torch.tensor(probes)


@pytest.mark.parametrize("V", [1025, 2048])
@pytest.mark.parametrize("exact", [False, True])
def test_sampler_kept_set_probes(ops, dev, V, exact):
    g = _gen(V + exact)
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
    report(f"sampler_probes[V={V},exact={exact}]", exact=True)


@pytest.mark.parametrize("V", [1025, 2048])
def test_sampler_at_and_embed_at(ops, dev, V):
    from open_musiclm_amd.hip import call, ptr, stream_ptr
    g = _gen(V + 3)
    B, steps, D, ld = 6, 5, 128, V + 7
    k, T = max(int(0.1 * V), 1), 0.95
    x = torch.randn(B, V, generator=g) * 4
    logits = torch.full((B, ld), NAN)
    logits[:, :V] = x
    U = torch.rand(steps, B, V, generator=g)
    lg, Ud = logits.to(dev), U.to(dev)
    step_dev = torch.tensor([3], dtype=torch.int32, device=dev)
    plain = torch.empty(B, dtype=torch.long, device=dev)
    ops.sample_topk_gumbel(lg, Ud[3].contiguous(), plain, V, k, T, True)
    _check_ids(plain.cpu(), x, U[3], k, T, True)
    out = torch.full((B,), -7, dtype=torch.long, device=dev)
    hist = torch.full((steps, B), -7, dtype=torch.long, device=dev)
    call("omlm_sample_topk_gumbel_at", ptr(lg), ptr(Ud), ptr(step_dev), ptr(out), ptr(hist), B, V, ld, k, T, 1, stream_ptr())
    h = hist.cpu()
    assert torch.equal(out, plain) and torch.equal(h[3], plain.cpu())
    assert bool((h[torch.arange(steps) != 3] == -7).all())                 # only slot 3 written
    E = 2 * V
    emb = torch.randn(E, D, generator=g).to(dev)
    for offset in (7, -V, E - V // 2):                                      # inside; every row clamped to 0; upper rows clamped to E - 1
        out.fill_(-7)
        hist.fill_(-7)
        xo = torch.full((B, D), NAN, device=dev)
        call("omlm_sample_embed_at", ptr(lg), ptr(Ud), ptr(step_dev), ptr(out), ptr(hist), B, V, ld, k, T, 1,
             ptr(emb), offset, E, ptr(xo), D, stream_ptr())
        assert torch.equal(out, plain) and torch.equal(hist[3], plain)
        r = (plain + offset).clamp(0, E - 1)
        assert torch.equal(xo, emb[r])                                      # a copy of the clamped row: bit-equal
    report(f"sampler_at_embed_at[V={V}]", exact=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. optimizer kernels
BIG = 4 * 4096 * 256 * 2 + 5                                   # two trips of the 4096-workgroup grid plus a scalar tail
ADAMW_CASES = [
    # n, scalar path (base pointers one element off), p16 dtype, decoupled (AdamW) or Adam + L2
    (1, False, torch.bfloat16, True), (1, True, torch.float16, False), (3, False, torch.float16, False), (3, True, None, True),
    (4, False, torch.bfloat16, False), (4, True, torch.bfloat16, True), (10007, False, torch.float16, True),
    (10007, True, torch.bfloat16, False), (10007, False, None, False), (10007, True, torch.float16, True),
    (BIG, False, torch.bfloat16, True), (BIG, True, torch.float16, False),
]


def _flat_bufs(n, scalar, dev, p16_dtype, vals):
    """p, g, m, v (+ p16) of n elements; scalar: every base pointer one element past an aligned one (forces the element path), with
    guard elements on both sides that must stay untouched."""
    off = 1 if scalar else 0
    out = []
    for t in vals:
        b = torch.full((n + 2 * 4,), 12345.0, device=dev)
        b[4 - off + 0:4 - off + n] = t.to(dev) if t is not None else 0.0
        out.append((b, b[4 - off:4 - off + n]))
    p16 = None
    if p16_dtype is not None:
        b16 = torch.full((n + 8,), 7.0, dtype=p16_dtype, device=dev)
        p16 = (b16, b16[4 - off:4 - off + n])
    return out, p16


def _guards_ok(bufs, n, off):
    for b, _ in bufs:
        c = b.cpu()
        if not (bool((c[:4 - off] == c[:4 - off][0]).all()) and bool((c[4 - off + n:] == c[4 - off + n:][0]).all())):
            return False
    return True


def _grads(n, g, norms, gscale=0.5):
    """3 steps of raw gradients whose gscale-scaled norms are `norms` (max_norm 1: step 2 clips, steps 1 and 3 do not)."""
    out = []
    for target in norms:
        x = torch.randn(n, generator=g) + 0.1
        out.append(x * (target / (gscale * float(x.double().norm()))))
    return out


@pytest.mark.parametrize("n,scalar,p16_dtype,decoupled", ADAMW_CASES)
def test_adamw_paths_against_torch(ops, dev, n, scalar, p16_dtype, decoupled):
    g = _gen(n + 2 * scalar + int(decoupled))
    p0 = torch.randn(n, generator=g)
    ref_p = torch.nn.Parameter(p0.clone().double())
    # the reference runs on the fp32 values the kernel receives: with beta2 = 0.99 exactly, 1 - beta2 differs from the kernel's
    # 1 - (float)0.99 by 9.5e-7 relative, which alone moves v by that much (measured 8e-7 .. 1.7e-6 against exact betas)
    kw = dict(lr=_f32(3e-3), betas=(_f32(0.9), _f32(0.99)), eps=_f32(1e-8), weight_decay=_f32(0.01))
    opt = torch.optim.AdamW([ref_p], **kw) if decoupled else torch.optim.Adam([ref_p], **kw)
    bufs, p16 = _flat_bufs(n, scalar, dev, p16_dtype, [p0, None, None, None])
    (_, P), (_, G), (_, M), (_, V) = bufs
    off = 1 if scalar else 0
    nsq = torch.zeros(1, device=dev)
    for step, grad in enumerate(_grads(n, g, (0.3, 10.0, 0.5)), start=1):
        ref_p.grad = grad.double() * 0.5
        torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
        opt.step()
        G.copy_(grad.to(dev))
        nsq.zero_()
        ops.sumsq_accumulate(G.clone(), nsq)
        ops.adamw_clip_step(P, G, M, V, p16[1] if p16 else None, lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, step=step,
                            gscale=0.5, gnorm_sq=nsq, max_norm=1.0, decoupled=decoupled, zero_grad=True)
        assert float(G.abs().max()) == 0.0                      # zero_grad in the same pass
        if p16:
            assert torch.equal(p16[1].view(torch.int16), P.to(p16_dtype).view(torch.int16))     # RNE cast of the kernel's own p
    st = opt.state[ref_p]
    e = dict(p=relerr(P.cpu(), ref_p.detach()), m=relerr(M.cpu(), st["exp_avg"]), v=relerr(V.cpu(), st["exp_avg_sq"]))
    assert _guards_ok(bufs, n, off)
    if p16:
        c = p16[0].cpu().float()
        assert bool((c[:4 - off] == 7.0).all()) and bool((c[4 - off + n:] == 7.0).all())
    report(f"adamw[n={n},scalar={scalar},p16={p16_dtype},decoupled={decoupled}]", **e)
    assert max(e.values()) <= 1e-6, e                           # fp32 update against fp64 (the existing AdamW bar): measured <= 4.6e-7


@pytest.mark.parametrize("scalar", [False, True])
def test_adamw_loss_scale_state(ops, dev, scalar):
    """ls_state {S, good, skipped, applied, S}: gradients carry S, the bias corrections follow applied + 1 (not the host's step)."""
    n, S = 4099, 1024.0
    g = _gen(40 + scalar)
    p0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    v0 = torch.rand(n, generator=g) * 1e-6
    grad = _grads(n, g, (3.0,))[0]                               # scaled norm 3 > max_norm 1: clipping active
    ref_p = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.AdamW([ref_p], lr=_f32(3e-3), betas=(_f32(0.9), _f32(0.99)), eps=_f32(1e-8), weight_decay=_f32(0.01))
    opt.state[ref_p] = dict(step=torch.tensor(5.0), exp_avg=m0.double().clone(), exp_avg_sq=v0.double().clone())
    ref_p.grad = grad.double() * 0.5
    torch.nn.utils.clip_grad_norm_([ref_p], 1.0)
    opt.step()                                                   # Adam step 6 = applied + 1
    bufs, p16 = _flat_bufs(n, scalar, dev, torch.float16, [p0, grad * S, m0, v0])
    (_, P), (_, G), (_, M), (_, V) = bufs
    ls = torch.tensor([S, 1.0, 2.0, 5.0, S], device=dev)
    nsq = torch.zeros(1, device=dev)
    ops.sumsq_accumulate(G.clone(), nsq)
    ops.adamw_clip_step(P, G, M, V, p16[1], lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, step=9, gscale=0.5, gnorm_sq=nsq,
                        max_norm=1.0, decoupled=True, zero_grad=True, ls_state=ls)
    st = opt.state[ref_p]
    e = dict(p=relerr(P.cpu(), ref_p.detach()), m=relerr(M.cpu(), st["exp_avg"]), v=relerr(V.cpu(), st["exp_avg_sq"]))
    assert float(G.abs().max()) == 0.0 and torch.equal(p16[1].view(torch.int16), P.to(torch.float16).view(torch.int16))
    assert ls.cpu().tolist() == [S, 1.0, 2.0, 5.0, S]            # the step reads the state; only loss_scale_update writes it
    # an overflowed step (norm inf or nan): p, m, v and p16 bit-unchanged, g still cleared
    for bad in (INF, NAN):
        before = [t.clone() for t in (P, M, V, p16[1])]
        G.copy_((grad * S).to(dev))
        nsq.fill_(bad)
        ops.adamw_clip_step(P, G, M, V, p16[1], lr=3e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, step=10, gscale=0.5, gnorm_sq=nsq,
                            max_norm=1.0, decoupled=True, zero_grad=True, ls_state=ls)
        assert all(torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a.view(torch.int32),
                               b.view(torch.int16) if b.dtype == torch.float16 else b.view(torch.int32))
                   for a, b in zip(before, (P, M, V, p16[1]))), bad
        assert float(G.abs().max()) == 0.0
    assert _guards_ok(bufs, n, 1 if scalar else 0)
    report(f"adamw_ls_state[scalar={scalar}]", **e)
    assert max(e.values()) <= 1e-6, e                           # same update as without the state (S is a power of two): measured <= 1e-7


def test_loss_scale_update_state_machine(ops, dev):
    """GradScaler's rule with interval 3 through both clamps; the 5 floats (powers of two and counts) must match exactly."""
    growth, backoff, interval, smin, smax = 2.0, 0.5, 3, 1.0, 8.0
    ls = torch.tensor([4.0, 0.0, 0.0, 0.0, 4.0], device=dev)
    st = ls.cpu().tolist()
    nsq = torch.zeros(1, device=dev)
    seq = [INF, NAN, INF] + [1.0] * 12 + [3.2e38] + [1.0, 1.0, NAN] + [1.0] * 3      # 3.2e38: finite, but past the overflow guard
    trace = []
    for gn in seq:
        nsq.fill_(gn)
        ops.loss_scale_update(ls, nsq, growth=growth, backoff=backoff, interval=interval, scale_min=smin, scale_max=smax)
        st = R.loss_scale_update(st, gn < 3.0e38, growth, backoff, interval, smin, smax)
        got = ls.cpu().tolist()
        trace.append(got[0])
        assert got == st, (gn, got, st)
    assert min(trace) == smin and max(trace) == smax            # both clamps were reached
    report("loss_scale_update", steps=len(seq), exact=True)


@pytest.mark.parametrize("n", [1, 3, 5, 2048 * 1024 + 7, 2048 * 1024 * 3 + 1])
def test_sumsq_forms(ops, dev, n):
    g = _gen(n)
    x = torch.randn(n, generator=g) * 3
    ref = 0.75 + float((x.double() ** 2).sum())
    X = x.to(dev)
    a = torch.tensor([0.75], device=dev)
    ops.sumsq_accumulate(X, a)
    parts = torch.empty(2048, device=dev)
    det = []
    for _ in range(3):
        o = torch.tensor([0.75], device=dev)
        ops.sumsq_accumulate(X, o, parts)
        det.append(o.cpu())
    assert all(torch.equal(det[0].view(torch.int32), d.view(torch.int32)) for d in det)   # fixed order: bit-identical launches
    e = dict(atomic=abs(float(a) - ref) / ref, partials=abs(float(det[0]) - ref) / ref)
    report(f"sumsq[n={n}]", **e)
    # fixed order: fp32 per-workgroup sums, then one fp32 pass over <= 2048 partials: measured <= 5.7e-8 (the same bits every run)
    assert e["partials"] <= 5e-7, e
    # float atomics: up to 2048 partials added onto one word in arrival order.  Each add rounds by up to half an ulp of the running sum
    # (2^-24 of it), so the error is a random walk of ~sqrt(2048) such steps: sigma ~ 1e-6 relative.  Measured 1.5e-7 .. 1.0e-6 over runs
    # (so a 1e-6 bar fails on some orders); bar 5e-6
    assert e["atomic"] <= 5e-6, e


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. FusedAdam against torch.optim, grouped the reference's way (optimizer.py:10-34, restated here: ndim < 2 -> no decay; wd == 0 -> Adam)
def _torch_opt(params, lr, wd):
    kw = dict(lr=lr, betas=(0.9, 0.99), eps=1e-8)
    if wd == 0:
        return torch.optim.Adam(params, **kw)
    groups = [{"params": [p for p in params if p.ndim >= 2]}, {"params": [p for p in params if p.ndim < 2], "weight_decay": 0}]
    return torch.optim.AdamW(groups, weight_decay=wd, **kw)


@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_fused_adam_matches_torch_optim(dev, wd):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.optimizer import get_optimizer, get_linear_scheduler
    torch.manual_seed(0)
    model = M.create_semantic_transformer(dim=128, depth=2, heads=2, attn_dropout=0.0, ff_dropout=0.0).to(dev)
    params = list(model.parameters())
    refs = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in params]
    lr, g = 1e-3, _gen(77)
    opt = get_optimizer(params, lr=lr, wd=wd)
    ref = _torch_opt(refs, lr, wd)
    sched = get_linear_scheduler(opt, total_iters=10, start_factor=0.1)
    rsched = torch.optim.lr_scheduler.LinearLR(ref, start_factor=0.1, end_factor=1.0, total_iters=10)
    scales = [10.0 ** (i % 5 - 3) for i in range(len(params))]          # mixed scales: 1e-3 .. 10 across parameters

    def step(o, mult):
        o.zero_grad()
        for p, r, s in zip(params, refs, scales):
            gr = torch.randn(p.shape, generator=g) * s * mult
            p.grad.copy_(gr.to(dev))
            r.grad = gr.double() * 0.5
        o.step(max_grad_norm=1.0, grad_scale=0.5)
        torch.nn.utils.clip_grad_norm_(refs, 1.0)
        ref.step()

    def check(tag):
        e = max(relerr(p.detach().cpu(), r.detach()) for p, r in zip(params, refs))
        for p in params:
            assert torch.equal(p._omlm_bf16.view(torch.int16), p.detach().to(p._omlm_bf16.dtype).view(torch.int16)), tag
        return e

    for mult in (1.0, 1e-4, 3.0):                                # clipping active, inactive, active
        step(opt, mult)
        sched.step()
        rsched.step()
    e3 = check("3 steps")
    sd = opt.state_dict()
    opt2 = get_optimizer(params, lr=lr, wd=wd)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
    step(opt2, 1.0)
    e4 = check("after load_state_dict")
    report(f"fused_adam[wd={wd}]", relerr_3_steps=e3, relerr_after_reload=e4)
    assert e3 <= 1e-6 and e4 <= 1e-6, (e3, e4)                  # fp32 masters against fp64 torch.optim: measured <= 2.9e-7
