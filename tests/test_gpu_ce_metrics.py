"""GPU: per-quantizer loss, accuracy, label rank and entropy (csrc/ce_metrics.hip, metrics.QuantizerMetrics) -- the two kernels against the
fp64 restatement (tests/ce_metrics_ref.py) on both routes, the bins' order, the wrapper's return_metrics on both preparation routes and the
trainer's logs.  Every bar sits next to its check with its reason; measured errors go to the kernel report."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_metrics_ref as MR
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_loss_optim_sampler import _ce_inputs
from test_gpu_model import build_from_golden

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")

# Worst values measured on an MI355X over every case of test_kernel_against_the_restatement (profiles/ce_metrics.md), and the bars: 4x the
# measurement rounded up to one digit (the convention of test_gpu_ce_reg.py; headroom for another machine of the pool).
#   entropy      max |H - H_ref| over live rows, nats (H <= log V <= 9.1)
#   bin_nll      max over bins |sum - ref| / max(sum over the bin's rows of max(|lse|, 1), 1): the fp64 sum of the kernel's fp32 rows against
#                the restatement's, in the units of the per-row bar (a row's nll carries the rounding of its lse)
#   bin_entropy  max over bins |sum - ref| / max(|ref|, 1) for the entropy sums
MEASURED = dict(entropy=1.5e-6, bin_nll=1.2e-7, bin_entropy=1.7e-7)
BAR = dict(entropy=6e-6, bin_nll=5e-7, bin_entropy=7e-7)


def _pad8(V):
    return (V + 7) // 8 * 8


def _inputs(R, V, kind, seed):
    """x fp32 [R, V], the logits buffer [R, ld] (ld = V rounded up to 8, pad columns NaN) and int32 labels.  kind "ce": the generator of
    the plain cross-entropy test; "ties": integers in [-3, 3], rows full of exact ties with the label.  Some labels -1; from R = 5 a row
    with a common offset of 1e4 and a row with -inf columns (label on a finite one); at R = 257 a second such row with the label ON a
    -inf column (nll = +inf, the rank still exact)."""
    x, _, labels = _ce_inputs(R, V, seed)
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "ties":
        x = (torch.randn(R, V, generator=g) * 1.5).round().clamp(-3, 3)
        first = torch.argmax(x, 1).int()
        last = (V - 1 - torch.argmax(x.flip(1), 1)).int()
        labels[0::4] = first[0::4]
        labels[2::8] = last[2::8]
    if R >= 3:
        labels[2] = -1
    if R >= 5:
        x[0] += 1e4
        x[4, ::3] = -INF
        labels[4] = 1 if V > 1 else 0                              # column 1 is finite
    if R >= 257:
        x[9, ::3] = -INF
        labels[9] = 0                                              # on a -inf column
    ld = _pad8(V)
    logits = torch.full((R, ld), NAN)
    logits[:, :V] = x
    return x, logits, labels


def _guarded(R, dtype, fill, dev):
    """An [R] output inside a larger buffer: (buffer, view)."""
    buf = torch.full((R + 16,), fill, dtype=dtype, device=dev)
    return buf, buf[8:8 + R]


KERNEL_SHAPES = [(R, V) for V in (2, 63, 64, 65, 1025, 1088, 1089, 2049, 8193) for R in (1, 3, 5, 257)] + \
                [(4099, 65), (4099, 1089)]                         # one row past a full trip of either grid (1024 x 4 rows, 4096 workgroups)


@pytest.mark.parametrize("kind", ["ce", "ties"])
@pytest.mark.parametrize("R,V", KERNEL_SHAPES)
def test_kernel_against_the_restatement(ops, dev, R, V, kind):
    x, logits, labels = _inputs(R, V, kind, seed=R * 31 + V)
    lg, lb = logits.to(dev), labels.to(dev)
    nbuf, nll = _guarded(R, torch.float32, NAN, dev)
    rbuf, rank = _guarded(R, torch.int32, -7777, dev)
    ebuf, ent = _guarded(R, torch.float32, NAN, dev)
    ops.ce_metrics(lg, lb, V, row_nll=nll, row_rank=rank, row_entropy=ent)
    for buf, fill in ((nbuf, None), (rbuf, -7777), (ebuf, None)):                 # nothing written around the outputs
        edge = torch.cat((buf[:8], buf[8 + R:])).cpu()
        assert bool(torch.isnan(edge).all()) if fill is None else bool((edge == fill).all())
    lse = torch.full((R,), NAN, device=dev)
    ops.ce_fwd(lg, lb, lse, torch.zeros(1, device=dev), V)                        # the existing forward on the same buffer
    nll_ref, rank_ref, ent_ref = MR.rows(x.double().numpy(), labels.numpy())
    got_nll, got_rank, got_ent = nll.cpu(), rank.cpu(), ent.cpu()
    live = (labels >= 0).numpy()
    # 1. the rank: exact, ignored rows -1
    assert np.array_equal(got_rank.numpy().astype(np.int64), rank_ref), (got_rank.numpy(), rank_ref)
    assert bool((got_nll[~torch.from_numpy(live)] == 0).all()) and bool((got_ent[~torch.from_numpy(live)] == 0).all())
    # 2. lse bit for bit the existing forward's.  Through this interface lse shows as row_nll = fl(lse - l[y]); adding l[y] back rounds a
    # second time, so fl(row_nll + l[y]) equals lse only to an ulp even where the two lse agree in every bit.  The check is therefore made
    # one step earlier, where it is exact: row_nll must equal fl(row_lse - l[y]) -- the same fp32 subtraction on the forward's own row_lse
    # -- in every bit, on every live row (the +inf of a label on a -inf column included).  No other reduction order proved necessary.
    own = x.gather(1, labels.clamp(min=0).long()[:, None])[:, 0]
    want = (lse.cpu() - own)
    lv = torch.from_numpy(live)
    assert torch.equal(got_nll[lv], want[lv]), float((got_nll[lv] - want[lv]).abs().max())
    # the issue's own form of the same comparison, on finite rows, at the plain test's lse bar
    fin = lv & torch.isfinite(got_nll)
    e_lse_form = float((((got_nll + own)[fin].double() - lse.cpu()[fin].double()).abs() / lse.cpu()[fin].double().abs().clamp(min=1.0)).max()) if fin.any() else 0.0
    assert e_lse_form <= 1e-6, e_lse_form
    # 3. row_nll against fp64: the plain test's bar on lse (1e-6 of max(|lse|, 1): __expf / __logf + an fp32 sum), nll being lse - l[y]
    lse_ref = torch.logsumexp(x.double(), 1).numpy()
    f = fin.numpy()
    e_nll = float((np.abs(got_nll.double().numpy()[f] - nll_ref[f]) / np.maximum(np.abs(lse_ref[f]), 1.0)).max()) if f.any() else 0.0
    assert np.array_equal(np.isinf(got_nll.numpy())[live], np.isinf(nll_ref)[live])
    # 4. the entropy, absolute (nats)
    e_ent = float(np.abs(got_ent.double().numpy() - ent_ref)[live].max()) if live.any() else 0.0
    assert bool(torch.isfinite(got_ent).all())                                    # a -inf column adds exactly 0, never 0 * inf
    # 5. the bins of these rows: n = R (one sample), Q = 3
    Q, k_top = 3, ops.default_metrics_top_k(V)
    bins = torch.zeros(Q + 1, 5, dtype=torch.float64, device=dev)
    ops.ce_metrics_bins(nll, rank, ent, lb, R, Q, V, k_top, bins)
    b_ref = MR.bins(nll_ref, rank_ref, ent_ref, labels.numpy(), R, Q, V, k_top)
    b = bins.cpu().numpy()
    assert np.array_equal(b[:, [0, 3, 4]], b_ref[:, [0, 3, 4]]), (b, b_ref)      # count, top1, topk: exact
    # the two fp64 sums in the units of their rows' bars: a row's nll carries the rounding of its lse (an offset of 1e4 costs 1e-3 absolute,
    # whatever the nll), so the nll sum of a bin is measured against the bin's sum of max(|lse|, 1); the entropy sum against max(|sum|, 1)
    scale = MR.bins(np.maximum(np.abs(lse_ref), 1.0), rank_ref, ent_ref, labels.numpy(), R, Q, V, k_top)[:, 1]
    e_bin = {}
    for name, col, den in (("bin_nll", 1, np.maximum(scale, 1.0)), ("bin_entropy", 2, np.maximum(np.abs(b_ref[:, 2]), 1.0))):
        okb = np.isfinite(b_ref[:, col])
        assert np.array_equal(b[~okb, col], b_ref[~okb, col])                      # a bin holding a +inf nll is +inf
        e_bin[name] = float((np.abs(b[okb, col] - b_ref[okb, col]) / den[okb]).max()) if okb.any() else 0.0
    # the reduce alone, from the kernel's own rows: an ordered fp64 sum of R fp32 terms, <= R 2^-53 of the sum of their magnitudes
    b_own = MR.bins(np.where(np.isfinite(got_nll.numpy()), got_nll.double().numpy(), 0.0), got_rank.numpy(), got_ent.double().numpy(),
                    labels.numpy(), R, Q, V, k_top)
    fin_rows = np.where(np.isfinite(got_nll.numpy()), 1.0, 0.0)
    if fin_rows.all():
        mag = MR.bins(np.abs(got_nll.double().numpy()), got_rank.numpy(), np.abs(got_ent.double().numpy()), labels.numpy(), R, Q, V, k_top)
        assert (np.abs(b[:, 1:3] - b_own[:, 1:3]) <= R * 2.0 ** -53 * mag[:, 1:3] + 1e-300).all()
    report(f"ce_metrics[{R}x{V},{kind}]", lse_form=e_lse_form, nll=e_nll, entropy=e_ent, **e_bin)
    print(f"ce_metrics[{R}x{V},{kind}] nll {e_nll:.3e} entropy {e_ent:.3e} bin_nll {e_bin['bin_nll']:.3e} bin_entropy {e_bin['bin_entropy']:.3e}")
    assert e_nll <= 1e-6, e_nll
    assert e_ent <= BAR["entropy"], e_ent
    assert e_bin["bin_nll"] <= BAR["bin_nll"] and e_bin["bin_entropy"] <= BAR["bin_entropy"], e_bin


@pytest.mark.parametrize("V", [65, 1089])
def test_null_outputs_and_labels_past_the_vocabulary(ops, dev, V):
    R = 6
    x, logits, labels = _inputs(R, V, "ce", seed=V)
    labels[1], labels[3] = V, V + 7                                               # past the vocabulary
    lg, lb = logits.to(dev), labels.to(dev)
    full = [torch.full((R,), NAN, device=dev), torch.full((R,), -7777, dtype=torch.int32, device=dev), torch.full((R,), NAN, device=dev)]
    ops.raise_on_index_error(dev)                                                 # clear
    ops.ce_metrics(lg, lb, V, row_nll=full[0], row_rank=full[1], row_entropy=full[2])
    with pytest.raises(IndexError, match="label"):
        ops.raise_on_index_error(dev)
    ops.raise_on_index_error(dev)                                                 # the raise cleared the flag
    assert full[0][[1, 3]].tolist() == [0, 0] and full[1][[1, 3]].tolist() == [-1, -1] and full[2][[1, 3]].tolist() == [0, 0]
    bins = torch.zeros(3, 5, dtype=torch.float64, device=dev)
    ops.ce_metrics_bins(full[0], full[1], full[2], lb, R, 2, V, 1, bins)
    assert float(bins[:, 0].sum()) == float(((labels >= 0) & (labels < V)).sum()) == 3     # rows 1, 3 (past V) and 2 (ignored) enter no bin
    # a null output pointer skips that output only
    for keep in range(3):
        outs = [torch.full((R,), NAN, device=dev), torch.full((R,), -7777, dtype=torch.int32, device=dev), torch.full((R,), NAN, device=dev)]
        kw = {name: (o if i == keep else None) for i, (name, o) in enumerate(zip(("row_nll", "row_rank", "row_entropy"), outs))}
        ops.ce_metrics(lg, lb, V, **kw)
        with pytest.raises(IndexError):
            ops.raise_on_index_error(dev)
        assert torch.equal(outs[keep], full[keep])
        for i in range(3):
            if i != keep:
                assert bool(torch.isnan(outs[i]).all()) if i != 1 else bool((outs[i] == -7777).all())
    ops.ce_metrics(lg, lb, V)                                                     # all three null: the flag alone
    with pytest.raises(IndexError):
        ops.raise_on_index_error(dev)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("Q", [1, 3, 5, 8])
def test_bins(ops, dev, Q, T, B):
    n, V = T * Q + 1, 9
    R = B * n
    g = torch.Generator().manual_seed(Q * 100 + T * 10 + B)
    labels = torch.randint(0, V - 1, (R,), generator=g, dtype=torch.int32)
    labels[n - 1::n] = V - 1                                                      # the eos where a sequence ends ...
    if R > 3:
        labels[1] = V - 1                                                         # ... and where it does not: bin Q wherever it stands
        labels[2] = -1
        labels[3] = V + 2
    nll = (torch.rand(R, generator=g) * 7).float()
    ent = (torch.rand(R, generator=g) * 2).float()
    rank = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    rank[(labels < 0) | (labels >= V)] = -1
    d = [t.to(dev) for t in (nll, rank, ent, labels)]
    for k_top in (1, 3, V):                                                       # 1 and V are the edges
        ref = MR.bins(nll.double().numpy(), rank.numpy(), ent.double().numpy(), labels.numpy(), n, Q, V, k_top)
        one = torch.zeros(Q + 1, 5, dtype=torch.float64, device=dev)
        ops.ce_metrics_bins(*d, n, Q, V, k_top, one)
        again = torch.zeros(Q + 1, 5, dtype=torch.float64, device=dev)
        ops.ce_metrics_bins(*d, n, Q, V, k_top, again)
        assert torch.equal(one, again)                                            # two fresh runs: the same bits
        got = one.cpu().numpy()
        assert np.array_equal(got[:, [0, 3, 4]], ref[:, [0, 3, 4]]), (got, ref)
        assert (np.abs(got[:, 1:3] - ref[:, 1:3]) <= R * 2.0 ** -53 * np.maximum(ref[:, 1:3], 1.0)).all()      # an ordered fp64 sum of R positive terms
        if k_top == 1:
            assert np.array_equal(got[:, 4], got[:, 3])                           # rank < 1 is rank == 0
        if k_top == V:
            assert np.array_equal(got[:, 4], got[:, 0])                           # every live row has rank < V
        ops.ce_metrics_bins(*d, n, Q, V, k_top, one)                              # a second launch onto the same buffer: the sum
        assert torch.equal(one, 2 * again)
    eos_rows = int((labels == V - 1).sum())
    assert ref[Q, 0] == eos_rows and ref[:, 0].sum() == int(((labels >= 0) & (labels < V)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the wrapper
def _host_bins(logits_bcn, labels, Q, V1, k_top):
    """From returned logits [B, V1, n] and labels [B, n] on the host: per bin the count, the fp64 nll sum and the argmax hits."""
    lg = logits_bcn.detach().cpu().transpose(1, 2).double()                       # [B, n, V1]
    lab = labels.detach().cpu().long()
    B, n = lab.shape
    live = (lab >= 0)
    nll = F.cross_entropy(lg.reshape(-1, V1), lab.reshape(-1).clamp(min=0), reduction="none").reshape(B, n)
    hit = lg.argmax(-1) == lab                                                    # CPU argmax: the first maximal entry
    bin_ = torch.where(lab == V1 - 1, torch.full_like(lab, Q), (torch.arange(n) % Q)[None].expand(B, n))
    out = np.zeros((Q + 1, 3))
    for b in range(Q + 1):
        m = live & (bin_ == b)
        out[b] = (float(m.sum()), float(nll[m].sum()), float(hit[m].sum()))
    return out


def _same_loss(a, b):
    """The loss of two calls on the same inputs.  The metrics launches only read, so every row's lse and nll are the same bits (the logits are
    compared bit for bit, and test_kernel_against_the_restatement holds row_nll to the forward's own row_lse in every bit); the scalar itself
    is an fp32 atomic sum over workgroups whose order differs between any two launches, with or without the metrics -- order-free to an
    ulp: the bar test_loss_only_step_skips_zero_weight_heads holds the same sum to."""
    a, b = float(a), float(b)
    return abs(a - b) <= 2e-6 * abs(a)


def _check_against_logits(metrics, logits, labels, loss, what):
    host = metrics.bins.cpu().numpy()
    for s in metrics.weighted:
        if logits[s] is None:
            continue
        Q, V1 = metrics.quantizers[s], metrics.vocab[s]
        ref = _host_bins(logits[s], labels[s], Q, V1, metrics.k_top[s])
        got = host[s, :Q + 1]
        assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 3], ref[:, 2]), (what, s, got, ref)      # count, top1: exact
        assert (got[:, 4] >= got[:, 3]).all() and (got[:, 4] <= got[:, 0]).all()
        assert (got[:, 2] >= 0).all() and (got[:, 2] <= got[:, 0] * math.log(V1) * (1 + 1e-6)).all()                   # 0 <= H <= log V per row
        # the plain test's bar of the nll sum (1e-5 relative: fp32 per-row terms)
        assert (np.abs(got[:, 1] - ref[:, 1]) <= 1e-5 * np.maximum(np.abs(ref[:, 1]), 1.0)).all(), (what, s, got[:, 1], ref[:, 1])
        assert (host[s, Q + 1:] == 0).all()
    for s in range(len(metrics.weights)):
        if s not in metrics.weighted:
            assert (host[s] == 0).all()
    # fp32 atomics against an ordered fp64 sum: the plain test's nll-sum bar
    assert abs(metrics.loss() - float(loss)) <= 1e-5 * abs(float(loss)), (what, metrics.loss(), float(loss))


@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
@pytest.mark.parametrize("name", ["tiny_coarse", "tiny_fine_allweights"])
def test_wrapper_return_metrics(golden_dir, dev, name, precision):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.metrics import QuantizerMetrics
    z, model = build_from_golden(golden_dir, name, dev, precision)
    weights = [float(w) for w in z["loss_weights"]]
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=weights, mask_prob=0.0)
    ids = [torch.from_numpy(z[f"ids.{i}"]).to(dev) for i in range(len(model.token_sequences))]
    # eval forward, the _prepare route
    wrapper.eval()
    with torch.no_grad():
        loss0, logits0, labels0 = wrapper(all_token_ids=ids, return_loss=True)
        out = wrapper(all_token_ids=ids, return_loss=True, return_metrics=True)
    assert len(out) == 4 and isinstance(out[3], QuantizerMetrics)
    loss1, logits1, labels1, m = out
    assert _same_loss(loss0, loss1) and all(torch.equal(a, b) for a, b in zip(logits0, logits1)) and all(torch.equal(a, b) for a, b in zip(labels0, labels1))
    assert m.k_top == [ops_default(v) for v in m.vocab]
    _check_against_logits(m, logits1, labels1, loss1, f"eval {name} {precision}")
    d = m.to_dict("valid_")
    many = sum(w > 0 for w in weights) > 1
    key = (f"valid_seq{len(weights) - 1}_" if many else "valid_") + "loss_q0"
    assert key in d and d[key] is not None
    # the fused preparation route, training mode, dropouts and masks at 0
    wrapper.train()
    lossf0, logitsf0, labelsf0 = wrapper(all_token_ids=ids, return_loss=True, return_logits=False)
    lossf1, logitsf1, labelsf1, mf = wrapper(all_token_ids=ids, return_loss=True, return_logits=False, return_metrics=True)
    assert _same_loss(lossf0.detach(), lossf1.detach())
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(logitsf0, logitsf1))
    assert labelsf1[-1].dtype == torch.int32                                      # the fused route's labels: it was taken
    _check_against_logits(mf, logitsf1, labelsf1, lossf1.detach(), f"fused {name} {precision}")
    lossf1.backward()                                                             # the backward runs as ever
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    # with the forgetful mask on: the same draws with and without the metrics
    wrapper.mask_prob = 0.15
    states = []
    for kw in ({}, dict(return_metrics=True)):
        torch.manual_seed(11)
        r = wrapper(all_token_ids=ids, return_loss=True, return_logits=False, **kw)
        states.append((r[0].detach().clone(), torch.cuda.get_rng_state(dev)))
    assert _same_loss(states[0][0], states[1][0]), (float(states[0][0]), float(states[1][0]))
    assert torch.equal(states[0][1], states[1][1])                                # the generator stands where it stood


def ops_default(V):
    from open_musiclm_amd import ops as o
    return o.default_metrics_top_k(V)


def test_accumulating_onto_a_given_object_doubles_it(golden_dir, dev):
    from open_musiclm_amd import open_musiclm as M
    z, model = build_from_golden(golden_dir, "tiny_coarse", dev, "bf16x3")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0).eval()
    ids = [torch.from_numpy(z[f"ids.{i}"]).to(dev) for i in range(3)]
    m = wrapper.new_metrics(top_k=7)
    assert m.k_top[-1] == 7
    with torch.no_grad():
        r1 = wrapper(all_token_ids=ids, return_loss=True, return_metrics=m)
        once = m.bins.clone()
        r2 = wrapper(all_token_ids=ids, return_loss=True, return_metrics=m)
    assert r1[3] is m and r2[3] is m and torch.equal(m.bins, 2 * once) and float(once[2, :, 0].sum()) == 2 * 16
    d = m.to_dict()
    assert "top7_accuracy_q0" in d and d["count_total"] == 64.0
    other = m.like().add_(m)
    assert torch.equal(other.bins, m.bins) and float(m.zero_().bins.abs().sum()) == 0


def test_unique_consecutive_sequence(dev):
    """The padded labels of a unique_consecutive sequence are ignored rows: they enter no bin, as they leave the loss's normaliser."""
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    seqs = [M.TokenSequenceInfo(32, 2, False), M.TokenSequenceInfo(32, 1, True)]
    model = M.TokenConditionedTransformer(token_sequences=seqs, dim=64, depth=2, heads=2, ff_dropout=0.0, precision="bf16x3").to(dev)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=True, cross_entropy_loss_weights=[0.5, 1.0], mask_prob=0.0)
    wrapper.eval()
    g = torch.Generator().manual_seed(2)
    a = torch.randint(0, 32, (3, 4, 2), generator=g).to(dev)
    b = torch.randint(0, 4, (3, 12), generator=g).to(dev)
    with torch.no_grad():
        loss0, logits0, _ = wrapper(all_token_ids=[a, b], return_loss=True)
        loss, logits, labels, m = wrapper(all_token_ids=[a, b], return_loss=True, return_metrics=True)
    assert _same_loss(loss0, loss) and all(torch.equal(x, y) for x, y in zip(logits0, logits))
    padded = int((labels[1] == -1).sum())
    assert padded > 0
    host = m.bins.cpu()
    assert float(host[1, :2, 0].sum()) == labels[1].numel() - padded and float(host[0, :3, 0].sum()) == labels[0].numel()
    _check_against_logits(m, logits, labels, loss, "unique_consecutive")
    d = m.to_dict()
    assert "seq0_loss_q1" in d and "seq1_loss_q0" in d and "seq1_loss_eos" in d


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
def _trainer(dev, folder, **kw):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.data import SyntheticTokenDataset
    from open_musiclm_amd.trainer import SingleStageTrainer
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=128, depth=2, heads=2, num_coarse_quantizers=3, ff_dropout=0.0, precision="bf16x3").to(dev)
    ds = SyntheticTokenDataset("coarse", length=8, coarse_window_seconds=1, semantic_window_seconds=2)
    base = dict(num_train_steps=4, batch_size=2, dataset=ds, lr=1e-3, lr_warmup=0, grad_accum_every=1, wd=0.01, max_grad_norm=0.5, valid_frac=0.0,
                save_results_every=1000, save_model_every=1000, results_folder=str(folder), save_predicted_tokens=False,
                save_reconstructed_wave=False, use_hip_graph=False)
    base.update(kw)
    tr = SingleStageTrainer(model, "coarse", **base)
    records = []
    tr.tracker.log = lambda values, step=None: records.append(dict(values))
    return tr, records


def test_trainer_defaults_log_what_they_logged(dev, tmp_path):
    tr, records = _trainer(dev, tmp_path / "res", save_results_every=1)
    logs = tr.train_step()
    assert set(logs) == {"loss"} and set(records[0]) == {"train_loss", "valid_loss", "valid_accuracy"}
    assert tr.train_metrics() is None and tr.last_valid_metrics is None


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_train_metrics(dev, tmp_path, use_graph, accum):
    import gc
    tr, records = _trainer(dev, tmp_path / "res", quantizer_metrics=True, use_hip_graph=use_graph, grad_accum_every=accum)
    try:
        for step in range(2):
            logs = tr.train_step()
            if use_graph:
                assert tr._graphed is not None and tr._graphed.graph is not None, tr._graphed.capture_error
            keys = [f"train_loss_q{i}" for i in range(3)]
            assert all(k in logs and logs[k] is not None for k in keys) and "train_top102_accuracy_q0" in logs and "train_entropy_q2" in logs
            rows = accum * 2 * 226                                               # micro-batches x samples x (75 x 3 ids + eos)
            assert logs["train_count_total"] == rows and logs["train_count_eos"] == accum * 2
            assert [logs[f"train_count_q{i}"] for i in range(3)] == [accum * 2 * 75] * 3
            # the count-weighted combination of the per-bin means is the step's loss (label_smoothing = z_loss = 0): fp32 atomics against
            # an ordered fp64 sum, the plain test's nll-sum bar
            comb = sum(logs[f"train_loss_{b}"] * logs[f"train_count_{b}"] for b in ("q0", "q1", "q2", "eos")) / rows
            assert abs(comb - logs["loss"]) <= 1e-5 * abs(logs["loss"]), (comb, logs["loss"])
            assert abs(logs["train_loss_total"] - logs["loss"]) <= 1e-5 * abs(logs["loss"])
            assert float(tr.train_metrics().bins.abs().sum()) == 0                # zeroed after the read
            assert all(k in records[-1] for k in keys) and records[-1]["train_loss"] == logs["loss"]
    finally:
        gc.unfreeze()


def test_trainer_validate(dev, tmp_path, monkeypatch):
    tr, records = _trainer(dev, tmp_path / "res", quantizer_metrics=True, ema_decay=0.99)
    tr.train_step()
    loss, acc = tr.validate(0)
    d = tr.last_valid_metrics
    n_labels = 2 * 226
    assert d["valid_count_total"] == n_labels
    assert round(d["valid_accuracy_total"] * n_labels) == round(acc * n_labels)  # the top-1 count of the bins is the count behind valid_accuracy
    assert abs(d["valid_loss_total"] - loss) <= 1e-5 * abs(loss)
    loss_e, acc_e = tr.validate(0, use_ema=True)                                  # on the EMA twin
    assert tr.last_valid_metrics["valid_count_total"] == n_labels and abs(tr.last_valid_metrics["valid_loss_total"] - loss_e) <= 1e-5 * abs(loss_e)
    # three batches: every host read comes after the last batch's launches
    tr3, records3 = _trainer(dev, tmp_path / "res3", quantizer_metrics=True, valid_batches=3, save_results_every=1)
    events = []
    w = tr3.train_wrapper.transformer_wrapper
    fwd = w.forward

    def logged_forward(**kw):
        events.append(("begin", kw.get("return_logits", True)))
        out = fwd(**kw)
        events.append(("end", None))
        return out
    monkeypatch.setattr(w, "forward", logged_forward)
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda o, nm: lambda self, *a, **k: (events.append(("read", nm if self.is_cuda else None)), o(self, *a, **k))[1])(orig, name))
    loss3, acc3 = tr3.validate(0)
    monkeypatch.undo()
    begins = [i for i, e in enumerate(events) if e[0] == "begin"]
    ends = [i for i, e in enumerate(events) if e[0] == "end"]
    assert len(begins) == 3 and [events[i][1] for i in begins] == [True, False, False]          # batches after the first: no logits leave the device
    outside = [i for i, e in enumerate(events) if e[0] == "read" and e[1] is not None and not any(b < i < e2 for b, e2 in zip(begins, ends))]
    assert outside and min(outside) > ends[-1], events
    d3 = tr3.last_valid_metrics
    assert d3["valid_count_total"] == 3 * n_labels
    assert abs(d3["valid_loss_total"] - loss3) <= 1e-5 * abs(loss3)              # the mean of three equal-sized batch losses
    assert acc3 == d3["valid_accuracy_total"]
    logs = tr3.train_step()                                                       # save_results_every = 1: validate runs inside, and is logged
    assert "valid_loss_q0" in records3[-1] and "train_loss_q0" in records3[-1] and "valid_loss_q0" not in logs
