"""GPU: models whose predicted sequence has a codebook of 2048 entries or more generate on every route of generate() -- the cached eager
loop, the graph-captured loop and the uncached re-forward -- with the ids of the CPU oracle, and the cached step's logit head holds the
project's own bars at such a width on the step kernels the shipped models use."""

import pytest
import torch

from test_gpu_model import TOL, dev, relerr, report  # noqa: F401  (the shared fixture and bars)

pytestmark = pytest.mark.gpu

# name -> (token sequences as (codebook size, quantizers), time steps).  V1 = 2049 is the first width on the workgroup sampler;
# V1 = 4101 is no multiple of 8, so the logits' leading dimension pads, and three quantizer heads share the embedding table.
TINY = {"semantic_like": ([(32, 2), (2048, 1)], 6), "coarse_like": ([(32, 2), (48, 1), (4100, 3)], 2)}
_ORACLE = {}


def _oracle_case(name, seed):
    """The oracle's ids for one tiny model, once per (model, seed), with the smallest relative margin between the best and the second
    best score it sampled from (the oracle's own fp32 values, teacher-forced on its own ids: the stack is causal, row j predicts id j)."""
    if (name, seed) in _ORACLE:
        return _ORACLE[(name, seed)]
    from oracle import musiclm_oracle as O
    seqs, steps = TINY[name]
    spec = O.ModelSpec([O.SeqInfo(c, q) for c, q in seqs], dim=64, depth=1, heads=1)
    sd = O.init_state_dict(spec, seed)
    g = torch.Generator().manual_seed(100 + seed)
    cond = [torch.randint(0, c, (2, 3, q), generator=g) for c, q in seqs[:-1]]          # conditioning drawn first
    V1, Q = seqs[-1][0] + 1, seqs[-1][1]
    U = torch.rand(steps * Q, 2, V1, generator=g)
    ids = O.generate(sd, spec, cond, steps, U)
    flat = ids.reshape(2, -1)
    condx = [O.append_eos(t.reshape(2, -1).long(), e) for t, e in zip(cond, spec.eos_ids)]
    lg = O.token_conditioned_forward(sd, spec, condx + [flat], None, only_final=True)[-1]
    margin = float("inf")
    for j in range(steps * Q):
        last = lg[:, j].clone()
        last[:, -1] = float("-inf")
        sc = O.top_k_filter(last, 0.9) + (-torch.log(-torch.log(U[j] + 1e-20) + 1e-20))
        v, i = sc.topk(2, dim=1)
        assert torch.equal(i[:, 0], flat[:, j]), (name, seed, j)                          # the teacher-forced rows are the sampled ones
        margin = min(margin, float(((v[:, 0] - v[:, 1]) / v[:, 0].abs().clamp(min=1.0)).min()))
    _ORACLE[(name, seed)] = (spec, sd, cond, U, steps, ids, margin)
    return _ORACLE[(name, seed)]


@pytest.mark.parametrize("route", ["cached", "uncached", "graph"])
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", list(TINY))
def test_wide_codebook_generate_equals_oracle(dev, name, seed, route):
    """The oracle's best score beats the runner-up by at least 1e-3 relative at every step of these seeds (asserted first, on the oracle's
    own values: 1.6e-2 / 2.9e-2 semantic-like, 5.4e-3 / 5.7e-3 coarse-like), far above what bf16x3 logits differ from the oracle's by, so
    the sampled ids must be the oracle's on every route."""
    from open_musiclm_amd import decode
    from open_musiclm_amd import open_musiclm as M
    spec, sd, cond, U, steps, want, margin = _oracle_case(name, seed)
    report(f"wide_codebook_oracle_margin[{name},seed={seed}]", margin=margin)
    assert margin >= 1e-3, margin
    seqs = [M.TokenSequenceInfo(s.codebook_size, s.num_quantizers, False) for s in spec.token_sequences]
    model = M.TokenConditionedTransformer(token_sequences=seqs, dim=64, depth=1, heads=1, ff_dropout=0.0, precision="bf16x3").to(dev)
    model.load_state_dict(sd, strict=True)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    assert decode.supports(model, 1, prompt_rows=12)                                     # the cached routes are really the cached ones
    kw = {"cached": dict(use_cache=True), "uncached": dict(use_cache=False), "graph": dict(use_cache=True, use_graph=True)}[route]
    got = wrapper.generate(conditioning_token_ids=[t.to(dev) for t in cond], max_time_steps=steps, uniforms=U, **kw).cpu()
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    assert int(got.min()) >= 0 and int(got.max()) < spec.token_sequences[-1].codebook_size


@pytest.mark.parametrize("precision,B,wide", [("fp16", 1, False), ("fp16", 16, False), ("bf16", 17, True)])
def test_wide_head_cached_steps_vs_oracle(dev, precision, B, wide):
    """dim 1024, 8 heads, predicted codebook 2048 (V1 = 2049: 129 head tiles) on the step kernels the shipped models use: prefill plus 4
    teacher-forced cached steps against the oracle's forward (as test_cached_steps_vs_oracle), bars TOL[precision]["logits"]; then 6 ids
    sampled through SamplingLoop land inside the codebook."""
    from open_musiclm_amd import decode
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.utils import append_eos_id
    from oracle import musiclm_oracle as O
    torch.manual_seed(0)
    model = M.create_semantic_transformer(dim=1024, depth=1, heads=8, semantic_codebook_size=2048, ff_dropout=0.0, precision=precision).to(dev)
    model.eval()
    spec = O.ModelSpec([O.SeqInfo(1024, 12), O.SeqInfo(2048, 1)], dim=1024, depth=1, heads=8)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    g = torch.Generator().manual_seed(11)
    V1, n0, n_steps, n_new = 2049, 3, 5, 6
    cond = [torch.randint(0, 1024, (B, 1, 12), generator=g)]
    flat = torch.randint(0, 2048, (B, n0 + n_steps), generator=g)
    sel = list(range(B))[:2] if B <= 2 else [0, B - 1]
    with torch.no_grad():
        condx = [append_eos_id(t.reshape(B, -1).long(), e) for t, e in zip(cond, wrapper.eos_ids)]
        rows = sum(t.shape[-1] + 1 for t in condx) + 1 + n0 + n_steps + n_new
        dec = decode.CachedDecoder(model, B, rows, precision, wide=wide)
        assert dec.V1 == V1
        fd = flat.to(dev)
        got = [dec.prefill([t.to(dev) for t in condx] + [fd[:, :n0]]).clone()]
        for k in range(n0, n0 + n_steps - 1):
            got.append(dec.step(fd[:, k].contiguous(), k).clone())
        o = O.token_conditioned_forward(sd, spec, [t[sel] for t in condx] + [flat[sel][:, :n0 + n_steps - 1]], only_final=True)[-1]
        worst = max(relerr(lg[sel][:, :V1], o[:, n0 + i]) for i, lg in enumerate(got))
        report(f"wide_head_cached_steps[{precision},B={B}]", worst=worst, steps=len(got))
        assert len(got) == 5 and worst < TOL[precision]["logits"], worst
        # sample on from the last teacher-forced row: ids n0 + n_steps - 1 .. of the predicted sequence
        U = torch.rand(n_new, B, V1, generator=g).to(dev)
        loop = decode.SamplingLoop(dec, got[-1], U, n0 + n_steps - 1, n_new, max(int(0.1 * V1), 1), 1.0, [True], use_graph=False)
        ids = loop.run().cpu()
    assert ids.shape == (n_new, B) and int(ids.min()) >= 0 and int(ids.max()) < 2048, ids
    assert len({tuple(r) for r in ids.t().tolist()}) > 1 or B == 1                         # the rows are sampled, not copies of one
