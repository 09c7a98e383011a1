"""CPU: the fp64 restatement of the sampled id's two log-probabilities (tests/sampler_logprob_ref.py) against a brute-force loop, its
properties, the new entry point's declaration and host arguments, the after-eos rule, and the condition that keeps the bracket of
tests/test_gpu_sampler_logprob.py from hiding a failure."""
import inspect
import math
import os
import re

import pytest
import torch

import loss_optim_sampler_ref as R
import sampler_logprob_ref as L
import sampler_top_p_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _rows(B, V, seed, ties):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, V), generator=g).float() if ties else torch.randn(B, V, generator=g) * 3
    return x, torch.rand(B, V, generator=g)


def _brute(row, s, k, T, p, forbid):
    """(lp_model, lp_sampled) of id s for one row, in plain Python floats."""
    raw = [float(v) for v in row]
    l = list(raw)
    if forbid:
        l[-1] = -INF
    S = sorted(range(len(l)), key=lambda c: (-l[c], c))[:k]
    m = l[S[0]]
    if m == -INF:
        return -INF, -INF
    w = {c: (math.exp((l[c] - m) / T) if l[c] > -INF else 0.0) for c in S}
    W = sum(w.values())
    N, before = [], 0.0
    for c in S:
        if p >= 1.0 or before < p * W:
            N.append(c)
        before += w[c]
    big = max(raw)
    model = raw[s] - (big + math.log(sum(math.exp(v - big) for v in raw if v > -INF)))
    sampled = (l[s] - m) / T - math.log(sum(w[c] for c in N))
    return model, sampled


@pytest.mark.parametrize("ties", [False, True])
def test_restatement_equals_a_brute_force_loop(ties):
    x, u = _rows(12, 37, 5 + ties, ties)
    x[3, 5:] = -INF
    x[4] = -INF
    for k in (1, 7, 37):
        for T in (0.4, 1.0):
            for p in (0.05, 0.9, 1.0):
                for forbid in (False, True):
                    ids = P.sample(x, u, k, T, p, forbid) if p < 1 else R.sample(x, u, k, T, forbid)
                    pm, ps = L.lp_model(x, ids, forbid), L.lp_sampled(x, ids, k, T, p, forbid)
                    for b in range(x.shape[0]):
                        wm, ws = _brute(x[b], int(ids[b]), k, T, p, forbid)
                        for got, want in ((float(pm[b]), wm), (float(ps[b]), ws)):
                            assert (got == want) if want == -INF else abs(got - want) < 1e-12, (ties, k, T, p, forbid, b, got, want)
                    assert float(pm[4]) == -INF and float(ps[4]) == -INF


def test_sampled_probabilities_sum_to_one_and_model_is_not_positive():
    for ties in (False, True):
        x, u = _rows(8, 60, 41 + ties, ties)
        V = x.shape[1]
        for k, T, p, forbid in ((7, 0.4, 0.9, True), (60, 1.0, 1.0, False), (20, 0.7, 0.5, False), (60, 1.0, 0.999, True)):
            N = L.kept_set(x, k, T, p, forbid)
            total = torch.zeros(x.shape[0], dtype=torch.float64)
            for c in range(V):
                ids = torch.full((x.shape[0],), c)
                lp = L.lp_sampled(x, ids, k, T, p, forbid)
                total += torch.where(N[:, c], torch.exp(lp), torch.zeros_like(lp))
                assert bool((L.lp_model(x, ids, forbid) <= 0).all())
            assert float((total - 1).abs().max()) < 1e-12, (k, T, p, forbid)


def test_whole_row_at_temperature_one_makes_the_two_equal():
    x, u = _rows(8, 50, 51, False)
    ids = R.sample(x, u, 50, 1.0, False)
    assert float((L.lp_model(x, ids) - L.lp_sampled(x, ids, 50, 1.0, 1.0, False)).abs().max()) < 1e-12


def test_a_one_entry_set_gives_exactly_zero():
    for ties in (False, True):
        x, u = _rows(8, 50, 61 + ties, ties)
        ids = R.sample(x, u, 1, 0.4, True)
        assert L.lp_sampled(x, ids, 1, 0.4, 1.0, True).tolist() == [0.0] * 8
        ids = P.sample(x, u, 20, 0.7, 1e-6, False)
        assert L.lp_sampled(x, ids, 20, 0.7, 1e-6, False).tolist() == [0.0] * 8
    one = torch.tensor([[3.5]])
    assert L.lp_sampled(one, torch.zeros(1, dtype=torch.long), 1, 1.0, 1.0, False).tolist() == [0.0]
    assert L.lp_model(one, torch.zeros(1, dtype=torch.long)).tolist() == [0.0]
    assert L.lp_sampled(one, torch.zeros(1, dtype=torch.long), 1, 1.0, 1.0, True).tolist() == [-INF]      # V = 1, forbidden: the "id 0" rule
    assert L.lp_model(one, torch.zeros(1, dtype=torch.long), True).tolist() == [-INF]


def test_entry_point_is_declared_and_the_host_takes_the_arguments():
    """Fails before omlm_sample_lp exists."""
    from open_musiclm_amd import decode, hip, ops
    from open_musiclm_amd import open_musiclm as M
    hdr = open(os.path.join(ROOT, "include", "omlm.h")).read()
    src = open(os.path.join(ROOT, "open_musiclm_amd", "csrc", "sampler.hip")).read()
    m = re.search(r"int omlm_sample_lp\(([^)]*)\);", hdr)
    assert m and m.group(1).split(",")[0].strip() == "const omlm_sample_args* args"
    assert len(hip.SIGNATURES["omlm_sample_lp"]) == m.group(1).count(",") + 1 == 4
    assert 'extern "C" int omlm_sample_lp(' in src
    for word in ("lp_model", "lp_sampled", "exactly 0.0f", "natural logarithms"):      # the quantities are stated beside the declaration
        assert word in hdr[hdr.index("int omlm_sample_lp(") - 3000:hdr.index("int omlm_sample_lp(")], word
    sample = inspect.signature(ops.sample).parameters
    assert sample["lp_model"].default is None and sample["lp_sampled"].default is None
    assert inspect.signature(decode.SamplingLoop.__init__).parameters["logprobs"].default is False
    assert "return_logprobs=False" in inspect.getsource(M.TokenConditionedTransformerWrapper)      # (generate is wrapped by decorators)
    assert M.LogProbs._fields == ("model", "sampled") and hasattr(M.TokenConditionedTransformerWrapper, "score")


def test_after_eos_rule_on_a_hand_made_id_tensor():
    from open_musiclm_amd.open_musiclm import zero_logprobs_after_eos
    from open_musiclm_amd.utils import mask_out_after_eos_id
    eos = 9
    ids = torch.tensor([[1, 2, 3, 4, 5, 6],
                        [1, 9, 3, 9, 5, 6],
                        [7, 7, 1, 2, 3, 9],
                        [7, 7, 9, 2, 3, 4]])
    lp = -torch.arange(1, 17, dtype=torch.float32).reshape(4, 4)             # beside the LAST four columns: the first two were supplied
    for keep, want in ((False, [[-1, -2, -3, -4], [0, 0, 0, 0], [-9, -10, -11, 0], [0, 0, 0, 0]]),
                       (True, [[-1, -2, -3, -4], [0, 0, 0, 0], [-9, -10, -11, -12], [-13, 0, 0, 0]])):
        got = zero_logprobs_after_eos(lp, ids, eos, keep)
        assert got.tolist() == want, keep
        replaced = (mask_out_after_eos_id(ids, eos, keep_eos=keep) != ids)[:, 2:]
        assert torch.equal(got == 0, replaced)
    assert lp[1].tolist() == [-5, -6, -7, -8]                                # the input is left as it was


def test_cpu_model_is_refused_by_score():
    from open_musiclm_amd import open_musiclm as M
    model = M.create_coarse_transformer(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                                        acoustic_codebook_size=16, num_clap_quantizers=2)
    w = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.score(conditioning_token_ids=[torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long)],
                pred_token_ids=torch.zeros(1, 2, 2, dtype=torch.long))


def test_the_bracket_is_tight_on_most_comparison_rows():
    """The kernels' nucleus lies between N- (cut at p (1 - DELTA)) and N+ (cut at p (1 + DELTA)); the GPU test accepts lp_sampled anywhere
    between the values of the two.  On at least 90 % of the finite comparison rows the two sets are EQUAL, so there the bracket is a
    point and the comparison is the plain one.  Measured with the restatement alone: printed below."""
    same = rows = wide = 0
    for V in P.COMPARE_V:
        x, u = P.compare_rows(V)
        for k in P.compare_ks(V):
            for forbid in (False, True):
                rk = P.Ranked(x, k, forbid)
                finite = torch.isfinite(rk.sorted[:, 0])
                for T in P.COMPARE_T:
                    for p in P.COMPARE_P:
                        ids = rk.sample(u, T, p)
                        lo, hi, eq = L.bracket(x, ids, k, T, p, forbid, ranked=rk)
                        assert bool((lo[finite] <= hi[finite]).all())
                        same += int((eq & finite).sum())
                        rows += int(finite.sum())
                        wide += int(((hi - lo)[finite] > 1e-4).sum())
    print(f"log-prob bracket: N- == N+ on {same} of {rows} finite rows ({100.0 * same / rows:.1f} %), wider than 1e-4 on {wide}")
    assert same >= 0.9 * rows, (same, rows)
