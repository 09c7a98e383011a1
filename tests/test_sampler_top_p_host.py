"""CPU: the fp64 restatement of the sampler's nucleus rule (tests/sampler_top_p_ref.py) against a brute-force loop and the sort / cumsum
form, its properties, the argument block's layout, the validation helper, and the cap on ambiguous rows over the inputs that
tests/test_gpu_sampler_top_p.py compares the kernels on."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import loss_optim_sampler_ref as R
import sampler_top_p_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _rows(B, V, seed, ties):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, V), generator=g).float() if ties else torch.randn(B, V, generator=g) * 3
    return x, torch.rand(B, V, generator=g)


def _brute_mask(row, k, T, p, forbid):
    """Steps 1-4 of the rule for one row, in plain Python floats."""
    l = [float(v) for v in row]
    if forbid:
        l[-1] = -INF
    S = sorted(range(len(l)), key=lambda c: (-l[c], c))[:k]                 # ranked by logit descending, then index: its first k are S
    m = l[S[0]]
    if m == -INF:
        return set(S)
    w = {c: (math.exp((l[c] - m) / T) if l[c] > -INF else 0.0) for c in S}
    W = sum(w[c] for c in S)
    keep, before = set(), 0.0
    for c in S:
        if before < p * W:
            keep.add(c)
        before += w[c]
    return keep


@pytest.mark.parametrize("ties", [False, True])
def test_restatement_equals_a_brute_force_loop(ties):
    x, u = _rows(12, 37, 5 + ties, ties)
    x[3, 5:] = -INF
    x[4] = -INF
    for k in (1, 7, 37):
        for T in (0.4, 1.0):
            for p in (0.05, 0.37, 0.9, 0.999):
                for forbid in (False, True):
                    mask = P.nucleus_mask(x, k, T, p, forbid)
                    for b in range(x.shape[0]):
                        assert set(mask[b].nonzero().flatten().tolist()) == _brute_mask(x[b], k, T, p, forbid), (ties, k, T, p, forbid, b)
                    ids = P.sample(x, u, k, T, p, forbid)
                    sc = R.gumbel_scores(x, u, k, T, forbid)
                    want = torch.where(mask, sc, torch.full_like(sc, -INF)).argmax(1)
                    assert torch.equal(ids, want) and int(ids[4]) == 0


def test_restatement_equals_the_sort_cumsum_form_on_tie_free_rows():
    """The form every sampling interface states: sort the kept probabilities descending, keep while the mass before an entry is < p."""
    x, _ = _rows(16, 200, 11, False)
    for k in (20, 200):
        for T in (0.4, 1.0):
            for p in (0.05, 0.5, 0.9, 0.999):
                S = R.kept_mask(x, k, False)
                prob = torch.softmax(torch.where(S, x.double() / T, torch.full_like(x.double(), -INF)), dim=1)
                sp, order = prob.sort(dim=1, descending=True)
                keep_sorted = (sp.cumsum(1) - sp) < p
                want = torch.zeros_like(S).scatter_(1, order, keep_sorted) & S
                assert torch.equal(P.nucleus_mask(x, k, T, p, False), want), (k, T, p)


def test_nuclei_are_nested_in_p_and_inside_the_top_k_set():
    for ties in (False, True):
        x, _ = _rows(16, 300, 21 + ties, ties)
        rk = P.Ranked(x, 40, True)
        prev = None
        for p in (1e-6, 0.05, 0.3, 0.5, 0.9, 0.999, 1 - 1e-12):
            mask = rk.nucleus_mask(0.7, p)
            assert bool((mask & ~rk.S).sum() == 0) and bool(mask.any(1).all())
            if prev is not None:
                assert bool((prev & ~mask).sum() == 0), p
            prev = mask
        assert torch.equal(rk.nucleus_mask(0.7, 1.0), rk.S)               # p = 1 cuts nothing: W itself is not below W


def test_tiny_p_keeps_one_entry_the_first_maximum():
    for ties in (False, True):
        x, u = _rows(16, 300, 31 + ties, ties)
        mask = P.nucleus_mask(x, 30, 1.0, 1e-6, False)
        assert mask.sum(1).tolist() == [1] * 16
        assert torch.equal(mask.long().argmax(1), x.argmax(1))             # torch.argmax: the first maximum, the lowest index among equals
        assert torch.equal(P.sample(x, u, 30, 1.0, 1e-6, False), x.argmax(1))


def test_tie_rule_on_equal_logits():
    """Ten equal top logits over a floor 30 below (weights e^-30): p = 0.45 keeps the five lowest indices of the ten (mass before the
    sixth is 5, above 0.45 W), p = 0.51 six.  p = 0.5 sits on the boundary: five when S is the ten alone (5 is not below 0.5 * 10), six
    as soon as S holds a floor entry (W is a little more than 10)."""
    V = 50
    x = torch.full((1, V), -30.0)
    top = [3, 7, 8, 20, 21, 22, 30, 41, 45, 49]
    x[0, top] = 0.0
    for p, n in ((0.45, 5), (0.51, 6), (0.05, 1), (0.95, 10)):
        for k in (10, 25, V):
            mask = P.nucleus_mask(x, k, 1.0, p, False)
            assert mask[0].nonzero().flatten().tolist() == top[:n], (p, k)
    assert P.nucleus_mask(x, 10, 1.0, 0.5, False)[0].nonzero().flatten().tolist() == top[:5]
    assert P.nucleus_mask(x, 25, 1.0, 0.5, False)[0].nonzero().flatten().tolist() == top[:6]
    # k cuts the tied block first: S = the 4 lowest indices, and p = 0.45 of THEIR mass keeps two
    assert P.nucleus_mask(x, 4, 1.0, 0.45, False)[0].nonzero().flatten().tolist() == top[:2]
    # the last logit forbidden: the block has nine entries left
    assert P.nucleus_mask(x, V, 1.0, 0.45, True)[0].nonzero().flatten().tolist() == top[:5]
    assert P.nucleus_mask(x, V, 1.0, 0.95, True)[0].nonzero().flatten().tolist() == top[:9]


def test_ambiguous_rows_marks_a_cut_on_the_boundary():
    """Two entries of weight 1/2 each: at p = 1/2 the second one is in for a cut a little above and out for a cut a little below; its
    uniform makes it the winner when it is in."""
    x = torch.zeros(2, 2)
    u = torch.tensor([[0.5, 1 - 2.0 ** -24], [0.5, 1 - 2.0 ** -24]])
    assert P.ambiguous_rows(x, u, 2, 1.0, 0.5, False).tolist() == [True, True]
    assert P.ambiguous_rows(x, u, 2, 1.0, 0.4, False).tolist() == [False, False]
    assert P.sample(x, u, 2, 1.0, 0.4, False).tolist() == [0, 0] and P.sample(x, u, 2, 1.0, 0.6, False).tolist() == [1, 1]


def test_sample_args_layout_matches_header(tmp_path):
    """The ctypes mirror of omlm_sample_args (ops.SampleArgs) has the size and the field offsets a C compiler gives the header struct."""
    from open_musiclm_amd import ops
    fields = [f[0] for f in ops.SampleArgs._fields_]
    assert fields == ["logits", "B", "V", "ld", "uniform", "seed_lo", "seed_hi", "step", "row0", "step_dev", "out", "hist", "k",
                      "temperature", "top_p", "forbid_last", "emb_table", "emb_row_offset", "emb_rows", "x", "D"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "omlm.h")}"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(omlm_sample_args));']
    lines += [f'  printf("%zu\\n", offsetof(omlm_sample_args, {f}));' for f in fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(ops.SampleArgs)
    assert out[1:] == [getattr(ops.SampleArgs, f).offset for f in fields]


def test_header_source_and_signatures_name_the_entry_point():
    from open_musiclm_amd import hip
    hdr = open(os.path.join(ROOT, "include", "omlm.h")).read()
    src = open(os.path.join(ROOT, "open_musiclm_amd", "csrc", "sampler.hip")).read()
    m = re.search(r"int omlm_sample\(([^)]*)\);", hdr)
    assert m and len(hip.SIGNATURES["omlm_sample"]) == m.group(1).count(",") + 1
    assert 'extern "C" int omlm_sample(const omlm_sample_args* a, void* stream)' in src
    for word in ("top_p", "nucleus", "2^40"):                                 # the function is stated beside the declaration
        assert word in hdr[hdr.index("typedef struct omlm_sample_args") - 3000:hdr.index("typedef struct omlm_sample_args")], word


def test_validation_helper():
    from open_musiclm_amd import ops
    from open_musiclm_amd.open_musiclm import stage_top_p
    assert ops.check_top_p(None) == 1.0 and ops.check_top_p(1) == 1.0 and ops.check_top_p(0.25) == 0.25
    assert ops.check_top_p(1e-6) == 1e-6
    for bad in (0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), "half", [0.5]):
        with pytest.raises(ValueError, match="top_p"):
            ops.check_top_p(bad)
    with pytest.raises(ValueError, match="nucleus_mass"):
        ops.check_top_p(1.5, "nucleus_mass")
    assert stage_top_p(None) == (None, None, None) and stage_top_p(0.5) == (0.5, 0.5, 0.5)
    assert stage_top_p({"coarse": 0.9, "fine": 0.3}) == (None, 0.9, 0.3)
    with pytest.raises(ValueError, match=r"top_p\['fine'\]"):
        stage_top_p({"fine": 0.0})
    with pytest.raises(ValueError, match="top_p.*unknown"):
        stage_top_p({"acoustic": 0.5})
    with pytest.raises(ValueError, match="top_p"):
        stage_top_p(1.5)


@pytest.mark.parametrize("V", P.COMPARE_V)
def test_cap_on_ambiguous_rows_of_the_comparison_inputs(V):
    """On the very rows the GPU test compares the kernels on, at most AMBIGUOUS_CAP row per case is ambiguous (its id depends on where
    inside p (1 +- 2^-16) the cut falls): the allowance of the GPU test is not a way out of the comparison."""
    x, u = P.compare_rows(V)
    worst = total = rows = 0
    for k in P.compare_ks(V):
        for forbid in (False, True):
            rk = P.Ranked(x, k, forbid)
            for T in P.COMPARE_T:
                for p in P.COMPARE_P:
                    n = int(rk.ambiguous_rows(u, T, p).sum())
                    worst, total, rows = max(worst, n), total + n, rows + x.shape[0]
    print(f"top-p ambiguous rows at V={V}: {total} of {rows}, worst case {worst}")
    assert worst <= P.AMBIGUOUS_CAP, (V, worst, total, rows)
