"""CPU: the two conditions that keep tests/test_gpu_attn_edges.py honest, and the routes it reaches.

For every case of attn_edge_ref.CASES and for bf16, fp16 and fp32 ("bf16x3") operands, in fp64 on the CPU:
 * the reference with the kernels' stated rounding points (emulate) stays under HALF the tolerance the GPU test applies, on every tensor --
   so a correct kernel has room;
 * every wrong formula of MUTANTS that changes the case's results at all puts its worst tensor over TEN times the tolerance -- so a kernel
   with that defect cannot pass -- and every mutant is caught in at least one case of every mask pattern it can affect.
And, from the route plan (csrc/attn_plan.h, built with the host c++ as tests/test_attn_plan_host.py does): the GPU test's routes, taken over
CASES, reach every kernel family in its short form, in both instantiations where there are two, and the mixed plan of N < 32.
"""
import pytest
import torch

import attn_edge_ref as R
from test_attn_plan_host import call_of, plan, run_plan  # noqa: F401  (plan: the fixture that builds the header)

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# fp32 operands: the same draws before rounding and no tolerance above bf16's, so a mutant over ten times bf16's is over ten times fp32's
MUTANT_DTYPES = (torch.bfloat16, torch.float16)
SCALE = 8.0


def _cannot_change(mutant, case, keymask):
    """mutants that are provably the reference itself for a case (not evaluated; every other one is compared element by element)"""
    return ((mutant == "drop_key_64" and case.N <= 64) or (mutant == "dbias_256" and case.N <= 256) or
            (mutant == "mask_next_sample" and keymask is None) or (mutant == "head_next_column" and case.H == 1) or
            (mutant == "last_row_as_prev" and case.N < 2))


@pytest.fixture(scope="module")
def survey():
    """{(case name, dtype): (emulate's {tensor: (metric / tol, metric, index)}, {mutant: worst metric / tol over the tensors})}"""
    res = {}
    for case in R.CASES:
        for dtype in DTYPES:
            inp = R.make_inputs(case, dtype)
            args = (inp["q"], inp["k"], inp["v"], inp["bias"], inp["keymask"], inp["dout"], case.H, SCALE)
            ref = R.reference(*args)
            assert not ref.dead.any(), case.name            # rows without a live key have a test of their own
            em = R.worst_ratio(R.emulate(*args, dtype).val, ref, dtype)
            mut = {}
            for m in R.MUTANTS if dtype in MUTANT_DTYPES else ():
                if _cannot_change(m, case, inp["keymask"]):
                    continue
                wrong = R.reference(*args, mutant=m, terms=False)
                if all(torch.equal(wrong.val[n], ref.val[n]) for n in ref.val):
                    continue                                 # e.g. the dropped key is masked in every sample already
                mut[m] = max(r[0] for r in R.worst_ratio(wrong.val, ref, dtype).values())
            res[case.name, dtype] = (em, mut)
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_rounding_is_under_half_and_mutants_over_ten_times_tolerance(survey, case, dtype):
    em, mut = survey[case.name, dtype]
    for name, (ratio, metric, at) in em.items():
        # fp32 operands: the forward's tolerances are this file's business (attn_edge_ref: X3_EPS) and keep the margin; the backward's 2e-2 is
        # the project's, and its kernels recompute the scores from q and k rounded to bf16 -- up to 0.55 of it, under it but not under half
        assert ratio < (1.0 if dtype == torch.float32 and name not in ("out", "lse") else 0.5), (name, metric, at)
    for m, ratio in mut.items():
        assert ratio > 10.0, (m, R.MUTANTS[m], ratio)


def test_every_mutant_is_caught_in_every_pattern_it_can_affect(survey):
    assert all(R.tol_of(n, torch.float32) <= R.tol_of(n, torch.bfloat16) for n in R.TENSORS + ("lse",))
    for dtype in MUTANT_DTYPES:
        for m in R.MUTANTS:
            caught = {c.pattern for c in R.CASES if survey[c.name, dtype][1].get(m, 0.0) > 10.0}
            can = set(R.PATTERNS) - ({"none"} if m == "mask_next_sample" else set())
            assert caught == can, (m, dtype, can - caught)


def test_case_table_is_the_one_the_edges_ask_for():
    assert all(c.N in R.EDGE_N for c in R.CASES) and {c.N for c in R.CASES} == set(R.EDGE_N)
    assert {c.H for c in R.CASES if c.N in R.HEAD_N} == {1, 3, 8, 9, 16} and {c.H for c in R.CASES if c.N not in R.HEAD_N} == {3}
    g = torch.Generator().manual_seed(0)
    for c in R.CASES:
        km = R.make_keymask(c, g)
        if c.pattern == "none":
            assert km is None
            continue
        assert km.shape == (R.B_CASES, c.N) and bool(km[:, 0].all())
        if c.N > 2:
            assert not all(torch.equal(km[0], km[b]) for b in range(1, R.B_CASES)), c.name        # a wrong rowbase shows
        if c.pattern == "picket":
            assert int(km.sum(1).max()) <= 10
            if c.N >= 257:                                   # whole dead stretches between the seams; sample 0's tile [192, 256) entirely
                assert not km[:, 131:254].any() and not km[0, 192:256].any() and not km[:, 67:127].any() and km[:, 128:131].any()
        if c.pattern == "hole" and c.N >= 256:
            assert not km[0, 64:128].any() and not km[1, 128:256].any()
        if c.pattern == "rpad":
            assert km.sum(1).tolist() == [c.N, 1, min(33, c.N)]
        if c.pattern == "rpad2":
            assert km.sum(1).tolist() == [64, 65, min(128, c.N)]


def test_check_names_the_element():
    ref = torch.zeros(2, 3, 4, dtype=torch.float64)
    got = ref.clone()
    got[1, 2, 3] = 0.5
    term = torch.full_like(ref, 2.0)
    assert R.check(got, ref, term) == (0.25, (1, 2, 3))
    term[1, 2, 3] = 0.0                                      # an element without terms is measured against 1e-6 of the largest term sum
    e, at = R.check(got, ref, term)
    assert at == (1, 2, 3) and abs(e - 0.5 / 2e-6) < 1e-3
    got[0, 0, 0] = float("nan")                              # a NaN is the worst error, not an ignored one
    assert R.check(got, ref, term) == (float("inf"), (0, 0, 0))


def test_rows_without_a_live_key_are_flagged_and_add_nothing():
    case = R.Case("dead", 65, 3, "dense")
    inp = R.make_inputs(case, torch.float32)
    km = inp["keymask"].clone()
    km[:, :33] = False
    km[:, 33] = True
    ref = R.reference(inp["q"], inp["k"], inp["v"], inp["bias"], km, inp["dout"], case.H, SCALE)
    assert torch.equal(ref.dead, (torch.arange(65) < 33)[None].expand(3, 65))
    assert float(ref.val["out"][:, :33].abs().max()) == 0.0 and float(ref.val["dq"][:, :33].abs().max()) == 0.0
    assert bool((ref.val["lse"][:, :, :33] == R.DEAD_LSE).all()) and bool(ref.val["lse"][:, :, 33:].abs().max() < 100)
    assert float(ref.val["dk"][:, :33].abs().max()) == 0.0 and float(ref.val["dv"][:, :33].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in ref.val.values())
    # the rows that are left are the attention of the keys from 33 on: the same numbers as the problem cut down to them
    cut = R.reference(inp["q"][:, 33:], inp["k"][:, 33:], inp["v"][:, 33:], inp["bias"][:32], km[:, 33:], inp["dout"][:, 33:], case.H, SCALE)
    for n in ("out", "dq", "dk", "dv"):
        assert float((ref.val[n][:, 33:] - cut.val[n]).abs().max()) < 1e-12, n
    assert float((ref.val["dbias"][:32] - cut.val["dbias"]).abs().max()) < 1e-12 and float(ref.val["dbias"][32:].abs().max()) == 0.0


def test_prefix_of_one_row_is_the_causal_reference():
    case = R.CASES[[c.name for c in R.CASES].index("N65-H3-dense")]
    inp = R.make_inputs(case, torch.bfloat16)
    args = (inp["q"], inp["k"], inp["v"], inp["bias"], inp["keymask"], inp["dout"], case.H, SCALE)
    a, b = R.reference(*args, P=0), R.reference(*args, P=1)
    assert all(torch.equal(a.val[n], b.val[n]) for n in a.val) and all(torch.equal(a.term[n], b.term[n]) for n in a.term)


def test_routes_reach_every_short_form_family(plan):
    seen, mixed = set(), False
    for route in R.ROUTES:
        for dtype in route.dtypes:
            for case in route.cases:
                for backward in (False, True):
                    got = run_plan(plan, call_of(R.plan_row(route, dtype, case, backward)))
                    assert got["rc"] == 0, (route.name, case.name, got["msg"])
                    assert all(l["form"] == "short" for l in got["launches"])
                    fam = [l["family"] for l in got["launches"]]
                    seen |= {(l["family"], l["precise"], l["fixed"]) for l in got["launches"]}
                    gen1 = route.name in ("fp32", "prefix1")
                    if not backward:
                        assert fam == (["a1_fwd"] if gen1 else ["a4_fwd", "a4_fwd"]), (route.name, case.name)
                        continue
                    reduce = ["dbias_reduce"] if route.table != "none" and route.ws else []
                    if gen1:
                        assert fam == ["a1_dq"] + reduce + ["a1_dkv"], (route.name, case.name)
                    elif case.N < 32:                       # the mixed plan: the dK / dV plan needs one whole 32-row query tile
                        assert fam == ["a2_dq"] + reduce + ["a1_dkv"], (route.name, case.name)
                        mixed = True
                    else:
                        assert fam == ["a2_dq"] + reduce + ["a3_zero", "a3_zero", "a3_dkv"], (route.name, case.name)
    assert mixed
    for f in ("a1_fwd", "a1_dq", "a1_dkv"):                  # the precise and the 16-bit instantiations
        assert (f, 1, 0) in seen and (f, 0, 0) in seen, f
    assert ("a4_fwd", 0, 0) in seen and ("a4_fwd", 0, 1) in seen
    assert {"a2_dq", "dbias_reduce", "a3_zero", "a3_dkv"} <= {f for f, _, _ in seen}
    assert "a3_reduce" not in {f for f, _, _ in seen}      # the slot form belongs to N > 4096 (tests/test_gpu_long_seq.py)
