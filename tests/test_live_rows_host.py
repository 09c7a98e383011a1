"""CPU: the live-rows rule of the last layer's feed-forward block (engine.live_rows) and its compact <-> full row maps.

With only some logit heads wanted (the trainers' loss weights [0, 0, 1]) the last layer's feed-forward block, the final LayerNorm and the
heads run on the rows [p0, N) of every sample.  The rule is a pure function of the layout, the wanted heads, the batch and the operand
type / FF width; these tests pin it at the three shipped stage layouts and at every refusal.
"""
import pytest
import torch

from open_musiclm_amd import engine

CPU = torch.device("cpu")
# tokens per sequence as run_forward sees them (eos appended, last token of the predicted sequence dropped) and quantizers per sequence:
# semantic (clap 12 + eos | 250 semantic), coarse (the bench shape: 12 + eos | 199 + eos | 3 x 300), fine (12 + eos | 3 x 200 + eos | 5 x 240)
STAGES = {
    "semantic": dict(lens=[13, 250], quant=[12, 1], Fp=2752),
    "coarse": dict(lens=[13, 200, 900], quant=[12, 1, 3], Fp=2752),
    "fine": dict(lens=[13, 601, 1200], quant=[12, 3, 5], Fp=2752),
}


def _lay(stage, B, final_rows_only=False):
    s = STAGES[stage]
    return engine.build_layout(B, s["lens"], s["quant"], CPU, final_rows_only)


def _last(stage):
    n = len(STAGES[stage]["lens"])
    return [False] * (n - 1) + [True]


def test_first_live_row_is_the_smallest_position_a_wanted_head_reads():
    for stage in STAGES:
        lay = _lay(stage, 2)
        for mask in range(1, 1 << len(lay.lens)):
            want = [bool(mask >> s & 1) for s in range(len(lay.lens))]
            reads = [int(a.min()) % lay.N for (s, _), (a, _, _) in lay.head_maps.items() if want[s]]
            assert engine.first_live_row(lay, want) == min(reads)
    assert engine.first_live_row(_lay("coarse", 2), [False, False, False]) is None


@pytest.mark.parametrize("B", [1, 2, 32])
@pytest.mark.parametrize("stage", list(STAGES))
def test_rule_at_the_shipped_layouts(stage, B):
    lay = _lay(stage, B)
    want = _last(stage)
    seg = engine.live_rows(lay, want, B, torch.float16, STAGES[stage]["Fp"])
    first = engine.first_live_row(lay, want)
    assert first == lay.starts[-1]
    if stage == "semantic":
        # the predicted sequence starts at row 14 of 265: nothing worth trimming (p0 would be < N / 16)
        assert seg is None
        return
    n_full, p0, n_live = seg
    assert n_full == lay.N and n_live == lay.N - p0
    assert p0 <= first - engine.CONV_HALO
    assert (B * n_live) % 64 == 0
    assert 16 * p0 >= lay.N
    # the largest such p0: no later row satisfies the K-multiple
    assert all((B * (lay.N - q)) % 64 != 0 for q in range(p0 + 1, first - engine.CONV_HALO + 1))
    for T in (torch.float16, torch.bfloat16):
        assert engine.live_rows(lay, want, B, T, STAGES[stage]["Fp"]) == seg


def test_rule_at_the_bench_shape():
    lay = _lay("coarse", 32)
    assert lay.N == 1116 and lay.starts == (0, 14, 215)
    assert engine.live_rows(lay, [False, False, True], 32, torch.float16, 2752) == (1116, 212, 904)
    assert 32 * 904 == 28928
    # every head wanted: the first sequence's heads read row 0
    assert engine.live_rows(lay, [True, True, True], 32, torch.float16, 2752) is None
    # the second and third: from row 14 on, less than N / 16
    assert engine.live_rows(lay, [False, True, True], 32, torch.float16, 2752) is None


def test_rule_refusals(monkeypatch):
    lay = _lay("coarse", 32)
    want = [False, False, True]
    ok = engine.live_rows(lay, want, 32, torch.bfloat16, 2752)
    assert ok is not None
    assert engine.live_rows(lay, want, 32, torch.float32, 2752) is None                       # fp32 operands ("bf16x3")
    assert engine.live_rows(lay, want, 32, torch.float16, 3072) == ok                          # the last one-pass FF width
    assert engine.live_rows(lay, want, 32, torch.float16, 3136) is None                        # two-pass backward / first-generation kernels
    assert engine.live_rows(lay, [False, False, False], 32, torch.float16, 2752) is None       # no head wanted
    assert engine.live_rows(_lay("coarse", 32, final_rows_only=True), want, 32, torch.float16, 2752) is None
    monkeypatch.setenv("OMLM_LIVE_ROWS", "0")                                                   # the test hook, read at every call
    assert engine.live_rows(lay, want, 32, torch.float16, 2752) is None
    monkeypatch.setenv("OMLM_LIVE_ROWS", "1")
    assert engine.live_rows(lay, want, 32, torch.float16, 2752) == ok
    monkeypatch.delenv("OMLM_LIVE_ROWS")
    # no p0 >= N / 16: a predicted sequence that starts too early
    early = engine.build_layout(2, [3, 4, 200], [1, 1, 1], CPU)
    assert early.starts[-1] == 9 and engine.live_rows(early, want, 2, torch.float16, 2752) is None
    # an odd batch needs N - p0 = 0 (mod 64): the step down from first_live - 2 may pass N / 16
    lay1 = engine.build_layout(1, [13, 20, 59], [12, 1, 3], CPU)                               # N = 95, first_live = 35
    assert engine.live_rows(lay1, want, 1, torch.float16, 2752) == (95, 31, 64)
    lay3 = engine.build_layout(3, [13, 4, 59], [12, 1, 3], CPU)                                # N = 79, first_live = 19: p0 = 15 (n_live = 64)
    assert engine.live_rows(lay3, want, 3, torch.float16, 2752) == (79, 15, 64)
    lay4 = engine.build_layout(3, [13, 2, 61], [12, 1, 3], CPU)                                # N = 79, first_live = 17: p0 <= 15 -> 15
    assert engine.live_rows(lay4, want, 3, torch.float16, 2752) == (79, 15, 64)
    lay5 = engine.build_layout(3, [13, 1, 62], [12, 1, 3], CPU)                                # first_live = 16: p0 <= 14 and = 15 (mod 64): none
    assert engine.live_rows(lay5, want, 3, torch.float16, 2752) is None


@pytest.mark.parametrize("seg", [(1116, 212, 904), (95, 31, 64), (40, 8, 32)])
def test_compact_and_full_rows_round_trip(seg):
    n_full, p0, n_live = seg
    B = 3
    r = torch.arange(B * n_live)
    full = engine.live_to_full(r, seg)
    assert torch.equal(full, (r // n_live) * n_full + p0 + r % n_live)
    assert int(full.min()) == p0 and int(full.max()) == B * n_full - 1
    assert torch.equal(full % n_full >= p0, torch.ones_like(full, dtype=torch.bool))
    assert torch.equal(engine.full_to_live(full, seg), r)
    # every full row of the segment, and only those, is hit once
    inside = torch.arange(B * n_full)
    inside = inside[inside % n_full >= p0]
    assert torch.equal(full, inside)
    assert engine.live_to_full(n_live, seg) == n_full + p0 and engine.full_to_live(n_full + p0, seg) == n_live


def test_head_maps_are_rebased_onto_the_segment():
    B = 2
    lay = engine.build_layout(B, [13, 20, 59], [12, 1, 3], CPU)
    seg = engine.live_rows(lay, [False, False, True], B, torch.float16, 2752)
    assert seg == (95, 31, 64)
    for qq in range(3):
        a_map, c_map, rows = lay.head_maps[(2, qq)]
        a_live, c_live, rows_live = engine.head_map(lay, 2, qq, seg)
        assert rows_live == rows and c_live is c_map and a_live.dtype == torch.int32
        assert torch.equal(engine.live_to_full(a_live.long(), seg), a_map.long())
        assert int(a_live.min()) >= 0 and int(a_live.max()) < B * seg[2]
        assert engine.head_map(lay, 2, qq, None) == lay.head_maps[(2, qq)]
    assert engine.head_map(lay, 2, 5, seg) is None
