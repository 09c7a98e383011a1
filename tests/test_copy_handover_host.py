"""The refusals of the twice-compiled families' C entries through the real library, against the pairs recorded before the hand-over changed; no GPU.

The bf16 copy of the library holds the C entries of the GEMM, ConvFeedForward-middle, attention and decode families and hands a call that names
fp16 (dtype code 2) to the fp16 copy (csrc/common.h).  tests/handover_refusals.json holds, per entry, per dtype code 1, 2 and an invalid 3 and
per call of tools/handover_refusal_calls.py -- every pointer null at non-empty sizes, each bad scalar the entry tests for, an empty call -- the
return code and the omlm_last_error text, recorded from the commit BEFORE the hand-over was rewritten (its "source" field).  The library
under test has to give the same pairs: a refusal keeps its code, its text and its place among the other checks of its entry, whichever copy
answers.

None of these calls reaches a launch.  The replay still runs in a process of its own that sees no GPU: the buffers that stand in for device
memory are host memory, and a library that lost a check must fail its launch, not run it.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "handover_refusals.json")))
ROWS = TABLE["rows"]
KEY = lambda r: (r["entry"], r["code"], r["case"])


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    import __graft_entry__ as G
    from open_musiclm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        G.build()
    out = str(tmp_path_factory.mktemp("handover") / "replayed.json")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "handover_refusal_calls.py"), hip.LIB_PATH, out, "replay"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {KEY(row): row for row in json.load(open(out))["rows"]}


def test_the_table_is_the_parents_and_covers_every_entry():
    assert TABLE["source"].startswith("recorded from b36ab75")
    entries = {r["entry"] for r in ROWS}
    assert entries == {"omlm_gemm", "omlm_gemm_qknorm", "omlm_gemm_planes16", "omlm_gemm_planes", "omlm_gemm_wgrad_group", "omlm_ffmid_fwd",
                       "omlm_ffmid_fwd_seg", "omlm_ffmid_fwd_planes", "omlm_ffmid_fwd_planes_seg", "omlm_ffmid_fwd_mx", "omlm_ffmid_fwd_mx_seg",
                       "omlm_ffmid_bwd", "omlm_mqa_attn_fwd", "omlm_mqa_attn_bwd", "omlm_decode_step", "omlm_decode_step_masked"}
    assert len({KEY(r) for r in ROWS}) == len(ROWS)
    for e in entries:
        for code in (1, 2, 3):
            mine = {r["case"]: r for r in ROWS if r["entry"] == e and r["code"] == code}
            assert len(mine) >= 3, (e, code)
            # an empty call of a real type returns 0 (omlm_gemm_planes16 tests its lo planes first; the decode entries have none: B = 0 is refused)
            if "empty" in mine and e != "omlm_gemm_planes16" and code != 3:
                assert (mine["empty"]["rc"], mine["empty"]["message"]) == (0, ""), (e, code)
    assert all(r["rc"] in (0, -1) and (r["rc"] == 0) == (r["message"] == "") for r in ROWS)      # nothing recorded is a failed launch (-2)
    texts = {r["message"] for r in ROWS}
    for part in ("null pointer [q && k && v && out && lse]", "prefix rows P >= 0 [P >= 0]", "dropout p in [0, 1) [attn_drop_args(p, seed, seed_dev, d)]",
                 "heads / bias pitch [H >= 1 && (!bias || bias_ld >= H)]", "fp16 operands produce fp32 or fp16 output [out_dtype == OMLM_DT_F32 || out_dtype == OMLM_DT_F16]",
                 "tail workspace: 16-byte aligned buffer and its size, or NULL / 0", "gemm_qknorm: operand dtype 1 (bf16) or 2 (fp16) [dtype == 1]",
                 "gemm_planes16: operand dtype 1 (bf16) or 2 (fp16) [dtype == 1]", "wgrad group: operand dtype must be 1 (bf16) or 2 (fp16) [dtype == 1]",
                 "null descriptor array [d]", "row segment: nseq must be n_full - p0, p0 > 0", "null argument block [a != nullptr]",
                 "ffmid_fwd_planes: dtype 1 (bf16) or 2 (fp16) [dtype == 1]", "du_tmp must be 8-byte aligned"):
        assert any(part in t for t in texts), part


@pytest.mark.parametrize("row", ROWS, ids=[f"{r['entry']}-{r['code']}-{r['case']}" for r in ROWS])
def test_every_call_answers_as_recorded(replayed, row):
    got = replayed[KEY(row)]
    assert (got["rc"], got["message"]) == (row["rc"], row["message"])


def test_the_replay_issued_the_recorded_calls_and_no_other(replayed):
    assert set(replayed) == {KEY(r) for r in ROWS}
