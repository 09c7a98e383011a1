"""The ConvFeedForward middle's plan (csrc/ffmid_plan.h) against the launches recorded on an MI355X, and the Python mirrors against the plan; no GPU.

tests/ffmid_routes.json holds, per omlm_ffmid_* call of tools/ffmid_route_calls.py (one call per arm of the dispatch: entry, operand type, kernel
generation, every NT / MAXC of every kernel, TRAIN / PL / MX / segment forms, one and two passes of the backward, which column sums are wanted,
and every refusal), the kernel launches a kernel trace saw -- kernel name with its template arguments, grid, workgroup -- or the refusal's
return code and message.  The table was recorded from the commit BEFORE the plan existed (its "source" field), so it is what the plan has to
reproduce.

The header is built with the host c++ (its OMLM_PLAN_TEST_ABI wrappers).  The trace reports no dynamic LDS size, so the plan's LDS bytes are
checked against a restatement of that commit's formulas (needed_lds below) and against the 160 KiB a workgroup can have.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

from kernel_names import parse_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_musiclm_amd", "csrc")
TABLE = json.load(open(os.path.join(ROOT, "tests", "ffmid_routes.json")))
ROWS = TABLE["rows"]
ERR_ARG = -1
OPS = ("fwd", "fwd_planes", "fwd_mx", "bwd")
KERNELS = ("fwd1", "bwd1", "bwd2", "strip_fwd", "strip_fwd_seg", "rowsum", "strip_bwd", "bwd3", "colsum_g", "colsum_c", "colsum_group")
LAUNCH = ("kernel", "t16", "n", "train", "pl", "mx", "gh", "gx", "gy", "threads", "lds", "RB", "strips", "total", "g_rows", "c_rows")
WS_G_ROWS, WS_C_ROWS = 1024, 512                               # the workspace's partial rows of d(gamma) / of d(conv taps)
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
BF16_COPY, FP16_COPY, PUBLIC = 0, 1, 2                         # (fp16_copy=False / True are the first two)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no c++ on PATH")
    so = str(tmp_path_factory.mktemp("plan") / "libffmid_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", CSRC, "-x", "c++", "-", "-o", so],
                   input=b'#include "ffmid_plan.h"\n', check=True)
    lib = C.CDLL(so)
    lib.omlm_plan_ffmid.argtypes = [C.POINTER(C.c_int), C.c_double, C.c_longlong, C.POINTER(C.c_longlong), C.c_char_p]
    lib.omlm_plan_ffmid_bwd_workspace_bytes.restype = lib.omlm_plan_ffmid_ws_dconv_at.restype = C.c_longlong
    return lib


def call(op, M, nseq, F, Fp, dtype, fp16_copy=False, p=0.0, operands=True, drop_bits=False, gh=False, dgamma=False, dconv=False, seg=(0, 0),
         h2_8_stride=0, planes_aligned=True, du_aligned=True, impl=1):
    """a call as the test ABI takes it"""
    v = (C.c_int * 17)(OPS.index(op), M, nseq, F, Fp, dtype, fp16_copy, operands, drop_bits, gh, dgamma, dconv, seg[0], seg[1], planes_aligned,
                       du_aligned, impl)
    return v, float(p), h2_8_stride


def call_of(row):
    """the call of a recorded row, as the public entry receives it (the mx forward has no dtype argument: its entry passes 1)"""
    op, M, Fp, bwd = row["op"], row["M"], row["Fp"], row["op"] == "bwd"
    rows = max(M, 1)
    stride = {"ok": (rows + 255) // 256 * 256 * 2 * Fp, "small": rows * 2 * Fp - 16, "odd": (rows + 255) // 256 * 256 * 2 * Fp + 8}[row["stride"]]
    dtype = (1 if op == "fwd_mx" else CODE[row["dt"]]) if row["dtype"] is None else row["dtype"]
    return call(op, M, row["nseq"], row["F"], Fp, dtype, fp16_copy=PUBLIC, p=row["p"], operands=row["null"] is None,
                drop_bits=row["drop"], gh=row["gh"], dgamma=bwd and row["dgamma"], dconv=bwd and row["dconv"], seg=row["seg"] or (0, 0),
                h2_8_stride=stride if op == "fwd_mx" else 0, planes_aligned=row["misalign"] != "planes", du_aligned=row["misalign"] != "du_tmp",
                impl=row["impl"])


def run_plan(plan, c):
    out, msg = (C.c_longlong * (3 + 16 * 4))(), C.create_string_buffer(384)
    plan.omlm_plan_ffmid(c[0], c[1], c[2], out, msg)
    ls = [dict(zip(LAUNCH, out[3 + 16 * i:19 + 16 * i])) for i in range(out[2])]
    for l in ls:
        l["kernel"] = KERNELS[l["kernel"]]
    return dict(rc=out[0], strips=bool(out[1]), fp16_copy=bool(plan.omlm_plan_ffmid_fp16_copy(c[0])), launches=ls, msg=msg.value.decode())


def implied(l, ns):
    """the kernel a launch of the plan names: (namespace, kernel, template arguments)"""
    T, k = "h16" if l["t16"] else "float", l["kernel"]
    if k.startswith("colsum"):                                 # omlm_colsum_accumulate / omlm_colsum_group exist once, in the bf16 copy
        return "omlm_bf16", "colsum_group_kernel" if k == "colsum_group" else "colsum_kernel", []
    if k in ("strip_fwd", "strip_fwd_seg"):
        return ns, "ffmid2_fwd_kernel" if k == "strip_fwd" else "ffmid2_fwd_seg_kernel", [T, l["n"], l["train"], l["pl"], l["mx"]]
    return ns, *{"fwd1": ("ffmid_fwd_kernel", [T, l["n"]]), "bwd1": ("ffmid_bwd1_kernel", [T, l["n"], l["gh"]]), "bwd2": ("ffmid_bwd2_kernel", [T]),
                 "rowsum": ("ffmid2_rowsum_kernel", [T, l["n"]]), "strip_bwd": ("ffmid2_bwd_kernel", [T]), "bwd3": ("ffmid3_bwd_kernel", [T, l["n"]])}[k]


def needed_lds(kernel, Fp):
    """dynamic LDS bytes by the formulas of the commit the table was recorded from: four fp32 rows where a wave holds a row"""
    return 4 * Fp * 4 if kernel in ("ffmid_fwd_kernel", "ffmid_bwd1_kernel", "ffmid2_rowsum_kernel") else 0


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_plan_implies_the_recorded_launches(plan, row):
    got = run_plan(plan, call_of(row))
    if "refused" in row:
        assert (got["rc"], got["msg"], got["launches"]) == (row["refused"]["rc"], row["refused"]["message"], [])
        assert row["launches"] == []
        return
    assert got["rc"] == 0, got["msg"]
    ns = "omlm_f16" if row["dt"] == "float16" else "omlm_bf16"
    # the copy that serves the call: the one whose namespace the recorded kernels carry -- fp16 wherever the code names it, and the mx forward
    assert got["fp16_copy"] == (ns == "omlm_f16") == (row["op"] == "fwd_mx" or call_of(row)[0][5] == 2)
    want = [(*parse_kernel(l["kernel"]), l["grid"], l["workgroup"]) for l in row["launches"]]
    have = [(*implied(l, ns), [l["gx"], l["gy"]], l["threads"]) for l in got["launches"]]
    assert have == want
    assert all(w[0] == ns for w in want if "colsum" not in w[1])
    for l, (_, kernel, _, _, _) in zip(got["launches"], want):
        assert l["lds"] == needed_lds(kernel, row["Fp"]) <= 160 * 1024, (kernel, l)
    second = any(k.startswith(("ffmid2_", "ffmid3_")) for _, k, _, _, _ in want)
    assert got["strips"] == second or not want


def test_table_covers_every_kernel_and_refusal():
    assert TABLE["source"].startswith("recorded from 1d3eb15")
    built = set()
    for f in ("ffmid.hip", "ffmid2.hip"):
        built |= set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, f)).read()))
    seen = {}
    for r in ROWS:
        for l in r["launches"]:
            ns, kernel, args = parse_kernel(l["kernel"])
            seen.setdefault(kernel, set()).add((ns, *args))
    assert set(seen) == built and len(built) == 10
    both = lambda *forms: {(ns, "h16", *f) for ns in ("omlm_bf16", "omlm_f16") for f in forms}
    every = lambda *forms: both(*forms) | {("omlm_bf16", "float", *f) for f in forms}
    # every instantiation of the first generation, of the backward kernels and of the plain strip forward; the one row-sum form that is left
    assert seen["ffmid_fwd_kernel"] == every((2,), (6,), (8,), (16,))
    assert seen["ffmid_bwd1_kernel"] == every(*[(mc, gh) for mc in (2, 6, 8, 16) for gh in (0, 1)])
    assert seen["ffmid_bwd2_kernel"] == seen["ffmid2_bwd_kernel"] == every(())
    assert seen["ffmid3_bwd_kernel"] == every((128,), (256,), (512,), (768,))
    assert seen["ffmid2_rowsum_kernel"] == every((8,))
    nts = range(64, 513, 64)
    assert seen["ffmid2_fwd_kernel"] >= every(*[(nt, tr, 0, 0) for nt in nts for tr in (0, 1)]) | both(*[(nt, 1, 1, 0) for nt in nts])
    assert seen["ffmid2_fwd_kernel"] >= {("omlm_f16", "h16", nt, 1, 1, 1) for nt in nts} | both((128, 0, 1, 0)) | {("omlm_f16", "h16", 128, 0, 1, 1)}
    assert not any(f[0] == "omlm_bf16" and f[-1] for f in seen["ffmid2_fwd_kernel"] | seen["ffmid2_fwd_seg_kernel"])        # MX: the fp16 copy only
    assert seen["ffmid2_fwd_seg_kernel"] >= every((64, 1, 0, 0), (128, 1, 0, 0), (512, 1, 0, 0), (128, 0, 0, 0)) | both((128, 1, 1, 0)) | {("omlm_f16", "h16", 128, 1, 1, 1)}
    assert seen["colsum_kernel"] == seen["colsum_group_kernel"] == {("omlm_bf16",)}
    messages = {r["refused"]["message"] for r in ROWS if "refused" in r}
    for part in ("null pointer [h1 && convw", "null pointer [h1 && h1_lo && convw && convw_lo && gamma && gamma_lo && h2 && h2_lo", "h2_8 && scale8",
                 "null pointer [dh2", "Fp must be F rounded up to 8 and <= 8192", "ffmid_fwd_planes: Fp must be F rounded up to 8 and <= 4096",
                 "ffmid_fwd_mx: Fp must be F rounded up to 8 and <= 4096", "M must be batch * nseq", "dropout p [", "dropout p (keep bits required when p > 0)",
                 "row segment: nseq must be n_full - p0, p0 > 0", "ffmid_fwd_mx: fp8 plane stride", "must hold Fp rounded up to 128 bytes",
                 "ffmid_fwd_planes: 16-byte aligned planes", "ffmid_fwd_mx: 16-byte aligned planes", "du_tmp must be 8-byte aligned",
                 "ffmid_fwd_planes: dtype 1 (bf16) or 2 (fp16)"):
        assert any(part in m for m in messages), part
    assert len(messages) == 17                                 # the texts above, and no other
    assert all(r["refused"]["rc"] == ERR_ARG and not r["launches"] for r in ROWS if "refused" in r)


def test_the_fp16_copy_refuses_other_operands(plan):
    """(not reachable through the C entries: the bf16 copy forwards fp16 operands as dtype 1)"""
    for op in ("fwd", "bwd"):
        got = run_plan(plan, call(op, 80, 40, 20, 24, 0, fp16_copy=True))
        assert (got["rc"], got["msg"], got["launches"]) == (ERR_ARG, "bad argument: the fp16 copy serves fp16 operands only [dtype == 1]", [])


def test_generations_workspace_and_partial_rows_over_the_widths(plan):
    """Fp = 8 .. 8192: the strip kernels up to 4096 and the one-pass backward up to 3072, exactly; the partial rows the kernels leave fit the
    workspace, whose size is the formula of the commit the table was recorded from; LDS within the workgroup's 160 KiB."""
    lim = (C.c_int * 5)()
    plan.omlm_plan_ffmid_limits(lim)
    assert list(lim) == [8192, 4096, 3072, WS_G_ROWS, WS_C_ROWS]
    worst = 0
    for Fp in range(8, 8193, 8):
        F = Fp - 3
        assert plan.omlm_plan_ffmid_bwd_workspace_bytes(F, Fp) == 4 * (1024 * Fp + 512 * 2 * F * 3)
        assert plan.omlm_plan_ffmid_ws_dconv_at(Fp) == 1024 * Fp
        assert (plan.omlm_plan_ffmid_fp_ok(F, Fp), plan.omlm_plan_ffmid_strip_ok(Fp), plan.omlm_plan_ffmid_one_pass(Fp)) == (1, Fp <= 4096, Fp <= 3072)
        for B, nseq in ((2, 40), (1, 1), (300, 37), (5, 1116), (410, 40), (64, 4096)):
            for dtype in (0, 1):
                fwd = run_plan(plan, call("fwd", B * nseq, nseq, F, Fp, dtype, p=0.1, drop_bits=True, gh=True))
                bwd = run_plan(plan, call("bwd", B * nseq, nseq, F, Fp, dtype, p=0.1, drop_bits=True, gh=True, dgamma=True, dconv=True))
                assert fwd["rc"] == bwd["rc"] == 0 and fwd["strips"] == bwd["strips"] == (Fp <= 4096)
                assert [l["kernel"] for l in fwd["launches"]] == (["strip_fwd"] if Fp <= 4096 else ["fwd1"])
                assert [l["kernel"] for l in bwd["launches"]] == (["bwd3"] if Fp <= 3072 else ["rowsum", "strip_bwd"] if Fp <= 4096 else ["bwd1", "bwd2"]) + ["colsum_group"]
                last = bwd["launches"][-1]
                assert 0 < last["g_rows"] <= WS_G_ROWS and 0 < last["c_rows"] <= WS_C_ROWS
                # the kernels in front of the sums write one partial row per workgroup (row of workgroups): the same counts
                first, main = bwd["launches"][0], bwd["launches"][-2]
                assert last["g_rows"] == (first["gy"] if first["kernel"] == "bwd3" else first["gx"]) and last["c_rows"] == main["gy"]
                worst = max([worst] + [l["lds"] for l in fwd["launches"] + bwd["launches"]])
    assert worst == 4 * 8192 * 4 <= 160 * 1024
    assert plan.omlm_plan_ffmid_fp_ok(8193, 8200) == plan.omlm_plan_ffmid_fp_ok(9, 8) == plan.omlm_plan_ffmid_fp_ok(4, 12) == 0
    assert plan.omlm_plan_ffmid_strip_ok(4100) == 0 and plan.omlm_plan_ffmid_strip_ok(4104) == 0


def test_python_mirrors_equal_the_plan(plan):
    from open_musiclm_amd import engine, ops
    lim = (C.c_int * 5)()
    plan.omlm_plan_ffmid_limits(lim)
    assert (engine.FF_PLANES_MAX_FP, engine.FF_ONE_PASS_MAX_FP) == (lim[1], lim[2])
    for Fp in range(8, 8193, 8):
        assert engine.ff_planes_ok(Fp) == bool(plan.omlm_plan_ffmid_strip_ok(Fp)), Fp
        # what engine.live_rows relies on below FF_ONE_PASS_MAX_FP: the strip forward and the one-pass backward
        assert (Fp <= engine.FF_ONE_PASS_MAX_FP) == bool(plan.omlm_plan_ffmid_strip_ok(Fp) and plan.omlm_plan_ffmid_one_pass(Fp)), Fp
    for F, Fp in ((4, 8), (20, 24), (341, 344), (2730, 2736), (4096, 4096), (8190, 8192)):
        assert ops.ffmid_bwd_workspace_floats(F, Fp) * 4 == plan.omlm_plan_ffmid_bwd_workspace_bytes(F, Fp)


def test_the_switch_changes_nothing_but_the_generation(plan):
    """impl = 0 and impl = 1 give the same plan wherever the strip kernels would not serve the call anyway, and another one where they would;
    the plane forwards know no switch."""
    n = {True: 0, False: 0}
    for Fp in (8, 520, 3072, 3080, 4096, 4104, 8192):
        for op, p, drop, gh in (("fwd", 0.0, False, False), ("fwd", 0.1, True, True), ("fwd", 0.1, False, True), ("bwd", 0.1, True, True),
                                ("bwd", 0.1, True, False), ("bwd", 0.1, False, True), ("bwd", 0.0, False, True)):
            a, b = (run_plan(plan, call(op, 80, 40, Fp - 4, Fp, 1, p=p, drop_bits=drop, gh=gh, dgamma=True, dconv=True, impl=impl)) for impl in (1, 0))
            served = bool(plan.omlm_plan_ffmid_strip_ok(Fp)) and (p == 0 or drop) and (op == "fwd" or gh)
            assert a["strips"] == served and not b["strips"] and (a == b) == (not served), (Fp, op, p, drop, gh)
            n[served] += 1
    assert min(n.values()) > 10, n
    for op, fp16 in (("fwd_planes", False), ("fwd_mx", True)):
        a, b = (run_plan(plan, call(op, 80, 40, 516, 520, 1, fp16_copy=fp16, p=0.1, drop_bits=True, gh=True, h2_8_stride=256 * 1040, impl=impl)) for impl in (1, 0))
        assert a == b and a["rc"] == 0 and a["strips"] and [l["kernel"] for l in a["launches"]] == ["strip_fwd"]


def test_an_empty_call_plans_nothing(plan):
    for op in OPS:
        got = run_plan(plan, call(op, 0, 40, 20, 24, 1, fp16_copy=op == "fwd_mx", operands=False))
        assert (got["rc"], got["launches"]) == (0, [])
