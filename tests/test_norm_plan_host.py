"""The LayerNorm / qk-norm plan (csrc/norm_plan.h) against the launches recorded on an MI355X, and the Python mirrors against the plan; no GPU.

tests/norm_routes.json holds, per omlm_layernorm_* / omlm_qk_norm_* call of tools/norm_route_calls.py (one call per arm of the dispatch: entry,
dtype codes, the general and the row-pair kernels, every FL of the row-pair backward for every (cast, dy) pair, XC / LO / SEG / MAXV forms, the
row seams of the grid caps and of the column sum's split, with and without workspace and dgamma, and every refusal), the kernel launches a
kernel trace saw -- kernel name with its template arguments, grid, workgroup -- or the refusal's return code and message.  The table was
recorded from the commit BEFORE the plan existed (its "source" field), so it is what the plan has to reproduce.

The header is built with the host c++ (its OMLM_PLAN_TEST_ABI wrappers).
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
TABLE = json.load(open(os.path.join(ROOT, "tests", "norm_routes.json")))
ROWS = TABLE["rows"]
TRACED = [r for r in ROWS if r["op"] != "ws_bytes"]
ERR_ARG = -1
OPS = ("fwd", "planes", "mx", "mx_seg", "bwd", "qk_fwd", "qk_bwd", "qk_bwd2")
KERNELS = ("ln_fwd", "ln_fwd_row1", "ln_fwd_mx", "ln_bwd", "ln_bwd_row1", "qk_fwd", "qk_bwd", "qk_bwd2", "colsum")
LAUNCH = ("kernel", "t16", "tdy16", "xc", "lo", "seg", "fl", "maxv", "gx", "gy", "threads", "rows", "fp32_only")
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
BF16_COPY, FP16_COPY, PUBLIC = 0, 1, 2
# the instantiations the fp16 copy does not build: every fp32-only form
FP32_ONLY = {("ln_fwd_kernel", "float", 0, 0), ("ln_fwd_row1_kernel", "float", 1, 0, 0), ("ln_fwd_row1_kernel", "float", 0, 0, 0),
             ("ln_bwd_kernel", "float", "float", 0), ("qk_norm_fwd_kernel", "float"), ("qk_norm_bwd_kernel", "float")} | {
                 ("ln_bwd_row1_kernel", "float", "float", fl, 0) for fl in range(8)}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no c++ on PATH")
    so = str(tmp_path_factory.mktemp("plan") / "libnorm_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", CSRC, "-x", "c++", "-", "-o", so],
                   input=b'#include "norm_plan.h"\n', check=True)
    lib = C.CDLL(so)
    lib.omlm_plan_norm.argtypes = [C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_longlong), C.c_char_p, C.c_char_p]
    lib.omlm_plan_ln_bwd_workspace_bytes.restype = C.c_longlong
    return lib


def call(op, M, D=1024, ldy=None, H=8, dtype=1, dy_dtype=1, copy=PUBLIC, operands=True, xcast=False, stats=True, xc=False, dres=True, dres2=False,
         dxcast=True, dgamma=True, workspace=True, seg=(0, 0, 0), y8_stride=0):
    """a call as the test ABI takes it"""
    v = (C.c_int * 20)(OPS.index(op), M, D, D if ldy is None else ldy, H, dtype, dy_dtype, copy, operands, xcast, stats, xc, dres, dres2, dxcast, dgamma,
                       workspace, *seg)
    return v, y8_stride


def call_of(row):
    """the call of a recorded row, as the public entry receives it"""
    op, M, ldy = row["op"], row["M"], row["ldy"]
    rows = max(M, 1)
    stride = {"ok": (rows + 255) // 256 * 256 * 2 * ldy, "small": rows * 2 * ldy - 16}[row["stride"]]
    none = row["null"] == "all"
    # what the entry requires: the statistics are operands of every entry but the plain forward
    operands = row["null"] is None and (op == "fwd" or op.startswith("qk") or row["stats"])
    have = lambda name: bool(row[name]) and not none
    return call("mx_seg" if op == "mx" and row["seg"] else op, M, row["D"], ldy, row["H"], CODE[row["dt"]] if row["code"] is None else row["code"],
                CODE[row["dy"]] if row["dy_code"] is None else row["dy_code"], PUBLIC, operands, have("xcast"), have("stats"), have("xc"), have("dres"),
                have("dres2"), have("dxcast"), have("dgamma"), have("ws"), row["seg"] or (0, 0, 0), stride if op == "mx" else 0)


def run_plan(plan, c):
    out, msg, label = (C.c_longlong * (3 + 13 * 2))(), C.create_string_buffer(384), C.create_string_buffer(64)
    plan.omlm_plan_norm(c[0], c[1], out, msg, label)
    ls = [dict(zip(LAUNCH, out[3 + 13 * i:16 + 13 * i])) for i in range(out[1])]
    for l in ls:
        l["kernel"] = KERNELS[l["kernel"]]
    return dict(rc=out[0], fp16_copy=bool(out[2]), launches=ls, msg=msg.value.decode(), label=label.value.decode())


def implied(l, ns):
    """the kernel a launch of the plan names: (namespace, kernel, template arguments)"""
    T, TDY, k = "h16" if l["t16"] else "float", "h16" if l["tdy16"] else "float", l["kernel"]
    if k == "colsum":                                          # omlm_colsum_accumulate exists once, in the bf16 copy
        return "omlm_bf16", "colsum_kernel", []
    return ns, *{"ln_fwd": ("ln_fwd_kernel", [T, l["lo"], l["seg"]]), "ln_fwd_row1": ("ln_fwd_row1_kernel", [T, l["xc"], l["lo"], l["seg"]]),
                 "ln_fwd_mx": ("ln_fwd_mx_kernel", [l["maxv"], l["seg"]]), "ln_bwd": ("ln_bwd_kernel", [T, TDY, l["seg"]]),
                 "ln_bwd_row1": ("ln_bwd_row1_kernel", [T, TDY, l["fl"], l["seg"]]), "qk_fwd": ("qk_norm_fwd_kernel", [T]),
                 "qk_bwd": ("qk_norm_bwd_kernel", [T]), "qk_bwd2": ("qk_norm_bwd2_kernel", [T])}[k]


@pytest.mark.parametrize("row", TRACED, ids=[r["id"] for r in TRACED])
def test_plan_implies_the_recorded_launches(plan, row):
    got = run_plan(plan, call_of(row))
    if "refused" in row:
        assert (got["rc"], got["msg"], got["launches"]) == (row["refused"]["rc"], row["refused"]["message"], [])
        assert row["launches"] == []
        return
    assert got["rc"] == 0, got["msg"]
    ns = "omlm_f16" if got["fp16_copy"] else "omlm_bf16"
    want = [(*parse_kernel(l["kernel"]), l["grid"], l["workgroup"]) for l in row["launches"]]
    have = [(*implied(l, ns), [l["gx"], l["gy"]], l["threads"]) for l in got["launches"]]
    assert have == want
    # the copy that serves the call: fp16 wherever a code names it, and the mx forward
    assert got["fp16_copy"] == (row["op"] == "mx" or 2 in (call_of(row)[0][5], call_of(row)[0][6] if row["op"] == "bwd" else 0))
    for l in got["launches"]:
        assert not (got["fp16_copy"] and l["fp32_only"])
        if l["kernel"] == "colsum":                            # over the partial rows the kernel in front of it left: one per workgroup
            assert l["rows"] == got["launches"][0]["gx"] == min(row["M"], 2048)


def test_table_covers_every_kernel_and_refusal():
    assert TABLE["source"].startswith("recorded from e0303e0")
    built = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, "norm.hip")).read()))
    seen = {}
    for r in ROWS:
        for l in r["launches"]:
            ns, kernel, args = parse_kernel(l["kernel"])
            seen.setdefault(kernel, set()).add((ns, *args))
    assert set(seen) == built | {"colsum_kernel"} and len(built) == 8
    both = lambda *forms: {(ns, *f) for ns in ("omlm_bf16", "omlm_f16") for f in forms}
    bf16 = lambda *forms: {("omlm_bf16", *f) for f in forms}
    h = "h16"
    # every instantiation either copy builds: 58 in the bf16 copy, 48 in the fp16 copy
    assert seen["ln_fwd_kernel"] == both((h, 0, 0), (h, 0, 1), (h, 1, 0), (h, 1, 1)) | bf16(("float", 0, 0))
    assert seen["ln_fwd_row1_kernel"] == both((h, 0, 0, 0), (h, 1, 0, 0), (h, 0, 0, 1), (h, 0, 1, 0), (h, 0, 1, 1)) | bf16(("float", 0, 0, 0), ("float", 1, 0, 0))
    assert seen["ln_fwd_mx_kernel"] == {("omlm_f16", mv, sg) for mv in (1, 4) for sg in (0, 1)}
    mixed = [(h, h), (h, "float"), ("float", h)]
    assert seen["ln_bwd_kernel"] == both(*[(*p, 0) for p in mixed], (h, h, 1)) | bf16(("float", "float", 0))
    assert seen["ln_bwd_row1_kernel"] == both(*[(*p, fl, 0) for p in mixed for fl in range(8)], *[(h, h, fl, 1) for fl in (0, 1, 4, 5)]) | bf16(
        *[("float", "float", fl, 0) for fl in range(8)])
    assert seen["qk_norm_fwd_kernel"] == seen["qk_norm_bwd_kernel"] == both((h,)) | bf16(("float",))
    assert seen["qk_norm_bwd2_kernel"] == both((h,))
    assert seen["colsum_kernel"] == {("omlm_bf16",)}
    per_copy = lambda ns: sum(1 for k, forms in seen.items() if k != "colsum_kernel" for f in forms if f[0] == ns)
    assert (per_copy("omlm_bf16"), per_copy("omlm_f16")) == (58, 48)
    assert {(k, *f[1:]) for k, forms in seen.items() for f in forms if f[0] == "omlm_bf16"} >= FP32_ONLY and len(FP32_ONLY) == 14
    messages = {r["refused"]["message"] for r in ROWS if "refused" in r}
    for part in ("null pointer [x && gamma && y]", "null pointer [x && gamma && y && y_lo", "y8 && scale8", "null pointer [dy && x", "null pointer [q_raw",
                 "null pointer [dq && dk && dv && q_raw", "null pointer [dq && dk && dv && q && k", "D must be a multiple of 4 and <= 4096", "ldy < D [ldy >= D]",
                 "ldy < D [ldy >= D && ldy % 4 == 0]", "ldy / plane stride", "must hold D rounded up to 128 bytes", "row segment: n_full = p0 + n_live",
                 "layernorm_fwd_seg: statistics wanted", "layernorm_fwd_planes: out_dtype 1 (bf16) or 2 (fp16)", "dy_dtype: 0 = fp32",
                 "layernorm_bwd2_seg: 16-bit dy and cast type, no dres2", "qk_norm_bwd2: 16-bit operand types only", "qk_norm_bwd: M * (H + 2) must stay below 2^31",
                 "qk_norm_bwd2: M * (H + 2) must stay below 2^31"):
        assert any(part in m for m in messages), part
    assert len(messages) == 20                                 # the texts above, and no other
    assert all(r["refused"]["rc"] == ERR_ARG and not r["launches"] for r in ROWS if "refused" in r)
    # the seams: both sides of every grid cap were recorded
    grids = lambda k: {l["grid"][0] for r in ROWS for l in r["launches"] if parse_kernel(l["kernel"])[1] == k}
    assert {511, 512, 2047, 2048} <= grids("ln_bwd_row1_kernel") & grids("ln_bwd_kernel") and {2047, 2048} <= grids("ln_fwd_row1_kernel") & grids("ln_fwd_kernel")
    assert {4095, 4096} <= grids("qk_norm_fwd_kernel") and {511, 512} <= grids("qk_norm_bwd_kernel") and {1, 5, 255, 256} <= grids("qk_norm_bwd2_kernel")
    assert {l["grid"][1] for r in ROWS for l in r["launches"] if "colsum" in l["kernel"]} == {1, 16, 128}


def test_launch_failure_labels(plan):
    """what a failed launch is reported under: the entry's name, except that both mx entries report as omlm_layernorm_fwd_mx and both
    backward entries as omlm_layernorm_bwd2 (as before the plan)"""
    seg = (48, 8, 40)
    for c, label in ((call("fwd", 80), "omlm_layernorm_fwd"), (call("fwd", 80, seg=seg), "omlm_layernorm_fwd_seg"),
                     (call("planes", 80), "omlm_layernorm_fwd_planes"), (call("planes", 80, seg=seg), "omlm_layernorm_fwd_planes_seg"),
                     (call("mx", 80, y8_stride=1 << 20), "omlm_layernorm_fwd_mx"), (call("mx_seg", 80, seg=seg, y8_stride=1 << 20), "omlm_layernorm_fwd_mx"),
                     (call("bwd", 80), "omlm_layernorm_bwd2"), (call("bwd", 80, seg=seg), "omlm_layernorm_bwd2"),
                     (call("qk_fwd", 80), "omlm_qk_norm_fwd"), (call("qk_bwd", 80), "omlm_qk_norm_bwd"), (call("qk_bwd2", 80), "omlm_qk_norm_bwd2")):
        got = run_plan(plan, c)
        assert got["rc"] == 0 and len(got["launches"]) >= 1 and got["label"] == label, (label, got)


def test_workspace_and_partial_rows(plan):
    for r in ROWS:
        if r["op"] == "ws_bytes":
            assert plan.omlm_plan_ln_bwd_workspace_bytes(r["D"]) == r["value"] == 2048 * r["D"] * 4
    for D in (4, 512, 768, 1024, 1028, 4096):
        assert plan.omlm_plan_ln_bwd_workspace_bytes(D) == 2048 * D * 4
        for M in (1, 63, 64, 2047, 2048, 2049, 35712):
            # the kernel writes one partial row per workgroup, the column sum reads as many, and the workspace holds them
            for dgamma in (True, False):
                got = run_plan(plan, call("bwd", M, D, dgamma=dgamma))
                assert got["rc"] == 0 and got["launches"][0]["gx"] == plan.omlm_plan_ln_bwd_partial_rows(M) == min(M, 2048)
                assert got["launches"][0]["gx"] * D * 4 <= plan.omlm_plan_ln_bwd_workspace_bytes(D)
                assert [l["kernel"] for l in got["launches"][1:]] == (["colsum"] if dgamma else [])
            got = run_plan(plan, call("bwd", M, D, workspace=False))
            assert [l["gx"] for l in got["launches"]] == [min(M, 512)]


def test_python_mirrors_equal_the_plan(plan):
    from open_musiclm_amd import engine, ops
    lim = (C.c_int * 9)()
    plan.omlm_plan_norm_limits(lim)
    assert list(lim) == [4096, 1024, 2048, 512, 4096, 512, 256, 1024, 256]
    # ops.layernorm_bwd sizes a deferred column sum by it: the rows omlm_layernorm_bwd2 leaves in the workspace
    assert ops.LN_BWD_PARTIAL_ROWS == lim[2]
    for M in (1, 80, 2047, 2048, 2049, 35712):
        assert min(M, ops.LN_BWD_PARTIAL_ROWS) == plan.omlm_plan_ln_bwd_partial_rows(M)
    # engine.ff_mx_ok's premise about omlm_layernorm_fwd_mx: at D % 64 == 0, D <= 4096 a row of 2 D bytes holds D rounded up to 128 -- and at no
    # other D % 4 == 0 does the route exist for every pitch (D < 64) or at all (D > 4096)
    Fp = 2752
    for D in range(4, 4200, 4):
        served = run_plan(plan, call("mx", 80, D, copy=FP16_COPY, y8_stride=256 * 2 * D))["rc"] == 0
        assert served == (64 <= D <= 4096), D
        if engine.ff_mx_ok(D, Fp):
            assert served, D
    assert engine.ff_mx_ok(4096, Fp) and not engine.ff_mx_ok(4160, Fp) and not engine.ff_mx_ok(1028, Fp)


def test_the_fp16_copy_names_no_fp32_instantiation(plan):
    """the fp16 copy builds none of the fp32-only forms: the plan refuses the calls that would need one (not reachable through the C entries:
    the bf16 copy hands over fp16 calls only, as code 1) and names none of them in what it serves"""
    text = "bad argument: the fp16 copy serves fp16 operands only [dtype == 1]"
    served = 0
    for D in (768, 1024):
        for op in ("fwd", "qk_fwd", "qk_bwd"):
            got = run_plan(plan, call(op, 80, D, dtype=0, copy=FP16_COPY))
            assert (got["rc"], got["msg"], got["launches"]) == (ERR_ARG, text, [])
        got = run_plan(plan, call("bwd", 80, D, dtype=0, dy_dtype=0, copy=FP16_COPY))
        assert (got["rc"], got["msg"], got["launches"]) == (ERR_ARG, text, [])
        for op in OPS:
            for dtype in (0, 1, 3):
                for dy in (0, 1):
                    for seg in ((0, 0, 0), (48, 8, 40)):
                        for fl in range(8):
                            got = run_plan(plan, call(op, 80, D, dtype=dtype, dy_dtype=dy, copy=FP16_COPY, xcast=bool(fl & 2), dres=bool(fl & 1),
                                                      dres2=bool(fl & 2), dxcast=bool(fl & 4), seg=seg, y8_stride=1 << 20))
                            assert not any(l["fp32_only"] for l in got["launches"])
                            assert not any((implied(l, "")[1], *implied(l, "")[2]) in FP32_ONLY for l in got["launches"])
                            served += bool(got["launches"])
    assert served > 500
    # ... and the bf16 copy, which has no mx kernels, refuses the mx forward
    for op in ("mx", "mx_seg"):
        got = run_plan(plan, call(op, 80, copy=BF16_COPY, seg=(48, 8, 40), y8_stride=1 << 20))
        assert (got["rc"], got["msg"], got["launches"]) == (ERR_ARG, "bad argument: the mx forward exists in the fp16 copy only [fp16_copy]", [])
    # the same calls in the bf16 copy reach the fp32 forms
    for op, k in (("fwd", "ln_fwd_row1"), ("qk_fwd", "qk_fwd"), ("qk_bwd", "qk_bwd"), ("bwd", "ln_bwd_row1")):
        got = run_plan(plan, call(op, 80, dtype=0, dy_dtype=0, copy=BF16_COPY))
        assert got["rc"] == 0 and got["launches"][0]["kernel"] == k and got["launches"][0]["fp32_only"]


def test_an_empty_call_plans_nothing(plan):
    """M <= 0 is success without a launch, before every check of the call's other arguments"""
    for op in OPS:
        got = run_plan(plan, call(op, 0, 6, ldy=2, operands=False, stats=False, dtype=2 if op != "qk_bwd2" else 0, dy_dtype=3, seg=(48, 0, 40)))
        assert (got["rc"], got["launches"]) == (0, []), op
