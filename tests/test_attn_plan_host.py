"""The attention route plan (csrc/attn_plan.h) against the launches recorded on an MI355X, without a GPU.

tests/attn_routes.json holds, per library call of tools/attn_route_calls.py (one call per arm of the dispatch: operand kind, prefix, dropout,
table form, workspace, the short / long boundaries and every refusal), the kernel launches a kernel trace saw -- kernel name with its
template arguments, grid, workgroup -- or the refusal's return code and message, and the values of the three pure size / limit exports over
a grid.  The table was recorded from the commit BEFORE the plan existed (its "source" field), so it is what the plan has to reproduce.

The header is built with the host c++ (its OMLM_PLAN_TEST_ABI wrappers).  The trace reports a dynamic LDS size of 0 for every dispatch, so
the plan's LDS bytes are checked against the layout each kernel states in its own comments (needed_lds below), and against the 160 KiB a
workgroup can have.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_musiclm_amd", "csrc")
TABLE = json.load(open(os.path.join(ROOT, "tests", "attn_routes.json")))
ROWS, SIZES = TABLE["rows"], TABLE["sizes"]
UNSUPPORTED = -3
FAMILIES = ("a1_fwd", "a1_dq", "a1_dkv", "a4_fwd", "a2_dq", "dbias_reduce", "a3_zero", "a3_dkv", "a3_reduce")
FORMS = ("short", "long", "part")
# kernels of attention2.hip that serve other entry points (table preparation, the keep-mask hook, the to_out dropout)
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
BF16_COPY, FP16_COPY, PUBLIC = 0, 1, 2
OTHER_ENTRIES = {"attn2_bias_prep_kernel", "attn_dropout_keep_kernel", "dropout_residual_fwd_kernel", "dropout_residual_bwd_kernel"}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no c++ on PATH")
    so = str(tmp_path_factory.mktemp("plan") / "libattn_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", CSRC, "-x", "c++", "-", "-o", so],
                   input=b'#include "attn_plan.h"\n', check=True)
    lib = C.CDLL(so)
    lib.omlm_plan_attn_table_floats.restype = lib.omlm_plan_attn_workspace_bytes.restype = C.c_longlong
    return lib


def parse_kernel(name):
    """(copy namespace, kernel, template arguments) of a kernel name as the trace has it -- demangled, or Itanium-mangled where the
    demangler does not know the 16-bit types; types as h16 / float, flags as 0 / 1"""
    m = re.match(r"(?:void )?(omlm_\w+)::(\w+)(?:<([^>]*)>)?\(", name)
    if m:
        # The profiler's demangler does not know the bf16 type (DF16b): it leaves a name that holds `DF16bLb0E` mangled and renders
        # `DF16bLb1E` as "bool _Accum, bool, E" -- the first-generation kernels' <h16_t, DROP = true, ...> instantiations.
        args = (m.group(3) or "").replace("bool _Accum, bool, E", "__bf16, true")
        words = {"true": 1, "false": 0, "float": "float", "__bf16": "h16", "_Float16": "h16"}
        return m.group(1), m.group(2), [words[a] for a in args.split(", ")] if args else []
    m = re.match(r"_ZN(\d+)", name)
    assert m, name
    at = 3 + len(m.group(1))
    ns, at = name[at:at + int(m.group(1))], at + int(m.group(1))
    m = re.match(r"(\d+)", name[at:])
    at += len(m.group(1))
    kernel, rest = name[at:at + int(m.group(1))], name[at + int(m.group(1)):]
    args = []
    if rest.startswith("I"):
        m = re.match(r"I((?:Lb[01]E|DF16_|DF16b|f)+)E", rest)
        assert m, name
        args = [int(t[2]) if t[0] == "L" else "float" if t == "f" else "h16" for t in re.findall(r"Lb[01]E|DF16_|DF16b|f", m.group(1))]
    return ns, kernel, args


def call_of(row, backward=None):
    """the call of a recorded row as the public entry receives it: the rule of the plan decides which copy serves it"""
    bias, biasT = row["bias"] in ("T", "raw"), row["bias"] in ("T", "zeroT")
    bwd = row["dir"] == "bwd" if backward is None else backward
    return (C.c_int * 13)(bwd, CODE[row["dt"]], PUBLIC, row["B"], row["N"], row["H"], row["P"], bias, biasT,
                          bool(row.get("dbias")), bool(row.get("dbias")) and row.get("ws", True), row.get("drop", 0.0) > 0, not row.get("split", False))


def run_plan(plan, call):
    out, msg = (C.c_longlong * (4 + 16 * 5))(), C.create_string_buffer(480)
    plan.omlm_plan_attn(call, out, msg)
    keys = ("family", "form", "precise", "pfx", "drop", "fixed", "win", "gx", "gy", "gz", "threads", "lds", "CH", "wps", "which", "floats")
    launches = [dict(zip(keys, out[4 + 16 * i:20 + 16 * i])) for i in range(out[1])]
    for l in launches:
        l["family"], l["form"] = FAMILIES[l["family"]], FORMS[l["form"]]
    return dict(rc=out[0], ldT=out[2], dkv_slots=out[3], fp16_copy=bool(plan.omlm_plan_attn_fp16_copy(call)), launches=launches, msg=msg.value.decode())


def implied(l, ns):
    """the kernel a launch of the plan names: (namespace, kernel, template arguments)"""
    f, T, dp = l["family"], "float" if l["precise"] else "h16", [l["drop"], l["pfx"]]
    long_, part = l["form"] == "long", l["form"] == "part"
    assert not ((long_ or part) and l["pfx"]), "the long and slot forms are causal"
    if f == "a1_fwd":
        return ns, "attn_fwd_kernel", [T] + dp
    if f == "a1_dq":
        return ns, "attn_bwd_dq_precise_kernel" if l["precise"] else "attn_bwd_dq_kernel", [T] + dp
    if f == "a1_dkv":
        return ns, "attn_bwd_dkv_kernel", [T] + dp
    assert not l["precise"], "fp32 operands run the first-generation kernels"
    if f == "a4_fwd":
        return ns, "attn4_fwd_long_kernel" if long_ else "attn4_fwd_kernel", [l["fixed"]] + dp
    if f == "a2_dq":
        return ns, "attn2_bwd_dq_long_kernel" if long_ else "attn2_bwd_dq_kernel", dp
    if f == "a3_dkv":
        return ns, "attn3_bwd_dkv_part_kernel" if part else "attn3_bwd_dkv_kernel", dp
    # the d(bias) reduction exists once, in the bf16 copy
    return {"dbias_reduce": ("omlm_bf16", "attn_dbias_reduce_kernel", []), "a3_zero": (ns, "a3_zero_kernel", []),
            "a3_reduce": (ns, "a3_part_reduce_kernel", [])}[f]


def needed_lds(kernel, args, row):
    """dynamic LDS bytes by the layout the kernel's own comments state"""
    N, H = row["N"], row["H"]
    Pn = min(row["P"], N)
    off = max(Pn - 1, 0)
    up = lambda n, m: (n + m - 1) // m * m
    precise = args[:1] == ["float"]
    if kernel == "attn_fwd_kernel":          # K | V tiles (fp32: hi / lo planes) + 4 heads' table
        return (4 if precise else 2) * 64 * 128 + 4 * (up(N, 32) + off) * 4
    if kernel in ("attn_bwd_dq_kernel", "attn_bwd_dq_precise_kernel"):     # 3 (5) tiles + 4 heads' table and bins + the mask words
        return (5 if precise else 3) * 64 * 128 + 8 * (up(N, 32) + off) * 4 + 8 * ((N + 63) // 64 + 1)
    if kernel == "attn_bwd_dkv_kernel":      # 32 KiB of tiles / reduction + H staged columns + 1 KiB, or the 4 waves' 128-float window patches
        staged = 32768 + H * (up(N, 32) + (31 if Pn else 0)) * 4 + 1024
        return 32768 + 4 * 128 * 4 if Pn == 0 and row["bias"] in ("T", "zeroT") and staged > 80 * 1024 else staged
    if kernel == "attn4_fwd_kernel":         # 3 stages of 20 KiB + 16-bit liveness per key + 64 ballot words + zeros
        return 3 * 20480 + up(N, 64) * 2 + 64 * 8 + 128
    if kernel == "attn4_fwd_long_kernel":    # per 64 keys: 64 x 16-bit liveness + one ballot word
        return 3 * 20480 + (N + 63) // 64 * (64 * 2 + 8) + 128
    if kernel == "attn2_bwd_dq_kernel":      # 3 stages of 28 KiB + 4 KiB scratch + the additive mask + 8 waves of bins
        return 3 * 28672 + 4096 + up(N, 64) * 4 + 8 * (up(N, 32) + off) * 4
    if kernel == "attn2_bwd_dq_long_kernel":     # ... + 4 KiB of bin rings + one mask byte per key
        return 3 * 28672 + 4096 + 4096 + up(N, 64)
    if kernel in ("attn3_bwd_dkv_kernel", "attn3_bwd_dkv_part_kernel"):     # 3 stages of two blocked images + four aux pieces
        return 3 * (2 * (4096 + 256) + 4 * 2048)
    assert kernel in ("attn_dbias_reduce_kernel", "a3_zero_kernel", "a3_part_reduce_kernel"), kernel
    return 0


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_plan_implies_the_recorded_launches(plan, row):
    got = run_plan(plan, call_of(row))
    if "refused" in row:
        assert (got["rc"], got["msg"], got["launches"]) == (row["refused"]["rc"], row["refused"]["message"], [])
        return
    assert got["rc"] == 0, got["msg"]
    ns = "omlm_f16" if row["dt"] == "float16" else "omlm_bf16"
    assert got["fp16_copy"] == (ns == "omlm_f16")              # the copy the plan names: fp16 wherever the code names it
    want = [(*parse_kernel(l["kernel"]), l["grid"], l["workgroup"]) for l in row["launches"]]
    have = [(*implied(l, ns), [l["gx"], l["gy"], l["gz"]], l["threads"]) for l in got["launches"]]
    assert have == want
    assert all(w[0] == ns for w in want if w[1] != "attn_dbias_reduce_kernel")     # ... is the one whose namespace the recorded kernels carry
    for l, (_, kernel, args, _, _) in zip(got["launches"], want):
        assert l["lds"] == needed_lds(kernel, args, row) <= 160 * 1024, kernel
    if got["ldT"]:
        assert got["ldT"] * ((row["H"] + 7) // 8 * 8) == plan.omlm_plan_attn_table_floats(row["N"], row["H"], row["P"])


def test_size_and_limit_exports_match_the_recorded_grid(plan):
    rows = lambda p, n: n if p == "N" else n + 5 if p == "N+5" else int(p)
    Ns, Hs, Bs, Ps = SIZES["N"], SIZES["H"], SIZES["B"], SIZES["P"]
    assert Ns[0] == 1 and Ns[-1] >= 16416 and len(Ns) >= 100
    assert [[[plan.omlm_plan_attn_table_floats(n, h, rows(p, n)) for p in Ps] for h in Hs] for n in Ns] == SIZES["table_floats"]
    assert [[[plan.omlm_plan_attn_workspace_bytes(b, n, h) for h in Hs] for n in Ns] for b in Bs] == SIZES["workspace_bytes"]
    for d, vals in SIZES["max_positions"].items():
        assert [plan.omlm_plan_attn_max_positions(int(d), p) for p in [-1, 0] + Ns] == vals, d


def test_table_covers_every_kernel_and_refusal():
    assert TABLE["source"].startswith("recorded from ")
    built = set()
    for f in os.listdir(CSRC):
        if re.match(r"attention\d?(\.hip|_\w+\.inc)$", f):
            src = open(os.path.join(CSRC, f)).read()
            built |= set(re.findall(r"#define A\w+_KERNEL (\w+)", src)) | set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    built -= OTHER_ENTRIES | {"A4_KERNEL", "A2Q_KERNEL", "A3_KERNEL"}
    seen = {}
    for r in ROWS:
        for l in r.get("launches", []):
            _, kernel, args = parse_kernel(l["kernel"])
            seen.setdefault(kernel, set()).add(tuple(args))
    assert set(seen) == built and len(built) == 13
    for kernel, combos in seen.items():          # every instantiation the library builds: both operand kinds, DROP, PFX, FIXED
        flags = combos
        if kernel in ("attn_fwd_kernel", "attn_bwd_dkv_kernel"):
            assert flags == {(t, d, p) for t in ("float", "h16") for d in (0, 1) for p in (0, 1)}, kernel
        elif kernel in ("attn_bwd_dq_kernel", "attn_bwd_dq_precise_kernel"):
            assert flags == {("float" if "precise" in kernel else "h16", d, p) for d in (0, 1) for p in (0, 1)}, kernel
        elif kernel == "attn4_fwd_kernel":
            assert flags == {(f, d, p) for f in (0, 1) for d in (0, 1) for p in (0, 1)}
        elif kernel == "attn4_fwd_long_kernel":
            assert flags == {(f, d, 0) for f in (0, 1) for d in (0, 1)}
        elif kernel in ("attn2_bwd_dq_kernel", "attn3_bwd_dkv_kernel"):
            assert flags == {(d, p) for d in (0, 1) for p in (0, 1)}, kernel
        elif kernel in ("attn2_bwd_dq_long_kernel", "attn3_bwd_dkv_part_kernel"):
            assert flags == {(0, 0), (1, 0)}, kernel
    assert {r["dt"] for r in ROWS if "launches" in r} == {"float16", "bfloat16", "float32"}
    messages = [r["refused"]["message"] for r in ROWS if "refused" in r]
    for part in ("with fp32 operands (bf16x3)", "with a non-causal prefix (P = ", "needs the prepared table (biasT, omlm_attn_bias_prepare)",
                 "is past the limit of 16384", "B N H >= 2^25 with N > 4096", "sequence too long for the LDS-resident bias table"):
        assert any(part in m for m in messages), part
    assert all(r["refused"]["rc"] == UNSUPPORTED for r in ROWS if "refused" in r)


def test_forward_and_backward_decide_alike(plan):
    """A prefix on the prepared table: the forward takes the second-generation kernel iff the backward's dQ and dK / dV kernels both do (lse is
    relative to the table's reference point there and only there), or the call is refused."""
    base = dict(dt="bfloat16", B=1, H=8, bias="T", dbias=True)
    n_second = n_first = 0
    for N in range(32, 4401):
        for P in (1, 14, 216, N):
            row = dict(base, N=N, P=P)
            fwd, bwd = run_plan(plan, call_of(row, False)), run_plan(plan, call_of(row, True))
            if fwd["rc"] or bwd["rc"]:
                assert (fwd["rc"] or UNSUPPORTED) == (bwd["rc"] or UNSUPPORTED) == UNSUPPORTED and N > 2048
                continue
            f2 = [l["family"] for l in fwd["launches"]] == ["a4_fwd", "a4_fwd"]
            assert f2 or [l["family"] for l in fwd["launches"]] == ["a1_fwd"]
            fam = [l["family"] for l in bwd["launches"]]
            assert fam == (["a2_dq", "dbias_reduce", "a3_zero", "a3_dkv"] if f2 else ["a1_dq", "dbias_reduce", "a1_dkv"]), (N, P)
            assert plan.omlm_plan_attn_second_generation(call_of(row, False)) == plan.omlm_plan_attn_second_generation(call_of(row, True)) == f2
            n_second, n_first = n_second + f2, n_first + (not f2)
    assert n_second > 4000 and n_first > 4000
    # the boundaries DESIGN.md quotes: the last N whose dQ kernel takes the prefix's bins
    fits = lambda N, P: [l["family"] for l in run_plan(plan, call_of(dict(base, N=N, P=P), False))["launches"]] == ["a4_fwd", "a4_fwd"]
    assert fits(2016, 14) and not fits(2017, 14) and fits(1856, 216) and not fits(1857, 216)


def test_prefix_past_the_32_bit_offsets_is_refused_before_any_launch(plan):
    """B N H = 2^25 with a prefix on the prepared table: the dK / dV kernel cannot address it and no other kernel shares the forward's
    reference point -- refused with a message that names the rule (it used to fail after the dQ kernel had run, without one)."""
    row = dict(dt="bfloat16", B=64, N=512, H=1024, P=14, bias="T")
    got = run_plan(plan, call_of(row, True))
    assert got["rc"] == UNSUPPORTED and got["launches"] == [] and "32-bit byte offsets (B N H 128 < 2^32)" in got["msg"]
    assert run_plan(plan, call_of(dict(row, B=63), True))["rc"] == 0
