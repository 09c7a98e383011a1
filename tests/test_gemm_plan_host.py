"""The GEMM route planner (csrc/gemm_plan.h) against the launches recorded on an MI355X, without a GPU.

tests/gemm_routes.json holds, per library call of tools/gemm_route_calls.py (the real shapes of a coarse-small training step and one call
per arm of each rule and hook), the kernel launches a kernel trace saw: kernel name, grid, workgroup.  The table was recorded from the
commit BEFORE the planner existed (its "source" field), so it is what the planner has to reproduce, for ncu = 256 and persist_slots = 256.

The header is built with the host c++ (its OMLM_PLAN_TEST_ABI wrappers); every launch the plan implies must be the recorded one: kernel
family and template arguments (tile, k-major flags, output type, form), grid.x, grid.y, workgroup size.  The trace reports a dynamic LDS
size of 0 for every dispatch, so the plan's LDS bytes are checked against what the kernel named in the trace needs by its own layout:
two k-tiles of (BM + BN) x 64 16-bit elements (+ the walk's 32 x (WN + 4) fp32 epilogue rows), 128 KiB for the 256 x 256 ring / MX /
grouped kernels, 64 KiB (four 128 x 64 planes) for the register-staged fp32 kernel.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "gemm_routes.json")))
FORMS = ("fp32", "general", "fastk", "kmap", "split3", "persist", "ring")
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
PUBLIC = 2                                                     # the test ABI's copy value of a call as the public entry receives it
TYPES = {"DF16_": "h16", "DF16b": "h16", "f": "float", "float": "float", "h16pl_t": "h16pl"}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no c++ on PATH")
    so = str(tmp_path_factory.mktemp("plan") / "libgemm_plan.so")
    csrc = os.path.join(ROOT, "open_musiclm_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", csrc, "-x", "c++", "-", "-o", so],
                   input=b'#include "gemm_plan.h"\n', check=True)
    lib = C.CDLL(so)
    lib.omlm_plan_tail_ws.restype = lib.omlm_plan_mx_ws.restype = C.c_longlong
    return lib


def parse_kernel(name):
    """(copy namespace, kernel, template arguments) of a demangled or an Itanium-mangled kernel name; types as h16 / float / h16pl"""
    m = re.match(r"void (omlm_\w+)::(\w+)<(.*)>\(", name)
    if m:
        args = [TYPES.get(a.split("::")[-1], a.split("::")[-1]) for a in m.group(3).split(", ")]
        return m.group(1), m.group(2), [{"true": 1, "false": 0}.get(a, int(a) if a.isdigit() else a) for a in args]
    n = int(re.match(r"_ZN(\d+)", name).group(1))             # _ZN <len> namespace <len> kernel I <template arguments> E E v ...
    ns, rest = name[4 + len(str(n)) - 1:][:n], name[4 + len(str(n)) - 1 + n:]
    m = re.match(r"\d+(gemm\w+?)I(.*)EEvNS_", rest)
    assert m, name
    args = [int(t[2:-1]) if t[0] == "L" else TYPES[t] for t in re.findall(r"L[ib]\d+E|DF16_|DF16b|f", m.group(2))]
    return ns, m.group(1), args


def hooks_of(env):
    tile = env.get("OMLM_GEMM_TILE", "")
    fb = {"256x256": (256, 256), "256x128": (256, 128)}.get(tile, (0, 0))
    off = lambda k: env.get(k, "1")[:1] == "0"
    return (C.c_int * 7)(not off("OMLM_GEMM_PERSIST"), int(env.get("OMLM_GEMM_T8", "2")), bool(tile), fb[0], fb[1],
                         not off("OMLM_GEMM_TAIL_SPLIT"), not off("OMLM_MX_FUSE_TAIL"))


def tile_launch(v, ns, ak, bk, tout, cin, epi=0, planes16=False, split3=False):
    """the launch a GemmLaunch (as the test ABI writes it) implies: (namespace, kernel, template arguments, grid.x, grid.y, workgroup, LDS)"""
    form, bm, bn, gx, gy, th, lds = FORMS[v[0]], *v[1:7]
    assert not v[9], "k-row map on a wide tile"
    wm, wn = (128, 64) if (bm, bn) == (256, 256) else (64, 64)
    if form == "fp32":
        return ns, "gemm_kernel", ["float", ak, bk, "float"], gx, gy, th, lds
    if form == "ring":
        return ns, "gemm_tile8_kernel", [ak, bk, tout, int(split3)], gx, gy, th, lds
    if form == "persist":
        return ns, "gemm_bf16_tile_persist_kernel", [bm, bn, wm, wn, 0, bk, tout, int(cin), epi], gx, gy, th, lds
    return (ns, "gemm_bf16_tile_kernel", [bm, bn, wm, wn, ak, bk, tout, int(form == "kmap"), int(form == "split3"), int(form == "fastk"), epi],
            gx, gy, th, lds)


def needed_lds(kernel, a):
    if kernel == "gemm_kernel":
        return 4 * 128 * 64 * 2
    if kernel in ("gemm_tile8_kernel", "gemm_mx_kernel", "gemm_mx_fused_kernel", "gemm_wgrad_group_kernel"):
        return 131072
    if kernel == "gemm_tail_reduce_kernel":
        return 0
    return 2 * (a[0] + a[1]) * 64 * 2 + (32 * (a[3] + 4) * 4 if "persist" in kernel else 0)


def expected(plan, c, ncu, slots, ws_bytes):
    """the launches the planners imply for a recorded call, taken as the public entry receives it: with the dtype codes of its tensors"""
    hooks = hooks_of(c.get("env", {}))
    ns = "omlm_f16" if c["dt"] == "float16" else "omlm_bf16"
    if c["entry"] in ("qknorm", "wgrad_group", "planes16"):    # the entries that name one type: the rule alone says which copy serves them
        code = C.c_int(CODE[c["dt"]])
        assert plan.omlm_plan_gemm_copy_of(C.byref(code)) == (ns == "omlm_f16") and code.value == 1
    M, N, K = c.get("M"), c.get("N"), c.get("K")
    reduce = lambda kind, blocks: (ns, "gemm_tail_reduce_kernel", [kind], blocks, 1, 256, 0)
    if c["entry"] == "qknorm":
        v = (C.c_int * 10)()
        plan.omlm_plan_qknorm(M, N, K, slots, hooks, v)
        return [tile_launch(v, ns, 0, 0, "h16", False, epi=1)]
    if c["entry"] == "wgrad_group":
        n = len(c["probs"])
        mnk = (C.c_int * (3 * n))(*[x for p in c["probs"] for x in p[:3]])
        out, kt, start = (C.c_int * 3)(), (C.c_int * n)(), (C.c_int * n)()
        plan.omlm_plan_wgrad(mnk, n, 0, ncu, hooks, out, kt, start)
        assert list(start) == sorted(start) and start[0] == 0
        return [(ns, "gemm_wgrad_group_kernel", [int(FORMS[out[1]] != "general"), int(FORMS[out[1]] == "ring")], out[2], 1, 512, 131072)]
    if c["entry"] == "mx16":
        v = (C.c_int * 8)()
        plan.omlm_plan_mx(M, N, K, C.c_longlong(ws_bytes), ncu, hooks, v)
        nk_all, M1, S, ktps, fused, main_tiles, tail_tiles, blocks = v
        tout = "h16pl" if c.get("c_lo") else "float"
        if S < 2:
            return [(ns, "gemm_mx_kernel", [tout, 0], main_tiles, 1, 512, 131072)]
        assert plan.omlm_plan_mx_ws(M, N, K, ncu) == S * (M - M1) * ((N + 3) // 4 * 4) * 4 <= ws_bytes
        head = ([(ns, "gemm_mx_fused_kernel", [tout], main_tiles + tail_tiles * S, 1, 512, 131072)] if fused else
                [(ns, "gemm_mx_kernel", [tout, 0], main_tiles, 1, 512, 131072), (ns, "gemm_mx_kernel", ["float", 1], tail_tiles, S, 512, 131072)])
        return head + [reduce(3 if c.get("c_lo") == "bf8" else 2 if c.get("c_lo") else 0, blocks)]
    planes16 = c["entry"] == "planes16"
    ak, bk = int(c.get("ak", False)), int(c.get("bk", False))
    # ops.gemm sends fp32 operands of large enough products to omlm_gemm_planes (bf16 hi/lo planes, three products) unless a k-major operand is mapped
    x3 = (c["dt"] == "float32" and c.get("planes", True) and M * N * K >= 1 << 26 and not (ak and c.get("a_map")) and not (bk and c.get("b_map"))
          and (ak and bk or K % 8 == 0))
    in_dtype = 1 if x3 else CODE[c["dt"]]                      # (omlm_gemm_planes takes bf16 planes)
    out16 = bool(c.get("c_lo")) if planes16 else c["out"] != "float32"
    out_dtype = (in_dtype if out16 else 0) if planes16 else CODE[c["out"]]
    cin = c.get("cin")
    sh = (C.c_int * 16)(M, N, K, ak, bk, bool(c.get("a_map")), bool(c.get("b_map")), bool(c.get("c_map")), in_dtype, out_dtype, planes16 or x3,
                        planes16, PUBLIC, cin == "c", cin is not None, c.get("alpha", 1.0) == 1.0)
    v = (C.c_int * 24)()
    plan.omlm_plan_gemm(sh, C.c_longlong(ws_bytes), ncu, slots, hooks, v)
    assert plan.omlm_plan_gemm_fp16_copy(sh) == (ns == "omlm_f16")                        # the copy the rule names: the one whose kernels the trace saw (checked by the caller)
    M1, S, kind, blocks = v[0:4]
    tout = ("h16pl" if out16 else "float") if planes16 else ("h16" if out16 else "float")
    kw = dict(planes16=planes16, split3=planes16 or x3)
    main = tile_launch(v[4:14], ns, ak, bk, tout, cin is not None, **kw)
    if M1 == 0:
        return [main]
    assert 0 < M1 < M and M1 % 256 == 0
    if S == 0:
        return [main, tile_launch(v[14:24], ns, ak, bk, tout, cin is not None, **kw)]
    assert S * (M - M1) * ((N + 3) // 4 * 4) * 4 <= min(ws_bytes, plan.omlm_plan_tail_ws(M, N, ncu))
    return [main, tile_launch(v[14:24], ns, ak, bk, "float", False, **kw), reduce(kind, blocks)]


@pytest.mark.parametrize("row", TABLE["rows"], ids=[r["id"] for r in TABLE["rows"]])
def test_plan_implies_the_recorded_launches(plan, row):
    want = []
    for l in row["launches"]:
        ns, kernel, args = parse_kernel(l["kernel"])
        want.append((ns, kernel, args, l["grid_x"], l["grid_y"], l["workgroup"], needed_lds(kernel, args)))
    got = expected(plan, row, TABLE["ncu"], TABLE["persist_slots"], TABLE["ws_bytes"])
    assert [tuple(map(str, g)) for g in got] == [tuple(map(str, w)) for w in want]
    assert {w[0] for w in want} == {"omlm_f16" if row["dt"] == "float16" else "omlm_bf16"}


def test_table_covers_every_form_and_hook():
    assert TABLE["source"].startswith("recorded from ") and len(TABLE["rows"]) >= 70
    kernels = {parse_kernel(l["kernel"])[1] for r in TABLE["rows"] for l in r["launches"]}
    assert kernels >= {"gemm_kernel", "gemm_bf16_tile_kernel", "gemm_bf16_tile_persist_kernel", "gemm_tile8_kernel", "gemm_tail_reduce_kernel",
                       "gemm_mx_kernel", "gemm_mx_fused_kernel", "gemm_wgrad_group_kernel"}
    hooks = {k for r in TABLE["rows"] for k in r.get("env", {})}
    assert hooks == {"OMLM_GEMM_PERSIST", "OMLM_GEMM_T8", "OMLM_GEMM_TILE", "OMLM_GEMM_TAIL_SPLIT", "OMLM_MX_FUSE_TAIL"}
