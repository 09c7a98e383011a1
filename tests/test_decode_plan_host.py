"""The decode step's plan (csrc/decode_plan.h) against the launches recorded on an MI355X, and decode.py's mirror against the plan; no GPU.

tests/decode_routes.json holds, per omlm_decode_step call of tools/decode_route_calls.py (one call per arm of the dispatch: generation, batch,
weight type, cache type, lo planes, which optional pointers are given, and every refusal), the kernel launches a kernel trace saw -- kernel
name with its template arguments, grid, workgroup -- or the refusal's return code and message.  The table was recorded from the commit BEFORE
the plan existed (its "source" field), so it is what the plan has to reproduce.  That commit launched the embedding gather before it checked
the lo-plane arguments: the rows of LATE keep those launches, and the plan must refuse them with the same message and launch nothing.

The header is built with the host c++ (its OMLM_PLAN_TEST_ABI wrappers).  The trace reports no dynamic LDS size, so the plan's LDS bytes
are checked against a restatement of that commit's formulas (needed_lds below) and against the 160 KiB a workgroup can have.
"""
import ctypes as C
import itertools
import json
import os
import re
import shutil
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_musiclm_amd", "csrc")
TABLE = json.load(open(os.path.join(ROOT, "tests", "decode_routes.json")))
ROWS = TABLE["rows"]
ERR_ARG = -1
LATE = ("refused/late: lo planes no W2p_lo, emb_table", "refused/late: lo planes B=2 L=0 no ln_parts, emb_table")
ROUTES = ("gen1", "dec3", "dec2", "dec4")
KERNELS = ("embed", "rowstat", "qkv1", "attn1", "gemv1", "ffin1", "attn2", "combine", "dec2", "dec3", "dec3_ffin", "dec4", "advance")
PHASES = ("prologue", "qkv", "attn", "combine", "out", "ffin", "ffout", "head", "advance")
QKV, OUT, FFIN, LNGEMV = 0, 1, 2, 3
HEAD = ("rc", "route", "G", "region", "npd", "npf", "stat_x", "stat_x1", "stat_u", "split", "comb_in_attn", "rowstat", "advance", "n", "layer", "tail")
LAUNCH = ("kernel", "phase", "w16", "c16", "n", "mode", "pl", "grp", "gx", "gy", "threads", "lds", "nsl", "nstat_in", "gtiles", "unrounded")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no c++ on PATH")
    so = str(tmp_path_factory.mktemp("plan") / "libdecode_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", CSRC, "-x", "c++", "-", "-o", so],
                   input=b'#include "decode_plan.h"\n', check=True)
    return C.CDLL(so)


def parse_kernel(name):
    """(copy namespace, kernel, template arguments) of a kernel name as the trace has it -- demangled, or Itanium-mangled where the
    demangler does not know the 16-bit types; types as h16 / float, numbers and flags as ints"""
    m = re.match(r"(?:void )?(omlm_\w+)::(\w+)(?:<([^>]*)>)?\(", name)
    if m:
        # The profiler's demangler reads the bf16 type (DF16b) as a fixed-point type and swallows the `L` behind it: `DF16bLi1ELi1E` comes
        # out as "bool _Accum, int, E, 1" and `DF16bLi2ELi1E` as "bool _Accum, int, EL, int, E" (the digit read as a name's length); every
        # other bf16 instantiation stays mangled.
        args = {"bool _Accum, int, E, 1": "__bf16, 1, 1", "bool _Accum, int, EL, int, E": "__bf16, 2, 1"}.get(m.group(3), m.group(3) or "")
        words = {"true": 1, "false": 0, "float": "float", "__bf16": "h16", "_Float16": "h16"}
        return m.group(1), m.group(2), [words[a] if a in words else int(a) for a in args.split(", ")] if args else []
    m = re.match(r"_ZN(\d+)", name)
    assert m, name
    at = 3 + len(m.group(1))
    ns, at = name[at:at + int(m.group(1))], at + int(m.group(1))
    m = re.match(r"(\d+)", name[at:])
    at += len(m.group(1))
    kernel, rest = name[at:at + int(m.group(1))], name[at + int(m.group(1)):]
    m = re.match(r"I((?:Li\d+E|Lb[01]E|DF16_|DF16b|f)+)E", rest)
    assert m, name
    args = [int(t[2:-1]) if t[0] == "L" else "float" if t == "f" else "h16" for t in re.findall(r"Li\d+E|Lb[01]E|DF16_|DF16b|f", m.group(1))]
    return ns, kernel, args


CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
BF16_COPY, FP16_COPY, PUBLIC = 0, 1, 2                         # (fp16_copy=False / True are the first two)
FLAGS = ("pos_dev", "parts", "ids", "emb_table", "head_W", "ln_parts", "splitk_ws", "splitk_cnt", "W1p_lo", "W2p_lo", "head_W_lo", "k_new", "advance_pos")


def call(B, D, H, Fp, w_dtype, L=1, Nmax=64, nsplit=1, V1=17, fp16_copy=False, round_bf16=None, kv16=False, **flags):
    """a call as the test ABI takes it; every flag of FLAGS that is not named is False"""
    assert set(flags) <= set(FLAGS), flags
    rb = (w_dtype != 0) if round_bf16 is None else round_bf16
    return (C.c_int * 25)(B, D, H, L, Fp, Nmax, nsplit, V1, w_dtype, fp16_copy, rb, kv16, *[bool(flags.get(f)) for f in FLAGS])


def call_of(row):
    """the call of a recorded row, as the public entry receives it"""
    null, lo, head = row["null"], row["lo"], row["head"]
    return call(row["B"], row["D"], row["H"], row["Fp"], CODE[row["w"]], L=row["L"], Nmax=row["Nmax"], nsplit=row["nsplit"],
                V1=row["V1"], fp16_copy=PUBLIC, round_bf16=row["round"], kv16=row["kv16"],
                pos_dev=null != "pos_dev", parts=null != "parts", ids=null != "ids", emb_table=row["emb"], head_W=head, ln_parts=row["ln"],
                splitk_ws=row["ws"], splitk_cnt=row["cnt"], W1p_lo=bool(lo), W2p_lo=bool(lo) and lo != "no_w2",
                head_W_lo=bool(lo) and head and lo != "no_head", k_new=bool(row["kv16"]) and null != "k_new", advance_pos=row["adv"])


def run_plan(plan, c):
    out, msg = (C.c_longlong * (16 + 16 * 11))(), C.create_string_buffer(320)
    plan.omlm_plan_decode(c, out, msg)
    got = dict(zip(HEAD, out[:16]))
    ls = [dict(zip(LAUNCH, out[16 + 16 * i:32 + 16 * i])) for i in range(got["n"] + 1)]
    for l in ls:
        l["kernel"], l["phase"] = KERNELS[l["kernel"]], PHASES[l["phase"]]
    got.update(route=ROUTES[got["route"]], launches=ls[:-1], q_rest=ls[-1], msg=msg.value.decode(), L=c[3], fp16_copy=bool(plan.omlm_plan_decode_fp16_copy(c)))
    return got


def expand(got):
    """the launches of the whole step in order, each with the layer it runs in: the layer's launches L times, q_rest as the q rows of layers >= 1"""
    ls, a, b = got["launches"], got["layer"], got["tail"]
    step = [(l, 0) for l in ls[:a]]
    for layer in range(got["L"]):
        step += [(got["q_rest"] if layer and i == a else ls[i], layer) for i in range(a, b)]
    return step + [(l, 0) for l in ls[b:]]


def implied(l, ns):
    """the kernel a launch of the plan names: (namespace, kernel, template arguments)"""
    T, C16 = "h16" if l["w16"] else "float", "h16" if l["c16"] else "float"
    k = l["kernel"]
    plain = {"embed": "dec_embed_kernel", "rowstat": "dec_rowstat_kernel", "combine": "dec_attn_combine_kernel"}
    if k in plain:
        return ns, plain[k], []
    if k == "advance":                                         # omlm_decode_advance exists once, in the bf16 copy
        return "omlm_bf16", "dec_advance_kernel", []
    if k in ("qkv1", "gemv1", "ffin1"):
        return ns, {"qkv1": "dec_qkv_kernel", "gemv1": "dec_gemv_kernel", "ffin1": "dec_ffin_kernel"}[k], [T]
    if k in ("attn1", "attn2"):
        return ns, "dec_attn_kernel" if k == "attn1" else "dec_attn2_kernel", [C16]
    if k == "dec2":
        assert not l["pl"] and not l["grp"]
        return ns, "dec2_kernel", [T, l["n"], l["mode"]]
    if k == "dec3":
        return ns, "dec3_kernel", [T, l["n"], l["mode"], l["pl"]]
    if k == "dec3_ffin":
        return ns, "dec3_ffin_kernel", [T, l["n"], l["pl"]]
    assert k == "dec4" and l["w16"], "the matrix-core kernels serve 16-bit weights"
    return ns, "dec4_kernel", [l["n"], l["mode"], l["pl"], l["grp"]]


def needed_lds(kernel, args, phase, layer, row):
    """dynamic LDS bytes by the formulas of the commit the table was recorded from (its launchers computed them next to each launch)"""
    B, D, H, Fp, L = row["B"], row["D"], row["H"], row["Fp"], row["L"]
    HD = H * 64
    K = {"qkv": D, "out": HD, "ffin": D, "ffout": Fp, "head": D}.get(phase)
    if kernel in ("dec_qkv_kernel", "dec_gemv_kernel", "dec_ffin_kernel"):      # the B activation rows + (16 rows x 8 samples + 16) floats
        return B * K * 4 + (16 * 8 + 16) * 4
    if kernel == "dec_attn_kernel":
        return (64 * 65 + 64 * 64 + 2 * HD) * 4
    if kernel == "dec_attn2_kernel":
        return (64 * 65 + 64 * 64 + HD + 8 * 64) * 4
    if kernel == "dec2_kernel":
        return (B * K + 8 * 8 + 8 * 2 + 4 * 8) * 4
    if kernel != "dec4_kernel":
        assert kernel in ("dec_embed_kernel", "dec_rowstat_kernel", "dec_attn_combine_kernel", "dec_advance_kernel", "dec3_kernel", "dec3_ffin_kernel"), kernel
        return 0
    NS, _, PL, _ = args
    nsl = 4 if NS == 6 else 0                                  # the NS = 6 instantiations are the four-slice FF-out launches
    kmax = 32 * (((K >> 5) + nsl - 1) // nsl) if nsl > 1 else K
    nb = min(B, 16)
    img = 16 if (NS + 7) // 8 == 1 else 8
    # LayerNorm statistics from the producers' partials (ln_parts given): behind the prologue's launch for the first q rows (and the head of
    # L = 0), behind an FF-out launch for the later ones; to_out applies no LayerNorm.  Without them: an fp32 staging copy
    first = row["emb"] or B > 8
    stat_in = row["ln"] and {"qkv": first or layer > 0, "head": first or L > 0}.get(phase, True)
    stage = nb * kmax * 4 if phase != "out" and not stat_in else 0
    return (((2 * img if PL else nb) * (kmax + 8) * 2 + 15) & ~15) + (16 * 8 + 16 * 2 + 4 * 256 + 256) * 4 + stage


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_plan_implies_the_recorded_launches(plan, row):
    if row["null"] == "args":                                  # the entry's own check, in front of the plan
        assert row["refused"]["message"] == "bad argument: null argument block [a != nullptr]" and not row["launches"]
        return
    got = run_plan(plan, call_of(row))
    if "refused" in row:
        assert (got["rc"], got["msg"], got["launches"]) == (row["refused"]["rc"], row["refused"]["message"], [])
        assert (row["launches"] != []) == (row["id"] in LATE)
        return
    assert got["rc"] == 0, got["msg"]
    ns = "omlm_f16" if row["w"] == "float16" else "omlm_bf16"
    assert got["fp16_copy"] == (ns == "omlm_f16")              # the copy the plan names: fp16 wherever w_dtype names it
    want = [(*parse_kernel(l["kernel"]), l["grid"], l["workgroup"]) for l in row["launches"]]
    step = expand(got)
    have = [(*implied(l, ns), [l["gx"], l["gy"]], l["threads"]) for l, _ in step]
    assert have == want
    assert all(w[0] == ns for w in want if w[1] != "dec_advance_kernel")       # ... is the one whose namespace the recorded kernels carry
    for (l, layer), (_, kernel, args, _, _) in zip(step, want):
        assert l["lds"] == needed_lds(kernel, args, l["phase"], layer, row) <= 160 * 1024, (kernel, l)
    names = {kernel for _, kernel, _, _, _ in want}
    if row["L"]:
        assert got["route"] == ("gen1" if "dec_qkv_kernel" in names else "dec3" if "dec3_ffin_kernel" in names else "dec4" if "dec4_kernel" in names else "dec2")


def test_table_covers_every_kernel_and_refusal():
    assert TABLE["source"].startswith("recorded from 6e642db")
    src = open(os.path.join(CSRC, "decode.hip")).read()
    built = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    seen = {}
    for r in ROWS:
        for l in r["launches"]:
            ns, kernel, args = parse_kernel(l["kernel"])
            seen.setdefault(kernel, set()).add((ns, *args))
    assert set(seen) == built and len(built) == 13
    both = lambda *forms: {(ns, *f) for ns in ("omlm_bf16", "omlm_f16") for f in forms}
    for kernel in ("dec_qkv_kernel", "dec_gemv_kernel", "dec_ffin_kernel"):
        assert seen[kernel] == both(("h16",)) | {("omlm_bf16", "float")}
    for kernel in ("dec_attn_kernel", "dec_attn2_kernel"):
        assert seen[kernel] == both(("h16",), ("float",))
    rows3 = [(2, QKV, 0), (6, LNGEMV, 0), (2, LNGEMV, 0)]
    assert seen["dec3_kernel"] == both(*[("h16", *f) for f in rows3]) | {("omlm_bf16", "float", *f) for f in rows3} | {("omlm_f16", "h16", 6, LNGEMV, 1), ("omlm_f16", "h16", 2, LNGEMV, 1)}
    assert seen["dec3_ffin_kernel"] == both(("h16", 4, 0)) | {("omlm_bf16", "float", 4, 0), ("omlm_f16", "h16", 2, 1)}
    # the vector kernels: every instantiation but <h16, 6, LNGEMV> (16-bit weights at B >= 2 with Fp <= 3072 and Fp % 32 != 0: no model has
    # such a width -- a model's Fp is a multiple of 64 -- and the recorder issues nothing a model could not)
    rows2 = [(2, QKV), (1, OUT), (2, OUT), (2, FFIN), (8, LNGEMV), (2, LNGEMV)]
    assert seen["dec2_kernel"] == {("omlm_bf16", "float", *f) for f in rows2 + [(6, LNGEMV)]} | both(*[("h16", *f) for f in rows2])
    # the matrix-core kernels: all nine forms, each alone and as the GRP instantiation of a call of more than 16 samples
    plain = [(8, QKV, 0), (8, LNGEMV, 0), (8, FFIN, 0), (6, LNGEMV, 0), (24, LNGEMV, 0)]
    lo = [(8, FFIN, 1), (6, LNGEMV, 1), (24, LNGEMV, 1), (8, LNGEMV, 1)]
    assert {f[1:] for f in seen["dec4_kernel"]} == {(*f, grp) for f in plain + lo for grp in (0, 1)}
    assert seen["dec4_kernel"] >= {("omlm_bf16", *f, grp) for f in plain for grp in (0, 1)} | {("omlm_f16", *f, grp) for f in lo for grp in (0, 1)}
    messages = {r["refused"]["message"] for r in ROWS if "refused" in r}
    for part in ("null argument block", "decode batch must be 1..64", "decode batches of 9..64 run on the matrix-core kernels only",
                 "decode batches of 17..64 need splitk_ws and splitk_cnt", "decode geometry", "heads", "nsplit must cover Nmax keys",
                 "B * Fp exceeds the LDS budget", "ids required with an embedding table", "kv16 (16-bit K/V cache) needs",
                 "lo planes: 16-bit weights, all three families", "lo planes at B >= 2 run on the matrix-core step kernels",
                 "lo planes: feed-forward width <= 3072", "lo planes: the head needs the LayerNorm partials", "lo planes: all three families ["):
        assert any(part in m for m in messages), part
    assert all(r["refused"]["rc"] == ERR_ARG for r in ROWS if "refused" in r)
    assert sorted(r["id"] for r in ROWS if "refused" in r and r["launches"]) == sorted(LATE)


def test_the_fp16_copy_refuses_other_weights(plan):
    """(not reachable through omlm_decode_step: the bf16 copy forwards fp16 weights as w_dtype 1)"""
    got = run_plan(plan, call(2, 1024, 8, 256, 0, fp16_copy=True, pos_dev=True, parts=True))
    assert (got["rc"], got["msg"], got["launches"]) == (ERR_ARG, "bad argument: the fp16 copy serves fp16 weights only [a->w_dtype == 1]", [])


def _header_macros(tmp_path, cases):
    """OMLM_DECODE_LN_PARTS_B, _SPLITK_FLOATS_B, _SPLITK_CNT_B of include/omlm.h at (B, D, Fp)"""
    src = tmp_path / "sizes.c"
    lines = ['#include <stdio.h>', f'#include "{os.path.join(ROOT, "include", "omlm.h")}"', 'static const int c[][3] = {']
    lines += [f"{{{B}, {D}, {Fp}}}," for B, D, Fp in cases]
    lines += ['};', 'int main(void) {', '  for (unsigned i = 0; i < sizeof(c) / sizeof(c[0]); ++i)',
              '    printf("%d %d %d\\n", (int)OMLM_DECODE_LN_PARTS_B(c[i][0], c[i][1], c[i][2]), (int)OMLM_DECODE_SPLITK_FLOATS_B(c[i][0], c[i][1]), '
              '(int)OMLM_DECODE_SPLITK_CNT_B(c[i][0], c[i][1]));', '  return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    return [[int(v) for v in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]


BS, DS, HS, FPS = range(1, 66), (64, 96, 512, 1024, 1056), (1, 2, 8, 9, 16, 17), (64, 256, 2752, 3072, 3104, 4096, 4160)


def _model(D, H, Fp):
    """what decode._geometry reads of a model"""
    ff = types.SimpleNamespace(inner_dim=Fp)
    return types.SimpleNamespace(transformer=types.SimpleNamespace(dim=D, heads=H, layers=[(None, None, ff)], non_causal_prefix_size=0))


def test_python_mirror_equals_the_plan(plan, tmp_path):
    """decode.py's route, limits and scratch sizes over the grid, with the scratch and partial pointers given as CachedDecoder gives them."""
    from open_musiclm_amd import decode, engine
    sizes = (C.c_longlong * 3)()
    macros = iter(_header_macros(tmp_path, [(B, D, Fp) for B in BS for D in DS for Fp in FPS]))
    for B, D, Fp in itertools.product(BS, DS, FPS):
        plan.omlm_plan_decode_scratch(B, D, Fp, sizes)
        s = decode.scratch_sizes(B, D, Fp)
        assert [s["ln_parts"], s["splitk_ws"], s["splitk_cnt"]] == list(sizes) == next(macros), (B, D, Fp)
    n = {r: 0 for r in ROUTES + (None,)}
    out, msg = (C.c_longlong * (16 + 16 * 11))(), C.create_string_buffer(320)
    for D, H, Fp, w16 in itertools.product(DS, HS, FPS, (False, True)):
        mb, mcb = decode.step_max_batch(D, H, Fp, w16), decode.step_max_batch(D, H, Fp, w16, wide=True)
        assert (mb, mcb) == (plan.omlm_plan_decode_max_batch(D, H, Fp, w16, 0), plan.omlm_plan_decode_max_batch(D, H, Fp, w16, 1)), (D, H, Fp, w16)
        heads_ok = 1 <= H <= decode.MAX_DECODE_HEADS
        model, precision = (_model(D, H, Fp), "bf16" if w16 else "bf16x3") if Fp % 64 == 0 else (None, None)       # (a model's Fp is a multiple of 64)
        if model is not None:
            assert (decode.max_batch(model, precision), decode.max_call_batch(model, precision)) == (mb, mcb)
        for B in BS:
            lo_ok = decode.step_lo_planes_ok(B, D, H, Fp)
            assert lo_ok == bool(plan.omlm_plan_decode_lo_planes_ok(B, D, H, Fp, 1, 1)), (B, D, H, Fp)
            if model is not None and w16:
                assert decode.lo_planes_ok(model, B) == (lo_ok and Fp <= 4096)
            for lo in ((False, True) if w16 and lo_ok else (False,)):
                # the pointers as CachedDecoder gives them: every scratch, head and advance, the lo planes only where lo_planes_ok
                plan.omlm_plan_decode(call(B, D, H, Fp, int(w16), L=6, V1=1025, pos_dev=True, parts=True, ids=True, emb_table=True, head_W=True,
                                           ln_parts=True, splitk_ws=True, splitk_cnt=True, W1p_lo=lo, W2p_lo=lo, head_W_lo=lo, advance_pos=True), out, msg)
                for wide in (False, True):
                    route = decode.step_route(B, D, H, Fp, w16, wide)
                    assert (route is not None) == (B <= (mcb if wide else mb)), (B, D, H, Fp, w16, wide)
                    served = heads_ok and route is not None
                    if served:
                        assert out[0] == 0 and ROUTES[out[1]] == route, (B, D, H, Fp, w16, wide, msg.value)
                    elif wide or B > mcb or not heads_ok:          # (not wide: the plan takes the batches of a wide call as well)
                        assert out[0] == ERR_ARG, (B, D, H, Fp, w16, wide)
                    if model is not None:
                        assert decode.supports(model, B, precision, wide=wide) == served
                    n[route if served else None] += 1
    assert min(n.values()) > 100, n


def test_plan_lds_fits_the_workgroup_over_the_grid(plan):
    """every launch of every served call of the grid: at most the 160 KiB its instantiation opted in to"""
    worst = 0
    for B, D, H, Fp, w16, scratch, lo in itertools.product((1, 2, 8, 9, 16, 17, 64), DS, HS, FPS, (0, 1), (False, True), (False, True)):
        got = run_plan(plan, call(B, D, H, Fp, w16, pos_dev=True, parts=True, head_W=True, ln_parts=scratch, splitk_ws=scratch, splitk_cnt=scratch,
                                  W1p_lo=lo, W2p_lo=lo, head_W_lo=lo))
        if got["rc"] == 0:
            worst = max([worst] + [l["lds"] for l in got["launches"] + [got["q_rest"]]])
    assert 100 * 1024 < worst <= 160 * 1024
