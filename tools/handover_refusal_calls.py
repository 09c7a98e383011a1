"""Refusals of the twice-compiled families' C entries, recorded through the real library without a GPU.

    python tools/handover_refusal_calls.py LIBRARY tests/handover_refusals.json "recorded from <sha>"

For every public entry of the GEMM, ConvFeedForward-middle, attention and decode families and for the dtype codes 1 (bf16), 2 (fp16: the bf16
copy of the library hands the call to its fp16 copy) and 3 (no type), this issues calls that end before any launch -- every pointer null at
non-empty sizes, each bad scalar the entry tests for, and an empty call -- and writes the return code and the omlm_last_error text of each.
tests/test_copy_handover_host.py replays the table against the library under test: a refusal must keep its code, its text and its place
among the other checks of its entry in whichever copy answers.  The table comes from the commit BEFORE a change to the hand-over, never from
the code under test.

The argument names come from include/omlm.h, the ctypes types from open_musiclm_amd.hip.SIGNATURES.  No call reaches a launch: a return code
of -2 (a failed launch) is an error of this tool.
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_musiclm_amd.hip import SIGNATURES, vp  # noqa: E402

CODES = (1, 2, 3)
# arguments that carry a dtype code, per entry (the mx forwards take none: fp16 only)
DTYPE_ARGS = ("dtype", "in_dtype", "out_dtype")
SIZES = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ldcin=64, a_rows=64, b_rows=64, nseq=32, F=60, Fp=64, B=2, H=2, bias_ld=2, scale=0.125,
             alpha=1.0, eps=1e-5, groups=1, ldnorm=1, ldc2=64, count=1, h2_8_stride=64 * 2 * 64, a_plane_bytes=64 * 64 * 2, b_plane_bytes=64 * 64 * 2)
EMPTY = dict(M=0, N=0, B=0, count=0)
ENTRIES = ("omlm_gemm", "omlm_gemm_qknorm", "omlm_gemm_planes16", "omlm_gemm_planes", "omlm_gemm_wgrad_group",
           "omlm_ffmid_fwd", "omlm_ffmid_fwd_seg", "omlm_ffmid_fwd_planes", "omlm_ffmid_fwd_planes_seg", "omlm_ffmid_fwd_mx", "omlm_ffmid_fwd_mx_seg",
           "omlm_ffmid_bwd", "omlm_mqa_attn_fwd", "omlm_mqa_attn_bwd")
DECODE = ("omlm_decode_step", "omlm_decode_step_masked")
# the first ten members of omlm_decode_args (include/omlm.h): int B, D, H, L, F, Fp, Nmax, w_dtype, round_bf16, nsplit
DECODE_INTS = dict(B=2, D=1024, H=8, L=1, F=2730, Fp=2752, Nmax=64, w_dtype=1, round_bf16=1, nsplit=1)
DECODE_BLOCK_BYTES = 1024                                      # more than sizeof(omlm_decode_args); everything behind the ints stays zero


def arg_names(header):
    """entry -> argument names, from the prototypes of include/omlm.h"""
    names = {}
    for m in re.finditer(r"^(?:int|long long) (omlm_\w+)\(([^;]*?)\);", header, re.M | re.S):
        names[m.group(1)] = [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(2).split(",")] if m.group(2).strip() not in ("", "void") else []
    return names


_KEEP = []                                                     # buffers that stand in for device memory (never read: no call launches)


def buffer(offset=0):
    """an address 16-byte aligned (+ offset)"""
    raw = C.create_string_buffer(4096 + 32)
    _KEEP.append(raw)
    return (C.addressof(raw) + 15) // 16 * 16 + offset


def cases(entry, names):
    """(label, {argument: value}) of the calls of one entry for one dtype code; pointers not named are null"""
    ptrs = [n for n, t in zip(names, SIGNATURES[entry]) if t is vp and n != "stream"]
    given = {n: buffer() for n in ptrs if not (n == "workspace" and "workspace_bytes" in names)}        # (a tail workspace comes with its size)
    out = [("every pointer null", {}), ("empty", dict(EMPTY))]
    bad = []
    if "P" in names:
        bad += [("P < 0", dict(P=-1)), ("dropout p = 1", dict(p=1.0)), ("bias_ld < H", dict(given, bias_ld=1)), ("H = 0", dict(given, H=0))]
    if "workspace_bytes" in names:
        bad += [("misaligned tail workspace", dict(workspace=buffer(8), workspace_bytes=1024)), ("tail workspace without its size", dict(workspace=buffer()))]
    if entry == "omlm_gemm":
        bad += [("out_dtype 1 (bf16)", dict(out_dtype=1)), ("out_dtype 3", dict(given, out_dtype=3)), ("K = 0", dict(given, K=0)), ("lda = 60", dict(given, lda=60)),
                ("K = 60", dict(given, K=60))]
    if entry == "omlm_gemm_qknorm":
        bad += [("N = 96", dict(given, N=96)), ("K = 60", dict(given, K=60)), ("c2_col0 = 8", dict(given, c2_col0=8))]
    if entry == "omlm_gemm_planes16":
        bad += [("residual with plane output", dict(given)), ("null lo plane", dict(given, A_lo=None))]
    if entry == "omlm_gemm_planes":
        bad += [("plane stride 0", dict(given, a_plane_bytes=0)), ("k-row map on a plane", dict(given, a_kmajor=1))]
    if "n_full" in names:
        bad += [("n_full / p0 that do not add up", dict(given, n_full=48, p0=8)), ("p0 = 0", dict(given, n_full=32, p0=0))]
    if "nseq" in names:                                        # (only what the entry at hand refuses: nothing here may reach a launch)
        fwd, planes = "eps" in names, "h1_lo" in names
        bad += [("Fp = 60", dict(given, Fp=60)), ("Fp < F", dict(given, F=72)), ("M no multiple of nseq", dict(given, M=65))]
        if fwd:
            bad += [("dropout p = 1", dict(given, p=1.0))]
        if planes:
            bad += [("dropout without keep bits", dict(given, p=0.5, drop_bits=None)), ("misaligned plane", dict(given, h1_lo=buffer(8)))]
        if "du_tmp" in names:
            bad += [("misaligned du_tmp", dict(given, du_tmp=buffer(4), gh=buffer()))]
        if "h2_8_stride" in names:
            bad += [("small fp8 plane stride", dict(given, h2_8_stride=64)), ("Fp = 8", dict(given, F=8, Fp=8, h2_8_stride=64 * 2 * 8))]
    return out + bad


def run_entry(lib, entry, names, code):
    rows = []
    for label, over in cases(entry, names):
        vals = []
        for n, t in zip(names, SIGNATURES[entry]):
            v = over.get(n, None if t is vp else code if n in DTYPE_ARGS else SIZES.get(n, 0))
            vals.append(t(v) if v is not None else None)
        lib.omlm_set_error(b"")
        rc = getattr(lib, entry)(*vals)
        rows.append(dict(entry=entry, code=code, case=label, rc=rc, message=(lib.omlm_last_error() or b"").decode() if rc else ""))
    return rows


def wgrad_cases(lib, code):
    """omlm_gemm_wgrad_group: its descriptors are a struct array (include/omlm.h: A B C c_map, then M N K lda ldb ldc)"""
    class Desc(C.Structure):
        _fields_ = [("A", vp), ("B", vp), ("C", vp), ("c_map", vp)] + [(n, C.c_int) for n in ("M", "N", "K", "lda", "ldb", "ldc")]
    rows = []
    for label, d, count in (("null descriptor array", None, 1), ("empty", None, 0), ("count < 0", None, -1),
                            ("null problem", Desc(None, None, None, None, 64, 64, 64, 64, 64, 64), 1),
                            ("M = 0", Desc(buffer(), buffer(), buffer(), None, 0, 64, 64, 64, 64, 64), 1),
                            ("lda = 60", Desc(buffer(), buffer(), buffer(), None, 64, 64, 64, 60, 64, 64), 1),
                            ("misaligned A", Desc(buffer(8), buffer(), buffer(), None, 64, 64, 64, 64, 64, 64), 1)):
        lib.omlm_set_error(b"")
        rc = lib.omlm_gemm_wgrad_group(C.byref(d) if d is not None else None, count, 0, code, None)
        rows.append(dict(entry="omlm_gemm_wgrad_group", code=code, case=label, rc=rc, message=(lib.omlm_last_error() or b"").decode() if rc else ""))
    return rows


def decode_cases(lib, entry, code):
    rows = []
    masked = entry.endswith("_masked")
    for label, ints in (("null block", None), ("every pointer null", {}), ("B = 0", dict(B=0)), ("B = 65", dict(B=65)), ("D = 100", dict(D=100))):
        block = None
        if ints is not None:
            block = (C.c_int * (DECODE_BLOCK_BYTES // 4))()
            for i, (n, v) in enumerate(dict(DECODE_INTS, w_dtype=code, **ints).items()):
                block[i] = v
        lib.omlm_set_error(b"")
        rc = lib.omlm_decode_step_masked(block, None, None, None) if masked else lib.omlm_decode_step(block, None, None)
        rows.append(dict(entry=entry, code=code, case=label, rc=rc, message=(lib.omlm_last_error() or b"").decode() if rc else ""))
    return rows


def record(lib_path):
    lib = C.CDLL(lib_path)
    for name in ENTRIES + DECODE + ("omlm_set_error", "omlm_last_error"):
        getattr(lib, name).argtypes = SIGNATURES[name]
    lib.omlm_last_error.restype = C.c_char_p
    lib.omlm_set_error.restype = None
    names = arg_names(open(os.path.join(ROOT, "include", "omlm.h")).read())
    rows = []
    for code in CODES:
        for entry in ENTRIES:
            assert len(names[entry]) == len(SIGNATURES[entry]), entry
            rows += wgrad_cases(lib, code) if entry == "omlm_gemm_wgrad_group" else run_entry(lib, entry, names[entry], code)
        for entry in DECODE:
            rows += decode_cases(lib, entry, code)
    assert all(r["rc"] in (0, -1, -3) for r in rows), [r for r in rows if r["rc"] not in (0, -1, -3)]
    return rows


if __name__ == "__main__":
    lib_path, out_path, source = sys.argv[1:4]
    rows = record(lib_path)
    json.dump(dict(source=source, rows=rows), open(out_path, "w"), indent=0)
    print(f"{len(rows)} calls, {sum(1 for r in rows if r['rc'])} refused, {len({r['message'] for r in rows if r['rc']})} distinct texts")
