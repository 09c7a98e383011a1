"""Route table of the attention family: which launches each omlm_mqa_attn_fwd / _bwd call makes, recorded from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tools/attn_route_calls.py calls.json
    python tools/attn_route_calls.py --merge calls.json DIR/*/r_kernel_trace.csv tests/attn_routes.json "recorded from <sha> on an MI355X"

The first form issues every call of calls() once (zero operands: a route depends on shapes and on which pointers are null, never on
values), each between two sentinel launches of tools/gemm_route_calls.py, and writes the calls it made -- for a refused call the return code and
the omlm_last_error text -- and the values of the three pure size / limit exports over a grid.  The second form cuts the trace at the
sentinels and stores per call the launches whose kernel name contains "attn" or "a3_": name, grid (x, y, z in workgroups), workgroup.
tests/test_attn_plan_host.py checks csrc/attn_plan.h against that table without a GPU; the table comes from the commit BEFORE a change to
the plan, never from the code under test.

Every operand is allocated at its real size, refused calls included.  Calls go through ops.attn_fwd / ops.attn_bwd where ops can express
them; the forms it cannot (no table at all, a raw causal table without its prepared form, a ceiling ops refuses itself) go through hip.lib().
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_route_calls import cut_trace, sentinel  # noqa: E402

BENCH = dict(B=32, N=1116, H=8)


def c(id, dir, dt, B, N, H, P=0, bias="T", **kw):
    """bias: "T" a prepared AttnBias (table + tableT), "zeroT" the all-zero prepared table of no bias, "raw" the raw table alone,
    "none" no table at all.  Backward: dbias (with "T" / "raw"), ws=False the null workspace, split=True dk / dv in two allocations.
    drop: dropout p."""
    return dict(id=id, dir=dir, dt=dt, B=B, N=N, H=H, P=P, bias=bias, **kw)


def calls():
    h, b, f = "float16", "bfloat16", "float32"
    r = []
    for dt in (h, b):
        r += [c(f"fwd/{dt} bench biasT", "fwd", dt, **BENCH), c(f"fwd/{dt} bench no bias", "fwd", dt, **BENCH, bias="none"),
              c(f"fwd/{dt} bench dropout", "fwd", dt, **BENCH, drop=0.1)]
    r += [c(f"fwd/prefix N={n} P={p}", "fwd", b, 2, n, 8, P=p) for n, p in ((77, 14), (77, 100), (1116, 216), (2016, 14), (2017, 14))]
    r += [c("fwd/prefix raw table", "fwd", b, 2, 77, 8, P=14, bias="raw"), c("fwd/prefix dropout", "fwd", h, 2, 77, 8, P=14, drop=0.1),
          c("fwd/prefix first-generation dropout", "fwd", b, 2, 77, 8, P=14, bias="raw", drop=0.1)]
    r += [c(f"fwd/long N={n}", "fwd", b, 1, n, 2) for n in (4096, 4097, 9536, 9537, 16384)]
    r += [c("fwd/long dropout", "fwd", h, 1, 4097, 2, drop=0.1), c("fwd/long no bias", "fwd", b, 1, 4097, 2, bias="none"),
          c("fwd/raw table N=77", "fwd", b, 2, 77, 8, bias="raw"), c("fwd/raw table dropout", "fwd", b, 2, 77, 8, bias="raw", drop=0.1),
          c("fwd/raw table N=9216", "fwd", b, 1, 9216, 2, bias="raw")]
    r += [c(f"fwd/fp32 N={n}", "fwd", f, 1, n, 2) for n in (77, 1116, 8192)]
    r += [c("fwd/fp32 dropout", "fwd", f, 2, 77, 8, drop=0.1), c("fwd/fp32 prefix", "fwd", f, 2, 77, 8, P=14),
          c("fwd/fp32 prefix dropout", "fwd", f, 2, 77, 8, P=14, drop=0.1)]
    r += [c("fwd/refused fp32 N=8224", "fwd", f, 1, 8224, 2), c("fwd/refused N=16385", "fwd", b, 1, 16385, 2),
          c("fwd/prefix N=4097 P=14", "fwd", b, 1, 4097, 2, P=14), c("fwd/refused prefix N=9248 P=14", "fwd", b, 1, 9248, 2, P=14),
          c("fwd/refused raw table N=9248", "fwd", b, 1, 9248, 2, bias="raw")]

    r += [c("bwd/bench dbias + workspace", "bwd", h, **BENCH, dbias=True), c("bwd/bench dbias, null workspace", "bwd", h, **BENCH, dbias=True, ws=False),
          c("bwd/bench no dbias", "bwd", h, **BENCH), c("bwd/bench dk dv apart", "bwd", b, **BENCH, dbias=True, split=True),
          c("bwd/bench dropout", "bwd", b, **BENCH, dbias=True, drop=0.1), c("bwd/bench no bias", "bwd", b, **BENCH, bias="none")]
    r += [c("bwd/N=2048", "bwd", b, 1, 2048, 8, dbias=True), c("bwd/N=2049", "bwd", b, 1, 2049, 8, dbias=True),
          c("bwd/N=2049 dropout", "bwd", b, 1, 2049, 8, dbias=True, drop=0.1),
          c("bwd/N=31", "bwd", b, 2, 31, 8, dbias=True), c("bwd/N=31 dropout", "bwd", b, 2, 31, 8, dbias=True, drop=0.1),
          c("bwd/N=32", "bwd", b, 2, 32, 8, dbias=True), c("bwd/H=9", "bwd", b, 2, 1116, 9, dbias=True),
          c("bwd/B=8 N=1817 H=16", "bwd", b, 8, 1817, 16, dbias=True),
          c("bwd/raw table", "bwd", b, 2, 77, 8, bias="raw", dbias=True), c("bwd/raw table dropout", "bwd", b, 2, 77, 8, bias="raw", dbias=True, drop=0.1)]
    r += [c(f"bwd/prefix N={n} P={p}", "bwd", b, 2, n, 8, P=p, dbias=True) for n, p in ((77, 14), (1116, 216), (2017, 14))]
    r += [c("bwd/prefix dropout", "bwd", h, 2, 77, 8, P=14, dbias=True, drop=0.1),
          c("bwd/prefix raw table", "bwd", b, 2, 77, 8, P=14, bias="raw", dbias=True),
          c("bwd/prefix raw table dropout", "bwd", b, 2, 77, 8, P=14, bias="raw", dbias=True, drop=0.1),
          c("bwd/prefix N=4320 P=14 H=7", "bwd", b, 1, 4320, 7, P=14, dbias=True),
          c("bwd/refused prefix N=4320 P=14 H=8", "bwd", b, 1, 4320, 8, P=14, dbias=True)]
    r += [c("bwd/long N=4097 workspace", "bwd", b, 1, 4097, 1, dbias=True), c("bwd/long N=4097 null workspace", "bwd", b, 1, 4097, 1, dbias=True, ws=False),
          c("bwd/long N=4097 dropout", "bwd", h, 1, 4097, 1, dbias=True, drop=0.1),
          c("bwd/long N=4097 dropout, null workspace", "bwd", h, 1, 4097, 1, dbias=True, ws=False, drop=0.1),
          c("bwd/long N=8229 H=9", "bwd", b, 1, 8229, 9, dbias=True), c("bwd/long N=16384 B=2 H=8", "bwd", b, 2, 16384, 8, dbias=True),
          c("bwd/refused N=16385", "bwd", b, 1, 16385, 1, dbias=True)]
    r += [c("bwd/fp32 N=1116 H=8", "bwd", f, 2, 1116, 8, dbias=True), c("bwd/fp32 B=8 N=1817 H=16", "bwd", f, 8, 1817, 16, dbias=True),
          c("bwd/fp32 dropout", "bwd", f, 2, 77, 8, dbias=True, drop=0.1), c("bwd/fp32 prefix", "bwd", f, 2, 77, 8, P=14, dbias=True),
          c("bwd/fp32 prefix dropout", "bwd", f, 2, 77, 8, P=14, dbias=True, drop=0.1),
          c("bwd/fp32 N=3808", "bwd", f, 1, 3808, 2, dbias=True), c("bwd/refused fp32 N=3840", "bwd", f, 1, 3840, 2, dbias=True)]
    # the 32-bit offset rule of the third-generation dK / dV kernel: B N H = 2^25
    r += [c("bwd/B N H = 2^25 zero prepared table", "bwd", b, 64, 512, 1024, bias="zeroT"),
          c("bwd/refused B N H = 2^25 no table", "bwd", b, 64, 512, 1024, bias="none"),
          c("bwd/refused B N H = 2^25 N=8192 no table", "bwd", b, 4, 8192, 1024, bias="none")]
    return r


def issue(k, dev):
    """the call; returns None, or (return code, message) of a refusal"""
    import torch
    from open_musiclm_amd import hip, ops
    tt = getattr(torch, k["dt"])
    B, N, H, P = k["B"], k["N"], k["H"], k["P"]
    Pn = min(P, N)
    z = lambda *s, t=torch.float32: torch.zeros(*s, dtype=t, device=dev)
    q, kk, v, out = z(B * N, H * 64, t=tt), z(B * N, 64, t=tt), z(B * N, 64, t=tt), z(B * N, H * 64, t=tt)
    lse = z(B, H, N)
    table = z(N + max(Pn - 1, 0), H) if k["bias"] in ("T", "raw") else None
    bias = table
    if k["bias"] == "T":
        one = torch.ones(64, device=dev)
        bias = ops.AttnBias.group(table, N, H, dev, [one], [one], half=k["dt"] == "float16", P=P)[0]
    elif k["bias"] == "zeroT":
        bias = ops.AttnBias(None, N, H, dev)
    drop = dict(p=k.get("drop", 0.0), seed=1)
    # what ops cannot express: no table at all and a raw causal table alone (it prepares one), the ceiling it refuses itself
    direct = (k["bias"] == "none" or (k["bias"] == "raw" and P == 0) or (P == 0 and k["dt"] != "float32" and N > 16384))
    tableT = bias.tableT if isinstance(bias, ops.AttnBias) else None
    ld = table.shape[-1] if table is not None else 0
    if k["dir"] == "bwd":
        dout, delta, dq = z(B * N, H * 64, t=tt), z(B, H, N), z(B * N, H * 64)
        dkv = z(2, B * N, 64)
        dk, dv = (dkv[0], z(B * N, 64)) if k.get("split") else (dkv[0], dkv[1])
        dbias = torch.zeros_like(table) if k.get("dbias") else None
        ws = ops._dbias_workspace(B, N, H, dev) if dbias is not None and k.get("ws", True) else None
    torch.cuda.synchronize()
    MARK()
    try:
        if not direct:
            if k["dir"] == "fwd":
                ops.attn_fwd(q, kk, v, bias, None, out, lse, B, N, H, 8.0, P=P, **drop)
            else:
                ops.attn_bwd(q, kk, v, bias, None, out, dout, lse, delta, dq, dk, dv, dbias, B, N, H, 8.0, P=P, workspace=k.get("ws", True), **drop)
        elif k["dir"] == "fwd":
            hip.call("omlm_mqa_attn_fwd", hip.ptr(q), hip.ptr(kk), hip.ptr(v), hip.ptr(table), hip.ptr(tableT), None, hip.ptr(out), hip.ptr(lse),
                     B, N, H, 8.0, ld, ops.dcode(tt), P, drop["p"], 1, None, hip.stream_ptr())
        else:
            hip.call("omlm_mqa_attn_bwd", hip.ptr(q), hip.ptr(kk), hip.ptr(v), hip.ptr(table), hip.ptr(tableT), None, hip.ptr(out), hip.ptr(dout),
                     hip.ptr(lse), hip.ptr(delta), hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.ptr(dbias), hip.ptr(ws), B, N, H, 8.0, ld,
                     ops.dcode(tt), P, drop["p"], 1, None, hip.stream_ptr())
    except RuntimeError as e:
        m = re.match(r"omlm_mqa_attn_\w+ failed \(rc=(-?\d+)\): (.*)", str(e), re.S)
        if not m:
            raise
        return int(m.group(1)), m.group(2)
    finally:
        MARK()                                                 # what follows in the trace is the next call's preparation
        torch.cuda.synchronize()
    return None


NS = sorted({n + d for n in (32, 64, 77, 128, 1116, 1817, 1856, 2016, 2040, 2048, 3808, 3840, 4000, 4064, 4096, 4320, 4400, 8192, 8224, 8229, 9216,
                            9248, 9536, 16384, 16416) for d in (-1, 0, 1)} | set(range(1, 16417, 257)))
HS, BS = (1, 7, 8, 9, 16), (1, 2, 32)
PS = ("0", "1", "14", "216", "N", "N+5")


def prefix_rows(p, n):
    return n if p == "N" else n + 5 if p == "N+5" else int(p)


def sizes():
    """the three pure host exports over the grid"""
    from open_musiclm_amd import hip
    L = hip.lib()
    return dict(N=NS, H=HS, B=BS, P=PS,
                table_floats=[[[int(L.omlm_attn_bias_table_floats(n, h, prefix_rows(p, n))) for p in PS] for h in HS] for n in NS],
                workspace_bytes=[[[int(L.omlm_mqa_attn_bwd_workspace_bytes(b, n, h)) for h in HS] for n in NS] for b in BS],
                # P over the same values as N (and 0, -1); dtype codes 0 fp32, 1 bf16, 2 fp16, 3 none
                max_positions={str(d): [int(L.omlm_attn_max_positions(d, p)) for p in [-1, 0] + NS] for d in (0, 1, 2, 3)})


def run(out):
    global MARK
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    dev = torch.device("cuda:0")
    MARK = sentinel(dev)
    done = calls()
    for k in done:
        r = issue(k, dev)
        if r is not None:
            k["refused"] = dict(rc=r[0], message=r[1])
        torch.cuda.empty_cache()
        print(k["id"], "refused" if r else "served", flush=True)
    json.dump(dict(calls=done, sizes=sizes()), open(out, "w"), indent=0)
    print(f"{len(done)} calls issued")


def merge(calls_json, trace_csv, out, source):
    rec = json.load(open(calls_json))
    done = rec["calls"]
    segs = cut_trace(trace_csv, lambda name: "attn" in name or "a3_" in name)
    assert len(segs) == 2 * len(done), (len(segs), len(done))
    segs = segs[0::2]                                          # a sentinel in front of each call and one behind it
    for k, seg in zip(done, segs):
        assert not (seg and "refused" in k), k["id"]
        if "refused" not in k:
            k["launches"] = [dict(kernel=r["Kernel_Name"], workgroup=int(r["Workgroup_Size_X"]),
                                  grid=[int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]) for r in seg]
    json.dump(dict(source=source, rows=done, sizes=rec["sizes"]), open(out, "w"), indent=0)
    print(f"{len(done)} rows, {sum(len(s) for s in segs)} launches -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:6])
    else:
        run(sys.argv[1])
