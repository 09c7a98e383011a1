"""Route table of the GEMM family: which launches each library call makes, recorded from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tools/gemm_route_calls.py calls.json
    python tools/gemm_route_calls.py --merge calls.json DIR/*/r_kernel_trace.csv tests/gemm_routes.json "recorded from <sha> on an MI355X"

The first form issues every call of CALLS once through `ops` (zero operands: a route depends on shapes, never on values), each behind a
sentinel launch (omlm_split_planes of 8 floats: one 256-thread workgroup), and writes the calls it made.  The second form cuts the trace at
the sentinels and stores per call the launches whose kernel name contains "gemm": (name, grid x, grid y, workgroup, and the LDS size
as the trace reports it: 0 for dynamic LDS on this ROCm).
tests/test_gemm_plan_host.py checks csrc/gemm_plan.h against that table without a GPU; the table comes from the commit BEFORE a change to
the planner, never from the code under test.

The shapes are the real ones of a coarse-small training step at B = 32, N = 1116 (M = 35 712 rows; 9600 / 9632 rows per logit head): a
route is a function of the shape against 256 CUs, so stand-ins would take other routes.
"""
import csv
import json
import os
import sys

M, D, FP2, FP, F, HD, V1, LDV = 35712, 1024, 5504, 2752, 2730, 512, 1025, 1032
H16 = ("float16", "bfloat16")


def g(id, dt, m, n, k, out=None, **kw):
    return dict(id=id, entry="gemm", dt=dt, M=m, N=n, K=k, out=out or dt, **kw)


def step_calls(dt):
    """every distinct GEMM call of one training step with 16-bit operands `dt` (fp16ff: float16) or fp32 operands (bf16x3)"""
    x3 = dt == "float32"
    p = {"float16": "fp16ff", "bfloat16": "bf16", "float32": "bf16x3"}[dt]
    c = []
    if x3:
        c += [g(f"{p}/q-proj", dt, M, 512, D), g(f"{p}/kv-proj", dt, M, 128, D)]
    else:
        c += [dict(id=f"{p}/q-proj+l2norm", entry="qknorm", dt=dt, M=M, N=512, K=D, groups=8, c2=0),
              dict(id=f"{p}/kv-proj+l2norm", entry="qknorm", dt=dt, M=M, N=128, K=D, groups=1, c2=64)]
    c.append(g(f"{p}/to_out", dt, M, D, 512, out="float32", cin="sep"))
    if dt == "float16":
        c += [dict(id=f"{p}/FF-in mx16", entry="mx16", dt=dt, M=M, N=FP2, K=D, c_lo="bf8"),
              dict(id=f"{p}/FF-out mx16", entry="mx16", dt=dt, M=M, N=D, K=FP, cin="sep"),
              dict(id=f"{p}/FF-in planes16", entry="planes16", dt=dt, M=M, N=FP2, K=D, c_lo=True),
              dict(id=f"{p}/FF-out planes16", entry="planes16", dt=dt, M=M, N=D, K=FP, cin="sep")]
        for rows in (9600, 9632):
            c.append(dict(id=f"{p}/head {rows} planes16", entry="planes16", dt=dt, M=rows, N=V1, K=D, cin=None, a_map=True, c_map=True, ldc=LDV, a_rows=M))
    else:
        c += [g(f"{p}/FF-in", dt, M, FP2, D), g(f"{p}/FF-out", dt, M, D, FP, out="float32", cin="sep")]
        for rows in (9600, 9632):
            c.append(g(f"{p}/head {rows}", dt, rows, V1, D, out="float32", a_map=True, c_map=True, ldc=LDV, a_rows=M))
    for rows in (9600, 9632):
        c.append(g(f"{p}/d(y) head {rows}", dt, rows, D, LDV, out="float32", bk=True, a_map=True, c_map=True, a_rows=rows, b_rows=V1, c_rows=M))
    c += [g(f"{p}/d(h2)", dt, M, FP, D, bk=True), g(f"{p}/d(xn2)", dt, M, D, FP2, bk=True), g(f"{p}/d(o)", dt, M, 512, D, bk=True),
          g(f"{p}/d(xn)", dt, M, D, 512, bk=True), g(f"{p}/d(x) kv", dt, M, D, 128, bk=True, cin="sep" if x3 else None)]
    wg = [(D, F, M, False), (FP2, D, M, True), (D, 512, M, False), (512, D, M, False), (128, D, M, False)]
    if x3:
        c += [g(f"{p}/dW {m}x{n}", dt, m, n, k, ak=True, bk=True, cin="c", c_map=cm) for m, n, k, cm in wg]
        c.append(g(f"{p}/dW head (k-row maps)", dt, V1, D, 9600, ak=True, bk=True, cin="c", a_map=True, b_map=True, lda=LDV, a_rows=9600, b_rows=M))
    else:
        c.append(dict(id=f"{p}/wgrad group", entry="wgrad_group", dt=dt, probs=[(V1, D, 9600, False), (V1, D, 9600, False), (V1, D, 9664, False)] + wg * 6))
    return c


def calls():
    c = step_calls("float16") + step_calls("bfloat16") + step_calls("float32")
    b, f = "bfloat16", "float32"
    # the rel-pos MLP's fp32 GEMMs on the register-staged kernel: plain (forward) and accumulating (backward: split along K)
    c += [g("relpos/fwd", f, 1116, HD, HD, planes=False), g("relpos/fwd last", f, 1116, 8, HD, ldc=8, planes=False),
          g("relpos/dW last", f, 8, HD, 1116, ak=True, bk=True, cin="c", lda=8, planes=False),
          g("relpos/dz last", f, 1116, HD, 8, bk=True, lda=8, b_rows=8, planes=False),
          g("relpos/dW", f, HD, HD, 1116, ak=True, bk=True, cin="c", planes=False),
          g("relpos/dz", f, 1116, HD, HD, bk=True, cin="c", planes=False)]
    c += [g("kmap/dW head (k-row maps, 128x128)", b, V1, D, 9600, out=f, ak=True, bk=True, cin="c", a_map=True, b_map=True, lda=LDV, a_rows=9600, b_rows=M),
          g("ragged-K", b, 4096, D, 1000)]
    # one call per arm of the tile rule that the step above does not take (forced tiles: below)
    c += [g("tile/256x128 (M >= 2048, 512 < N < 1024)", b, M, 768, D), g("tile/256x256 (N >= 2048, M < 1024)", b, 512, 4096, D),
          g("tile/128x128 (nothing else applies)", b, 512, 512, D),
          g("peel/none (last round more than half full: 400 tiles)", b, 25600, D, D)]
    # each hook in its non-default state on the shape where it changes the route
    c += [g("hook/PERSIST=0 FF-in", b, M, FP2, D, env={"OMLM_GEMM_PERSIST": "0"}),
          g("hook/PERSIST=0 to_out", b, M, D, 512, out=f, cin="sep", env={"OMLM_GEMM_PERSIST": "0"}),
          dict(id="hook/PERSIST=0 q-proj+l2norm", entry="qknorm", dt=b, M=M, N=512, K=D, groups=8, c2=0, env={"OMLM_GEMM_PERSIST": "0"}),
          g("hook/T8=0 d(xn2)", b, M, D, FP2, bk=True, env={"OMLM_GEMM_T8": "0"}),
          g("hook/T8=1 FF-in", b, M, FP2, D, env={"OMLM_GEMM_T8": "1"}),
          dict(id="hook/T8=0 FF-out planes16", entry="planes16", dt="float16", M=M, N=D, K=FP, cin="sep", env={"OMLM_GEMM_T8": "0"}),
          dict(id="hook/T8=0 wgrad group", entry="wgrad_group", dt=b, probs=[(D, F, M, False), (FP2, D, M, True)], env={"OMLM_GEMM_T8": "0"}),
          g("hook/TILE=128x128 d(xn2)", b, M, D, FP2, bk=True, env={"OMLM_GEMM_TILE": "128x128"}),
          g("hook/TILE=256x256 d(o)", b, M, 512, D, bk=True, env={"OMLM_GEMM_TILE": "256x256"}),
          g("hook/TILE=256x128 d(o)", b, M, 512, D, bk=True, env={"OMLM_GEMM_TILE": "256x128"}),
          g("hook/TAIL_SPLIT=0 d(xn2)", b, M, D, FP2, bk=True, env={"OMLM_GEMM_TAIL_SPLIT": "0"}),
          dict(id="hook/MX_FUSE_TAIL=0 FF-in mx16", entry="mx16", dt="float16", M=M, N=FP2, K=D, c_lo="bf8", env={"OMLM_MX_FUSE_TAIL": "0"})]
    return c


HOOKS = ("OMLM_GEMM_PERSIST", "OMLM_GEMM_T8", "OMLM_GEMM_TILE", "OMLM_GEMM_TAIL_SPLIT", "OMLM_MX_FUSE_TAIL")


def issue(c, dev):
    import torch
    from open_musiclm_amd import ops
    tt = getattr(torch, c["dt"])
    m, n, k = c.get("M"), c.get("N"), c.get("K")
    z = lambda r, cols, t=tt: torch.zeros(r, cols, dtype=t, device=dev)
    arange = lambda cnt: torch.arange(cnt, dtype=torch.int32, device=dev)
    if c["entry"] == "gemm":
        ak, bk = c.get("ak", False), c.get("bk", False)
        lda = c.get("lda", (m + 7) // 8 * 8 if ak else k)
        ldb = (n + 7) // 8 * 8 if bk else k
        ldc = c.get("ldc", n)
        a_rows = c.get("a_rows", k if ak else m)
        b_rows = c.get("b_rows", k if bk else n)
        A, B = z(a_rows, lda), z(b_rows, ldb)
        C = z(c.get("c_rows", m), ldc, getattr(torch, c["out"]))
        cin = C if c.get("cin") == "c" else z(m, ldc, torch.float32) if c.get("cin") == "sep" else None
        ops.gemm(A, B, C, M=m, N=n, K=k, lda=lda, ldb=ldb, ldc=ldc, a_kmajor=ak, b_kmajor=bk, Cin=cin,
                 a_map=arange(k if ak else m) if c.get("a_map") else None, b_map=arange(k if bk else n) if c.get("b_map") else None,
                 c_map=arange(m) if c.get("c_map") else None, a_rows=a_rows, b_rows=b_rows, planes=c.get("planes", True))
    elif c["entry"] == "qknorm":
        C2 = z(m, n - c["c2"]) if c["c2"] else None
        ops.gemm_qknorm(z(m, k), z(n, k), z(m, c["c2"] or n), torch.ones(n, device=dev), torch.empty(m, c["groups"], device=dev), c["groups"],
                        M=m, N=n, K=k, C2=C2, c2_col0=c["c2"])
    elif c["entry"] == "planes16":
        ldc = c.get("ldc", n)
        lo = c.get("c_lo")
        A, B = z(c.get("a_rows", m), k), z(n, k)
        C = z(c.get("a_rows", m) if c.get("c_map") else m, ldc, tt if lo else torch.float32)
        ops.gemm_planes16(A, A.clone(), B, B.clone(), C, C.clone() if lo else None, M=m, N=n, K=k, Cin=z(m, ldc, torch.float32) if c.get("cin") == "sep" else None,
                          a_map=arange(m) if c.get("a_map") else None, c_map=arange(m) if c.get("c_map") else None, ldc=ldc,
                          a_rows=c.get("a_rows"), b_rows=n)
    elif c["entry"] == "mx16":
        lo = c.get("c_lo")
        A, B = z(m, k), z(n, k)
        ops.gemm_mx16(A, ops.Fp8Planes(m, k, dev), B, ops.Fp8Planes(n, k, dev), z(m, n, tt if lo else torch.float32),
                      z(m, n, torch.uint8) if lo else None, M=m, N=n, K=k, Cin=z(m, n, torch.float32) if c.get("cin") == "sep" else None)
    elif c["entry"] == "wgrad_group":
        wg = ops.WgradGroup()
        ops_ = {}                                             # operands by (rows, width): a route depends on no pointer
        for pm, pn, pk, cm in c["probs"]:
            dY = ops_.setdefault((pk, pm), z(pk, (pm + 7) // 8 * 8))
            X = ops_.setdefault((pk, pn), z(pk, (pn + 7) // 8 * 8))
            wg.add(dY, X, ops_.setdefault(("w", pm, pn), z(pm, pn, torch.float32)), M=pm, N=pn, K=pk, c_map=arange(pm) if cm else None)
        wg.flush()
    else:
        raise ValueError(c["entry"])


def sentinel(dev):
    """the launch that marks the start of a call in the trace: omlm_split_planes of 8 floats, one 256-thread workgroup"""
    import torch
    from open_musiclm_amd import hip
    sx, sp = torch.zeros(8, device=dev), torch.zeros(16, dtype=torch.bfloat16, device=dev)
    return lambda: hip.call("omlm_split_planes", hip.ptr(sx), hip.ptr(sp), 8, 8, hip.stream_ptr())


def cut_trace(trace_csv, keep):
    """the trace's rows in start order, cut at the sentinels: per call the rows whose kernel name `keep` accepts"""
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        name = r["Kernel_Name"]
        if "split_planes_kernel" in name and int(r["Grid_Size_X"]) == 256:
            segs.append([])
        elif segs and keep(name):
            segs[-1].append(r)
    return segs


def run(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from open_musiclm_amd import ops
    dev = torch.device("cuda:0")
    mark = sentinel(dev)
    done = calls()
    for c in done:
        for h in HOOKS:
            os.environ.pop(h, None)
        os.environ.update(c.get("env", {}))
        torch.cuda.synchronize()
        mark()
        issue(c, dev)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    json.dump(dict(ws_bytes=ops._TAIL_WS_BYTES, calls=done), open(out, "w"), indent=0)
    print(f"{len(done)} calls issued")


def merge(calls_json, trace_csv, out, source):
    rec = json.load(open(calls_json))
    done = rec["calls"]
    segs = []
    for seg in cut_trace(trace_csv, lambda name: "gemm" in name):
        segs.append([])
        for r in seg:
            wg = int(r["Workgroup_Size_X"])
            segs[-1].append(dict(kernel=r["Kernel_Name"], grid_x=int(r["Grid_Size_X"]) // wg, grid_y=int(r["Grid_Size_Y"]), workgroup=wg,
                                 lds=int(r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", 0)))))
    assert len(segs) == len(done), (len(segs), len(done))
    for c, s in zip(done, segs):
        c["launches"] = s
    json.dump(dict(source=source, ncu=256, persist_slots=256, ws_bytes=rec["ws_bytes"], rows=done), open(out, "w"), indent=0)
    print(f"{len(done)} rows, {sum(len(s) for s in segs)} launches -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:6])
    else:
        run(sys.argv[1])
