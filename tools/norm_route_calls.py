"""Route table of the LayerNorm / qk-norm family: which launches each omlm_layernorm_* / omlm_qk_norm_* call makes, recorded from a kernel trace.

    timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tools/norm_route_calls.py calls.json
    python tools/norm_route_calls.py --merge calls.json DIR/*/r_kernel_trace.csv tests/norm_routes.json "recorded from <sha> on an MI355X"

The first form (a kernel trace only: no counters with it) issues every call of calls() once through hip.lib() (zero operands at their real
sizes: a route depends on sizes, dtype codes and on which pointers are null, never on values), each between two sentinel launches of
tools/gemm_route_calls.py, and writes the calls it made -- for a refused call the return code and the omlm_last_error text.  The second form
cuts the trace at the sentinels and stores per call the launches whose kernel name contains "ln_", "qk_norm" or "colsum": name with template
arguments, grid (x, y in workgroups), workgroup.  tests/test_norm_plan_host.py checks csrc/norm_plan.h against that table without a GPU; the
table comes from the commit BEFORE a change to the plan, never from the code under test.

Shapes are the smallest that reach each arm: the row seams of the grid caps (512, 2048) and of the column sum's split (64, 1024), the widths
on both sides of the row-pair kernels' D = 1024 and of one float4 piece per thread, a segment of B = 2, n_full = 48, p0 = 8.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_route_calls import cut_trace, sentinel  # noqa: E402

F32, B16, F16 = "float32", "bfloat16", "float16"
H16 = (B16, F16)
ALL = (F32, B16, F16)
CODE = {F32: 0, B16: 1, F16: 2}
SEAMS = (1, 80, 511, 512, 513, 2047, 2048, 2049)               # the grid caps of the forward / two-level backward (2048) and of the atomics (512)
SEG = [48, 8, 40]                                              # n_full, p0, n_live; M = 2 * 40
PAIRS = ((F32, F32), (F32, B16), (B16, F32), (B16, B16), (F32, F16), (F16, F32), (F16, F16))       # (cast, dy) of the backward


def k(id, op, dt, M, D=1024, **kw):
    """One call.  op: fwd, planes, mx, bwd, ws_bytes, qk_fwd, qk_bwd, qk_bwd2.  dt: the output / cast / operand dtype; dy (bwd): dy's dtype.
    code / dy_code: the dtype codes where they are not the dtypes'.  ldy: y's pitch (D).  seg: None (the plain entry) or [n_full, p0, n_live]
    (the `_seg` entry).  Which of the optional pointers are given: xcast, stats (mean and rstd), xc, dres, dres2, dxcast, dgamma, ws.  null: a
    required pointer to leave out.  stride (mx): "ok" or "small".  tiny: one-element operands (a call that is refused before any launch)."""
    r = dict(id=id, op=op, dt=dt, dy=dt if dt in H16 else F32, M=M, D=D, H=8, ldy=None, seg=None, code=None, dy_code=None, xcast=False, stats=True,
             xc=False, dres=True, dres2=False, dxcast=True, dgamma=True, ws=True, null=None, stride="ok", tiny=False)
    r.update(kw)
    if r["ldy"] is None:
        r["ldy"] = D
    return r


def fl_of(i):
    return dict(dres=bool(i & 1), dres2=bool(i & 2), dxcast=bool(i & 4))


def calls():
    r = []
    # ---- forward: row seams at both kernels, widths, dtypes, the optional pointers ----
    for D in (1024, 768):
        r += [k(f"fwd/{B16} D={D} M={M}", "fwd", B16, M, D) for M in SEAMS]
    for dt in ALL:
        r += [k(f"fwd/{dt} D={D}", "fwd", dt, 5, D) for D in (4, 768, 1024, 1028, 4096)]
        r += [k(f"fwd/{dt} D={D} cast copy of x", "fwd", dt, 5, D, xcast=True) for D in (768, 1024)]
        r += [k(f"fwd/{dt} D={D} no statistics", "fwd", dt, 5, D, stats=False) for D in (768, 1024)]
        r += [k(f"fwd/{dt} D=1024 no statistics, cast copy of x", "fwd", dt, 5, xcast=True, stats=False),
              k(f"fwd/{dt} D=768 ldy=800", "fwd", dt, 5, 768, ldy=800)]
    r += [k("fwd/dtype code 3 (taken as 16-bit)", "fwd", B16, 5, 768, code=3)]
    for dt in H16:
        for D in (1024, 512):
            r += [k(f"fwd/{dt} D={D} segment", "fwd", dt, 80, D, seg=SEG), k(f"fwd/{dt} D={D} segment, xc", "fwd", dt, 80, D, seg=SEG, xc=True)]
        # ---- planes ----
        r += [k(f"planes/{dt} D={D}", "planes", dt, 5, D) for D in (4, 768, 1024, 1028, 4096)]
        r += [k(f"planes/{dt} D=1024 M={M}", "planes", dt, M) for M in (2047, 2048, 2049)]
        r += [k(f"planes/{dt} D=768 ldy=800", "planes", dt, 5, 768, ldy=800)]
        for D in (1024, 512):
            r += [k(f"planes/{dt} D={D} segment", "planes", dt, 80, D, seg=SEG), k(f"planes/{dt} D={D} segment, xc", "planes", dt, 80, D, seg=SEG, xc=True)]
    # ---- mx (fp16 only): both MAXV ----
    r += [k(f"mx/D={D}", "mx", F16, 5, D) for D in (64, 1024, 1088, 4096)]
    r += [k(f"mx/D=1024 M={M}", "mx", F16, M) for M in (2047, 2048, 2049)]
    r += [k("mx/D=768 ldy=800", "mx", F16, 5, 768, ldy=800)]
    for D in (1024, 512, 2048):
        r += [k(f"mx/D={D} segment", "mx", F16, 80, D, seg=SEG), k(f"mx/D={D} segment, xc", "mx", F16, 80, D, seg=SEG, xc=True)]
    # ---- backward: every FL of the row-pair kernel for every type pair; the general kernel; workspace and dgamma ----
    for cast, dy in PAIRS:
        t = f"bwd/{cast},{dy}"
        r += [k(f"{t} D=1024 FL={i}", "bwd", cast, 80, dy=dy, **fl_of(i)) for i in range(8)]
        r += [k(f"{t} D=768", "bwd", cast, 80, 768, dy=dy, dres2=True)]
        r += [k(f"{t} D={D}", "bwd", cast, 5, D, dy=dy) for D in (4, 1028, 4096)]
    for D in (1024, 768):
        for ws in (True, False):
            r += [k(f"bwd/{B16} D={D} M={M} {'workspace' if ws else 'atomics'}", "bwd", B16, M, D, ws=ws) for M in SEAMS]
            r += [k(f"bwd/{B16} D={D} {'workspace' if ws else 'atomics'}, no dgamma", "bwd", B16, 80, D, ws=ws, dgamma=False)]
        r += [k(f"bwd/{B16} D={D} M={M} workspace (column sum's split)", "bwd", B16, M, D) for M in (63, 64, 1023, 1024)]
    r += [k("bwd/cast dtype code 3 (taken as 16-bit)", "bwd", B16, 80, 768, code=3),
          k("bwd/cast dtype code 3, dy fp32", "bwd", B16, 80, dy=F32, code=3),
          k("bwd/no cast copy, dres2 names the type", "bwd", B16, 80, 768, dxcast=False, dres2=True)]
    for dt in H16:
        r += [k(f"bwd/{dt} D=1024 segment FL={i}", "bwd", dt, 80, seg=SEG, **fl_of(i)) for i in (0, 1, 4, 5)]
        r += [k(f"bwd/{dt} D=512 segment", "bwd", dt, 80, 512, seg=SEG), k(f"bwd/{dt} D=512 segment, atomics", "bwd", dt, 80, 512, seg=SEG, ws=False),
              k(f"bwd/{dt} D=1024 segment, no dgamma", "bwd", dt, 80, seg=SEG, dgamma=False)]
    r += [k(f"ws_bytes/D={D}", "ws_bytes", F32, 0, D) for D in (4, 768, 1024, 4096)]
    # ---- qk-norm ----
    for dt in ALL:
        r += [k(f"qk_fwd/{dt} M={M}", "qk_fwd", dt, M) for M in (1, 150, 6552, 6553, 6554)]            # ceil(10 M / 16) against 4096
        r += [k(f"qk_fwd/{dt} H=6 M={M}", "qk_fwd", dt, M, H=6) for M in (8190, 8192, 8193)]
        r += [k(f"qk_bwd/{dt} M={M}", "qk_bwd", dt, M) for M in (1, 150, 819, 820)]                   # ceil(10 M / 16) against 512
        r += [k(f"qk_bwd/{dt} H=6 M={M}", "qk_bwd", dt, M, H=6) for M in (1022, 1024, 1025)]
    for dt in H16:
        r += [k(f"qk_bwd2/{dt} H=4 M=1", "qk_bwd2", dt, 1, H=4)]                                      # want = 0 -> one workgroup
        r += [k(f"qk_bwd2/{dt} M={M}", "qk_bwd2", dt, M) for M in (1, 150, 8160, 8161, 8192, 8193)]   # (M + 31) / 32 against 256
    # ---- nothing to do ----
    r += [k(f"empty/{op}", op, F16, 0, null="all") for op in ("fwd", "planes", "mx", "bwd", "qk_fwd", "qk_bwd", "qk_bwd2")]
    r += [k(f"empty/{op} segment", op, F16, 0, seg=SEG, null="all") for op in ("fwd", "planes", "bwd")]
    r += [k("empty/mx segment (no segment check)", "mx", F16, 0, seg=[48, 0, 40], null="all")]
    # ---- refusals ----
    for op, dt in (("fwd", F32), ("fwd", B16), ("fwd", F16), ("planes", B16), ("planes", F16), ("mx", F16), ("bwd", F32), ("bwd", B16), ("bwd", F16)):
        t = f"refused/{op} {dt}"
        r += [k(f"{t} null pointer", op, dt, 5, null="gamma"), k(f"{t} D=4100", op, dt, 5, 4100), k(f"{t} D=6", op, dt, 5, 6, ldy=8)]
        if op != "bwd":
            r += [k(f"{t} ldy < D", op, dt, 5, 768, ldy=764)]
        if dt in H16:
            r += [k(f"{t} segment p0=0", op, dt, 80, seg=[40, 0, 40]), k(f"{t} segment M % n_live", op, dt, 81, seg=SEG),
                  k(f"{t} segment p0 + n_live != n_full", op, dt, 80, seg=[50, 8, 40])]
    r += [k("refused/fwd segment, float32 output", "fwd", F32, 80, seg=SEG), k("refused/fwd segment, cast copy of x", "fwd", B16, 80, seg=SEG, xcast=True),
          k("refused/fwd segment, no statistics", "fwd", B16, 80, seg=SEG, stats=False),
          k("refused/fwd last null pointer", "fwd", B16, 5, null="y"),
          k("refused/planes float32 output", "planes", B16, 5, code=0), k("refused/planes dtype code 3", "planes", B16, 5, code=3),
          k("refused/planes ldy % 4", "planes", B16, 5, 768, ldy=770), k("refused/planes no statistics", "planes", B16, 5, stats=False),
          k("refused/planes no lo plane", "planes", F16, 5, null="y_lo"),
          k("refused/mx ldy % 4", "mx", F16, 5, 768, ldy=770), k("refused/mx stride too small", "mx", F16, 5, stride="small"),
          k("refused/mx row pitch D=32", "mx", F16, 5, 32), k("refused/mx row pitch D=60", "mx", F16, 5, 60),
          k("refused/mx no scales", "mx", F16, 5, null="scale8"), k("refused/mx no statistics", "mx", F16, 5, stats=False),
          k("refused/mx segment, n_full=0", "mx", F16, 80, seg=[0, 0, 0]),
          k("refused/bwd dy dtype code 3", "bwd", B16, 80, dy_code=3), k("refused/bwd last null pointer", "bwd", B16, 80, null="dx"),
          k("refused/bwd no statistics", "bwd", F16, 80, stats=False),
          k("refused/bwd segment, dres2", "bwd", B16, 80, seg=SEG, dres2=True), k("refused/bwd segment, float32 cast type", "bwd", F32, 80, dy=B16, seg=SEG),
          k("refused/bwd segment, float32 dy", "bwd", B16, 80, dy=F32, seg=SEG), k("refused/bwd segment, float32 types", "bwd", F32, 80, seg=SEG),
          k("refused/bwd segment D=4100", "bwd", B16, 80, 4100, seg=SEG)]
    for dt in ALL:
        r += [k(f"refused/qk_fwd {dt} null pointer", "qk_fwd", dt, 5, null="q_scale"), k(f"refused/qk_bwd {dt} null pointer", "qk_bwd", dt, 5, null="dk_scale"),
              k(f"refused/qk_bwd {dt} 2^31 vectors", "qk_bwd", dt, 1 << 28, tiny=True)]
    r += [k("refused/qk_bwd2 float32 operands", "qk_bwd2", F32, 5)]
    for dt in H16:
        r += [k(f"refused/qk_bwd2 {dt} null pointer", "qk_bwd2", dt, 5, null="qn"), k(f"refused/qk_bwd2 {dt} 2^31 vectors", "qk_bwd2", dt, 1 << 28, tiny=True)]
    assert len({c["id"] for c in r}) == len(r)
    return r


def issue(c, dev):
    """the call; returns None, (return code, message) of a refusal, or -- ws_bytes -- the value"""
    import torch
    from open_musiclm_amd import hip, ops
    L = hip.lib()
    op, M, D, H, ldy = c["op"], c["M"], c["D"], c["H"], c["ldy"]
    if op == "ws_bytes":
        return int(L.omlm_layernorm_bwd_workspace_bytes(D))
    T, TDY = getattr(torch, c["dt"]), getattr(torch, c["dy"])
    f32, u8 = torch.float32, torch.uint8
    tiny = c["tiny"]
    z = lambda *s, t=f32: torch.zeros(*((1,) if tiny else s), dtype=t, device=dev)
    one = lambda *s: torch.ones(*((1,) if tiny else s), dtype=f32, device=dev)
    rows = max(M, 1)
    n_full, p0, n_live = c["seg"] or (0, 0, 0)
    full = rows // n_live * n_full if c["seg"] and n_live > 0 and n_full > 0 else rows             # rows of the full-size buffers of a segment call
    code = CODE[c["dt"]] if c["code"] is None else c["code"]
    dy_code = CODE[c["dy"]] if c["dy_code"] is None else c["dy_code"]
    seg = (n_full, p0, n_live) if c["seg"] else ()
    sfx = "_seg" if c["seg"] else ""
    if op in ("fwd", "planes", "mx"):
        t = dict(x=z(max(full, rows), D), gamma=z(D), y=z(rows, ldy, t=T), xcast=z(rows, D, t=T), y_lo=z(rows, ldy, t=T), mean=z(rows), rstd=z(rows),
                 xc=z(rows, D))
        if op == "mx":
            P = ops.Fp8Planes(rows, ldy, dev)
            t.update(y8=P.planes, scale8=P.scale)
    elif op == "bwd":
        t = dict(dy=z(rows, D, t=TDY), x=z(rows, D), gamma=z(D), mean=z(rows), rstd=z(rows), dres=z(rows, D), dres2=z(rows, D, t=T), dx=z(max(full, rows), D),
                 dxcast=z(max(full, rows), D, t=T), dgamma=z(D), ws=z(2048 * D))
    elif op == "qk_fwd":
        t = dict(q_raw=z(rows, H * 64), kv_raw=z(rows, 128), q_scale=one(64), k_scale=one(64), q=z(rows, H * 64, t=T), k=z(rows, 64, t=T), v=z(rows, 64, t=T))
    elif op == "qk_bwd":
        t = dict(dq=z(rows, H * 64), dk=z(rows, 64), dv=z(rows, 64), q_raw=z(rows, H * 64), kv_raw=z(rows, 128), q_scale=one(64), k_scale=one(64),
                 dq_raw=z(rows, H * 64, t=T), dkv_raw=z(rows, 128, t=T), dq_scale=z(64), dk_scale=z(64))
    else:
        t = dict(dq=z(rows, H * 64), dk=z(rows, 64), dv=z(rows, 64), q=z(rows, H * 64, t=T), k=z(rows, 64, t=T), qn=one(rows, H), kn=one(rows), q_scale=one(64),
                 k_scale=one(64), dq_raw=z(rows, H * 64, t=T), dkv_raw=z(rows, 128, t=T), dq_scale=z(64), dk_scale=z(64))
    optional = dict(xcast=c["xcast"], mean=c["stats"], rstd=c["stats"], xc=c["xc"], dres=c["dres"], dres2=c["dres2"], dxcast=c["dxcast"], dgamma=c["dgamma"],
                    ws=c["ws"])
    p = lambda name: t[name].data_ptr() if optional.get(name, True) and c["null"] not in (name, "all") else None
    st = hip.stream_ptr()
    torch.cuda.synchronize()
    MARK()
    try:
        if op == "fwd":
            a = (p("x"), p("gamma"), p("y"), p("xcast"), p("mean"), p("rstd")) + ((p("xc"),) if seg else ())
            rc = getattr(L, "omlm_layernorm_fwd" + sfx)(*a, M, D, ldy, 1e-5, code, *seg, st)
        elif op == "planes":
            a = (p("x"), p("gamma"), p("y"), p("y_lo"), p("mean"), p("rstd")) + ((p("xc"),) if seg else ())
            rc = getattr(L, "omlm_layernorm_fwd_planes" + sfx)(*a, M, D, ldy, 1e-5, code, *seg, st)
        elif op == "mx":
            stride = {"ok": P.stride, "small": rows * 2 * ldy - 16}[c["stride"]]
            a = (p("x"), p("gamma"), p("y"), p("y8"), stride, p("scale8"), p("mean"), p("rstd")) + ((p("xc"),) if seg else ())
            rc = getattr(L, "omlm_layernorm_fwd_mx" + sfx)(*a, M, D, ldy, 1e-5, *seg, st)
        elif op == "bwd":
            rc = getattr(L, "omlm_layernorm_bwd2" + sfx)(p("dy"), p("x"), p("gamma"), p("mean"), p("rstd"), p("dres"), p("dres2"), p("dx"), p("dxcast"),
                                                         p("dgamma"), p("ws"), M, D, 1.0, code, dy_code, *seg, st)
        elif op == "qk_fwd":
            rc = L.omlm_qk_norm_fwd(p("q_raw"), p("kv_raw"), p("q_scale"), p("k_scale"), p("q"), p("k"), p("v"), M, H, code, st)
        elif op == "qk_bwd":
            rc = L.omlm_qk_norm_bwd(p("dq"), p("dk"), p("dv"), p("q_raw"), p("kv_raw"), p("q_scale"), p("k_scale"), p("dq_raw"), p("dkv_raw"), p("dq_scale"),
                                    p("dk_scale"), M, H, code, st)
        else:
            rc = L.omlm_qk_norm_bwd2(p("dq"), p("dk"), p("dv"), p("q"), p("k"), p("qn"), p("kn"), p("q_scale"), p("k_scale"), p("dq_raw"), p("dkv_raw"),
                                     p("dq_scale"), p("dk_scale"), M, H, code, st)
    finally:
        MARK()                                                 # what follows in the trace is the next call's preparation
        torch.cuda.synchronize()
    if rc != 0:
        msg = L.omlm_last_error()
        return int(rc), msg.decode() if msg else "?"
    return None


def run(out):
    global MARK
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    dev = torch.device("cuda:0")
    MARK = sentinel(dev)
    done = calls()
    for c in done:
        if c["tiny"]:
            # a call at a size no buffer here has: it may be issued only where its refusal precedes every launch
            assert c["M"] * (c["H"] + 2) >= 1 << 31 and c["op"] in ("qk_bwd", "qk_bwd2")
        r = issue(c, dev)
        if isinstance(r, int):
            c["value"] = r
        elif r is not None:
            c["refused"] = dict(rc=r[0], message=r[1])
        torch.cuda.empty_cache()
        print(c["id"], "refused" if isinstance(r, tuple) else "served", flush=True)
    json.dump(dict(calls=done), open(out, "w"), indent=0)
    print(f"{len(done)} calls issued")


def merge(calls_json, trace_csv, out, source):
    done = json.load(open(calls_json))["calls"]
    segs = cut_trace(trace_csv, lambda name: "ln_" in name or "qk_norm" in name or "colsum" in name)
    traced = [c for c in done if c["op"] != "ws_bytes"]
    assert len(segs) == 2 * len(traced), (len(segs), len(traced))
    segs = segs[0::2]                                          # a sentinel in front of each call and one behind it
    for c in done:
        c["launches"] = []
    for c, seg in zip(traced, segs):
        c["launches"] = [dict(kernel=r["Kernel_Name"], workgroup=int(r["Workgroup_Size_X"]),
                              grid=[int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XY"]) for r in seg]
    json.dump(dict(source=source, rows=done), open(out, "w"), indent=0)
    print(f"{len(done)} rows, {sum(len(s) for s in segs)} launches, {len({c['refused']['message'] for c in done if 'refused' in c})} refusal texts -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:6])
    else:
        run(sys.argv[1])
