"""Route table of the ConvFeedForward middle: which launches each omlm_ffmid_* call makes, recorded from a kernel trace.

    timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tools/ffmid_route_calls.py calls.json
    python tools/ffmid_route_calls.py --merge calls.json DIR/*/r_kernel_trace.csv tests/ffmid_routes.json "recorded from <sha> on an MI355X"

The first form (a kernel trace only: no counters with it) issues every call of calls() once through hip.lib() (zero operands at their real
sizes: a route depends on sizes and on which pointers are null, never on values), each between two sentinel launches of
tools/gemm_route_calls.py, and writes the calls it made -- for a refused call the return code and the omlm_last_error text.  The second form
cuts the trace at the sentinels and stores per call the launches whose kernel name contains "ffmid" or "colsum": name with template
arguments, grid (x, y in workgroups), workgroup.  tests/test_ffmid_plan_host.py checks csrc/ffmid_plan.h against that table without a GPU;
the table comes from the commit BEFORE a change to the plan, never from the code under test.

Shapes are the smallest that reach each arm: B = 2, nseq = 40 (two strips per sample at RB = 20), nseq = 1 and 37 for the strip-count
seams, F = Fp - 4.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_route_calls import cut_trace, sentinel  # noqa: E402

F32, B16, F16 = "float32", "bfloat16", "float16"
H16 = (B16, F16)
ALL = (F32, B16, F16)
FWD_FP = (8, 512, 520, 1024, 1536, 2048, 2560, 2752, 3072, 3584, 4096)        # every NT of the strip forward, 64 .. 512
BWD_FP = (8, 512, 520, 1024, 1032, 2048, 2056, 3072)                           # every NT of the one-pass backward, 128 .. 768


def k(id, op, dt, Fp, **kw):
    """One call.  op: fwd, fwd_planes, fwd_mx, bwd.  dt: the operand dtype.  p / drop / gh / seed_dev: dropout and which of the optional
    pointers are given; dgamma / dconv (bwd).  seg: None or [n_full, p0].  impl: omlm_ffmid_set_impl for the call.  null: a required pointer
    to leave out.  misalign: "planes" (h1_lo two bytes off) or "du_tmp" (one element off).  stride: h2_8_stride "ok", "small" or "odd".
    M: the row count where it is not B * nseq.  dtype: the dtype code where it is not dt's."""
    r = dict(id=id, op=op, dt=dt, B=2, nseq=40, Fp=Fp, F=max(Fp - 4, 1), p=0.0, drop=False, gh=False, seed_dev=False, dgamma=True, dconv=True,
             seg=None, impl=1, null=None, misalign=None, stride="ok", M=None, dtype=None)
    r.update(kw)
    if r["M"] is None:
        r["M"] = r["B"] * r["nseq"]
    return r


TRAIN = dict(p=0.1, drop=True, gh=True, seed_dev=True)


def calls():
    r = []
    # ---- strip forward: every NT, the training form and the plain one ----
    for dt in ALL:
        r += [k(f"fwd/{dt} Fp={Fp} train", "fwd", dt, Fp, **TRAIN) for Fp in FWD_FP]
        r += [k(f"fwd/{dt} Fp={Fp} p=0", "fwd", dt, Fp) for Fp in FWD_FP]
        # TRAIN off: any one of p, drop_bits, gh missing (p > 0 without keep bits is the first generation's: below)
        r += [k(f"fwd/{dt} Fp=520 p=0, keep bits and gh", "fwd", dt, 520, drop=True, gh=True),
              k(f"fwd/{dt} Fp=520 p>0, no gh", "fwd", dt, 520, p=0.1, drop=True),
              k(f"fwd/{dt} Fp=520 p=0, gh", "fwd", dt, 520, gh=True)]
        # the strip-count seams
        r += [k(f"fwd/{dt} Fp=520 nseq={n} train", "fwd", dt, 520, nseq=n, **TRAIN) for n in (1, 36, 37, 72, 73)]
        # a row segment: the _seg kernel with dropout, the plain kernel without
        r += [k(f"fwd/{dt} Fp={Fp} segment, train", "fwd", dt, Fp, seg=[48, 8], **TRAIN) for Fp in (8, 520, 4096)]
        r += [k(f"fwd/{dt} Fp=520 segment, p>0, no gh", "fwd", dt, 520, seg=[48, 8], p=0.1, drop=True),
              k(f"fwd/{dt} Fp=520 segment, p=0", "fwd", dt, 520, seg=[48, 8], gh=True)]
    for dt in H16:
        r += [k(f"planes/{dt} Fp={Fp} train", "fwd_planes", dt, Fp, **TRAIN) for Fp in FWD_FP]
        r += [k(f"planes/{dt} Fp={Fp} p=0", "fwd_planes", dt, Fp, gh=True) for Fp in (8, 520, 4096)]
        r += [k(f"planes/{dt} Fp=520 segment, train", "fwd_planes", dt, 520, seg=[48, 8], **TRAIN),
              k(f"planes/{dt} Fp=520 segment, p=0", "fwd_planes", dt, 520, seg=[48, 8]),
              k(f"planes/{dt} Fp=520 p>0, no gh", "fwd_planes", dt, 520, p=0.1, drop=True)]
    r += [k(f"mx/Fp={Fp} train", "fwd_mx", F16, Fp, **TRAIN) for Fp in (64,) + FWD_FP[1:]]
    r += [k(f"mx/Fp={Fp} p=0", "fwd_mx", F16, Fp, gh=True) for Fp in (64, 520, 4096)]
    r += [k("mx/Fp=520 segment, train", "fwd_mx", F16, 520, seg=[48, 8], **TRAIN), k("mx/Fp=520 segment, p=0", "fwd_mx", F16, 520, seg=[48, 8]),
          k("mx/Fp=520 p>0, no gh", "fwd_mx", F16, 520, p=0.1, drop=True)]
    # ---- one-pass backward: every NT; dgamma / dconv both, one, none ----
    for dt in ALL:
        r += [k(f"bwd/{dt} Fp={Fp} train", "bwd", dt, Fp, **TRAIN) for Fp in BWD_FP]
        r += [k(f"bwd/{dt} Fp=520 p=0", "bwd", dt, 520, gh=True),
              k(f"bwd/{dt} Fp=520 dgamma only", "bwd", dt, 520, dconv=False, **TRAIN), k(f"bwd/{dt} Fp=520 dconv only", "bwd", dt, 520, dgamma=False, **TRAIN),
              k(f"bwd/{dt} Fp=520 no sums", "bwd", dt, 520, dgamma=False, dconv=False, **TRAIN)]
        r += [k(f"bwd/{dt} Fp=520 nseq={n}", "bwd", dt, 520, nseq=n, **TRAIN) for n in (1, 35, 36, 37, 71)]
        r += [k(f"bwd/{dt} Fp=8 B=300 nseq=37", "bwd", dt, 8, B=300, nseq=37, **TRAIN)]           # more than 256 strips: several per workgroup
        # ---- two-pass backward ----
        r += [k(f"bwd/{dt} Fp={Fp} two passes", "bwd", dt, Fp, **TRAIN) for Fp in (3080, 4096)]
        r += [k(f"bwd/{dt} Fp=3080 two passes, dgamma only", "bwd", dt, 3080, dconv=False, **TRAIN),
              k(f"bwd/{dt} Fp=3080 two passes, no sums", "bwd", dt, 3080, dgamma=False, dconv=False, **TRAIN),
              k(f"bwd/{dt} Fp=3080 two passes, nseq=37, p=0", "bwd", dt, 3080, nseq=37, gh=True)]
    # ---- first generation ----
    for dt in ALL:
        for Fp in (4104, 8192):
            r += [k(f"gen1/{dt} fwd Fp={Fp}", "fwd", dt, Fp, **TRAIN), k(f"gen1/{dt} bwd Fp={Fp}", "bwd", dt, Fp, **TRAIN)]
        r += [k(f"gen1/{dt} fwd p>0, no keep bits", "fwd", dt, 520, p=0.1, gh=True),
              k(f"gen1/{dt} fwd p>0, no keep bits, segment", "fwd", dt, 520, p=0.1, gh=True, seg=[48, 8]),
              k(f"gen1/{dt} bwd no gh", "bwd", dt, 520, p=0.1, drop=True),
              *[k(f"gen1/{dt} bwd no gh Fp={Fp}", "bwd", dt, Fp, p=0.1, drop=True) for Fp in (3072, 4096, 8192)],
              k(f"gen1/{dt} bwd p>0, no keep bits", "bwd", dt, 520, p=0.1, gh=True),
              k(f"gen1/{dt} bwd no gh, dgamma only", "bwd", dt, 520, dconv=False), k(f"gen1/{dt} bwd no gh, dconv only", "bwd", dt, 520, dgamma=False),
              k(f"gen1/{dt} bwd no gh, no sums", "bwd", dt, 520, dgamma=False, dconv=False)]
        for Fp in (128, 384, 512, 1024, 1032, 3072, 3080, 4096):                 # chunks per lane 1, 2 (MAXC 2), 3, 6 (MAXC 6), 7, 8 (MAXC 8)
            r += [k(f"gen1/{dt} fwd impl=0 Fp={Fp}", "fwd", dt, Fp, impl=0, **TRAIN), k(f"gen1/{dt} bwd impl=0 Fp={Fp}", "bwd", dt, Fp, impl=0, **TRAIN)]
        r += [k(f"gen1/{dt} fwd impl=0 M=16400", "fwd", dt, 8, B=410, impl=0), k(f"gen1/{dt} bwd impl=0 M=16400", "bwd", dt, 8, B=410, impl=0, gh=True)]
    # (the plane forwards know one generation: the switch does not reach them)
    r += [k("planes/impl=0", "fwd_planes", B16, 520, impl=0, **TRAIN), k("mx/impl=0", "fwd_mx", F16, 520, impl=0, **TRAIN)]
    r += [k(f"empty/{op}", op, F16, 520, B=0, M=0) for op in ("fwd", "fwd_planes", "fwd_mx", "bwd")]
    # ---- refusals ----
    for op, dt in (("fwd", F32), ("fwd", F16), ("fwd_planes", B16), ("fwd_planes", F16), ("fwd_mx", F16), ("bwd", F32), ("bwd", F16)):
        t = f"refused/{op} {dt}"
        r += [k(f"{t} null pointer", op, dt, 520, null="h1"), k(f"{t} Fp % 8", op, dt, 516, F=512), k(f"{t} Fp < F", op, dt, 520, F=521),
              k(f"{t} Fp=8200", op, dt, 8200), k(f"{t} M % nseq", op, dt, 520, M=81), k(f"{t} nseq=0", op, dt, 520, nseq=0, M=80)]
        if op != "bwd":
            r += [k(f"{t} p=1", op, dt, 520, p=1.0, drop=True), k(f"{t} p<0", op, dt, 520, p=-0.5, drop=True),
                  k(f"{t} segment p0=0", op, dt, 520, seg=[40, 0]), k(f"{t} segment p0 + nseq != n_full", op, dt, 520, seg=[50, 8])]
        if op in ("fwd_planes", "fwd_mx"):
            r += [k(f"{t} Fp=4104", op, dt, 4104), k(f"{t} p>0, no keep bits", op, dt, 520, p=0.1, gh=True),
                  k(f"{t} misaligned planes", op, dt, 520, misalign="planes")]
    r += [k("refused/fwd_planes float32 operands", "fwd_planes", B16, 520, dtype=0),
          k("refused/fwd_mx stride too small", "fwd_mx", F16, 520, stride="small"), k("refused/fwd_mx stride % 16", "fwd_mx", F16, 520, stride="odd"),
          k("refused/fwd_mx row pitch Fp=32", "fwd_mx", F16, 32), k("refused/fwd_mx last null pointer", "fwd_mx", F16, 520, null="scale8")]
    r += [k(f"refused/bwd {dt} misaligned du_tmp", "bwd", dt, 520, misalign="du_tmp", **TRAIN) for dt in ALL]
    r += [k("refused/bwd no workspace", "bwd", B16, 520, null="workspace", **TRAIN)]
    assert len({c["id"] for c in r}) == len(r)
    return r


def issue(c, dev):
    """the call; returns None, or (return code, message) of a refusal"""
    import torch
    from open_musiclm_amd import hip, ops
    L = hip.lib()
    T = getattr(torch, c["dt"])
    M, nseq, F, Fp, op = c["M"], c["nseq"], c["F"], c["Fp"], c["op"]
    rows = max(M, 1)
    z = lambda *s, t=T: torch.zeros(*s, dtype=t, device=dev)
    f32, u8 = torch.float32, torch.uint8
    t = dict(h1=z(rows, 2 * Fp), convw=z(3, 2 * Fp), gamma=z(Fp), h2=z(rows, Fp), mean=z(rows, t=f32), rstd=z(rows, t=f32),
             seed_dev=z(1, t=torch.int64), drop_bits=z(rows, (Fp + 7) // 8, t=u8), gh=z(rows, Fp))
    if op in ("fwd_planes", "fwd_mx"):
        t.update(convw_lo=z(3, 2 * Fp), gamma_lo=z(Fp), h1_lo=z(rows * 2 * Fp + 8, t=u8 if op == "fwd_mx" else T), h2_lo=z(rows, Fp))
    if op == "fwd_mx":
        P = ops.Fp8Planes(rows, Fp, dev)
        t.update(h2_8=P.planes, scale8=P.scale)
    if op == "bwd":
        t.update(dh2=z(rows, Fp), du_tmp=z(rows * 2 * Fp + 8), dh1=z(rows, 2 * Fp), dgamma=z(F, t=f32), dconv=z(2 * F * 3, t=f32),
                 workspace=z(ops.ffmid_bwd_workspace_floats(F, Fp), t=f32))
    off = {None: {}, "planes": {"h1_lo": 2}, "du_tmp": {"du_tmp": T.itemsize}}[c["misalign"]]       # bytes
    p =lambda name, on=True: t[name].data_ptr() + off.get(name, 0) if on and c["null"] != name else None
    dcode = {F32: 0, B16: 1, F16: 2}[c["dt"]] if c["dtype"] is None else c["dtype"]
    n_full, p0 = c["seg"] or (0, 0)
    opt = (p("seed_dev", c["seed_dev"]), p("drop_bits", c["drop"]), p("gh", c["gh"]))
    st = hip.stream_ptr()
    assert L.omlm_ffmid_set_impl(c["impl"]) == 0
    torch.cuda.synchronize()
    MARK()
    try:
        if op == "fwd":
            rc = L.omlm_ffmid_fwd_seg(p("h1"), p("convw"), p("gamma"), p("h2"), p("mean"), p("rstd"), M, nseq, F, Fp, 1e-5, c["p"], 7, *opt, dcode,
                                      n_full, p0, st)
        elif op == "fwd_planes":
            rc = L.omlm_ffmid_fwd_planes_seg(p("h1"), p("h1_lo"), p("convw"), p("convw_lo"), p("gamma"), p("gamma_lo"), p("h2"), p("h2_lo"), p("mean"),
                                             p("rstd"), M, nseq, F, Fp, 1e-5, c["p"], 7, *opt, dcode, n_full, p0, st)
        elif op == "fwd_mx":
            stride = {"ok": P.stride, "small": rows * 2 * Fp - 16, "odd": P.stride + 8}[c["stride"]]
            rc = L.omlm_ffmid_fwd_mx_seg(p("h1"), p("h1_lo"), p("convw"), p("convw_lo"), p("gamma"), p("gamma_lo"), p("h2"), p("h2_8"), stride,
                                         p("scale8"), p("mean"), p("rstd"), M, nseq, F, Fp, 1e-5, c["p"], 7, *opt, n_full, p0, st)
        else:
            rc = L.omlm_ffmid_bwd(p("dh2"), p("h1"), p("convw"), p("gamma"), p("mean"), p("rstd"), p("du_tmp"), p("dh1"), p("dgamma", c["dgamma"]),
                                  p("dconv", c["dconv"]), p("workspace"), M, nseq, F, Fp, c["p"], 7, *opt, dcode, st)
    finally:
        MARK()                                                 # what follows in the trace is the next call's preparation
        torch.cuda.synchronize()
        L.omlm_ffmid_set_impl(1)
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
        r = issue(c, dev)
        if r is not None:
            c["refused"] = dict(rc=r[0], message=r[1])
        torch.cuda.empty_cache()
        print(c["id"], "refused" if r else "served", flush=True)
    json.dump(dict(calls=done), open(out, "w"), indent=0)
    print(f"{len(done)} calls issued")


def merge(calls_json, trace_csv, out, source):
    done = json.load(open(calls_json))["calls"]
    segs = cut_trace(trace_csv, lambda name: "ffmid" in name or "colsum" in name)
    assert len(segs) == 2 * len(done), (len(segs), len(done))
    segs = segs[0::2]                                          # a sentinel in front of each call and one behind it
    for c, seg in zip(done, segs):
        c["launches"] = [dict(kernel=r["Kernel_Name"], workgroup=int(r["Workgroup_Size_X"]),
                              grid=[int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XY"]) for r in seg]
    json.dump(dict(source=source, rows=done), open(out, "w"), indent=0)
    print(f"{len(done)} rows, {sum(len(s) for s in segs)} launches -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:6])
    else:
        run(sys.argv[1])
