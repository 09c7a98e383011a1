"""Route table of the KV-cached decode step: which launches each omlm_decode_step call makes, recorded from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python tools/decode_route_calls.py calls.json
    python tools/decode_route_calls.py --merge calls.json DIR/*/r_kernel_trace.csv tests/decode_routes.json "recorded from <sha> on an MI355X"

The first form issues every call of calls() once through hip.lib() (zero operands at their real sizes: a route depends on sizes and on which
pointers are null, never on values), each between two sentinel launches of tools/gemm_route_calls.py, and writes the calls it made -- for a
refused call the return code and the omlm_last_error text.  The second form cuts the trace at the sentinels and stores per call the launches
whose kernel name contains "dec": name with template arguments, grid (x, y in workgroups), workgroup.
tests/test_decode_plan_host.py checks csrc/decode_plan.h against that table without a GPU; the table comes from the commit BEFORE a change to
the plan, never from the code under test.

Geometries are the smallest that reach each arm: L = 1, Nmax = 64 (nsplit = 1), V1 = 17; dim 1024 for the second-generation kernels, dim 64
for the first.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_route_calls import cut_trace, sentinel  # noqa: E402

F32, B16, F16 = "float32", "bfloat16", "float16"


def k(id, B, w, **kw):
    """One call.  w: weight dtype.  Pointers that are given unless named otherwise: emb (emb_table + ids), head (head_W), adv (advance_pos),
    ln (ln_parts), ws / cnt (splitk_ws / splitk_cnt).  lo: None, "all" (W1p_lo, W2p_lo and, with head, head_W_lo), "no_w2", "no_head".
    null: a pointer to leave out ("args", "pos_dev", "parts", "ids", "k_new").  round: round_bf16 (default: 16-bit weights)."""
    r = dict(id=id, B=B, w=w, D=1024, H=8, L=1, Fp=256, Nmax=64, nsplit=1, V1=17, kv16=0, lo=None, emb=True, head=True, adv=True, ln=True,
             ws=True, cnt=True, null=None)
    r.update(kw)
    r.setdefault("round", 0 if w == F32 else 1)
    return r


def calls():
    g1 = dict(D=64, H=1, Fp=64)
    r = []
    # ---- second generation (dim 1024): row kernels (B = 1), vector kernels (dec2), matrix-core kernels (dec4) ----
    for w in (F32, B16, F16):
        r += [k(f"gen2/{w} B={B}", B, w) for B in (1, 2, 8)]
    for w in (B16, F16):
        r += [k(f"gen2/{w} B={B}", B, w) for B in (9, 16, 17, 64)]
    for H in (2, 9):                                           # to_out of the vector kernels: NI = 1 / 2 at H * 64 = 512
        r += [k(f"gen2/{F32} B=2 H={H}", 2, F32, H=H), k(f"gen2/{B16} B=1 H={H}", 1, B16, H=H), k(f"gen2/{B16} B=2 H={H}", 2, B16, H=H)]
    r += [k(f"gen2/{B16} B=17 H=16", 17, B16, H=16), k(f"gen2/{F16} B=1 H=9", 1, F16, H=9)]
    r += [k(f"gen2/{w} B={B} Fp={Fp}", B, w, Fp=Fp) for w, B, Fp in (
        (B16, 2, 64), (B16, 16, 64), (B16, 64, 64), (F32, 2, 64),                                   # (Fp >> 5) < 8: no split
        (B16, 1, 3072), (B16, 2, 3072), (B16, 16, 3072), (B16, 64, 3072), (F32, 1, 3072), (F32, 2, 3072),      # matrix-core ceiling
        (B16, 1, 3104), (B16, 2, 3104), (F16, 8, 3104), (F32, 1, 3104), (F32, 2, 3104),                         # dec2<..., 8>
        (B16, 1, 4096), (B16, 8, 4096), (F32, 8, 4096),                                             # second-generation ceiling
        (B16, 1, 4160), (B16, 8, 4160), (F32, 2, 4160))]                                            # ... past it: first generation at dim 1024
    r += [k(f"gen2/{w} B={B} kv16", B, w, kv16=1) for w, B in ((B16, 1), (B16, 2), (B16, 17), (F16, 2))]
    r += [k(f"gen2/{B16} B=2 Fp=4096 kv16", 2, B16, Fp=4096, kv16=1)]
    r += [k(f"gen2/lo planes B={B}", B, F16, lo="all") for B in (1, 2, 16, 17, 64)]
    r += [k("gen2/lo planes B=2 Fp=64", 2, F16, lo="all", Fp=64), k("gen2/lo planes B=17 Fp=64", 17, F16, lo="all", Fp=64),
          k("gen2/lo planes B=1 Fp=3072", 1, F16, lo="all", Fp=3072),
          k("gen2/lo planes B=2 Fp=3072", 2, F16, lo="all", Fp=3072), k("gen2/lo planes B=2 no head", 2, F16, lo="all", head=False),
          k("gen2/lo planes B=1 no head", 1, F16, lo="all", head=False), k("gen2/lo planes B=2 kv16", 2, F16, lo="all", kv16=1),
          k("gen2/lo planes bf16 B=2", 2, B16, lo="all"), k("gen2/lo planes B=2 no splitk_ws", 2, F16, lo="all", ws=False)]
    # the caller embedded the ids itself: the row-sum launch at B > 8, nothing below
    r += [k(f"gen2/{B16} B={B} no emb_table", B, B16, emb=False) for B in (1, 8, 9, 17)]
    r += [k(f"gen2/{B16} B=9 no emb_table, lo planes", 9, F16, emb=False, lo="all")]
    # the advance: in the head, or a launch of its own
    for B in (1, 2):
        r += [k(f"gen2/{B16} B={B} no head, advance", B, B16, head=False), k(f"gen2/{B16} B={B} head, no advance", B, B16, adv=False),
              k(f"gen2/{B16} B={B} no head, no advance", B, B16, head=False, adv=False)]
    r += [k(f"gen2/{F32} B=2 no head, advance", 2, F32, head=False)]
    # LayerNorm partials and the split-K scratch: combine in attention against the combine kernel, split against whole rows
    r += [k(f"gen2/{B16} B=2 no ln_parts", 2, B16, ln=False), k(f"gen2/{B16} B=8 no ln_parts", 8, B16, ln=False),
          k(f"gen2/{B16} B=2 no splitk_ws", 2, B16, ws=False), k(f"gen2/{B16} B=2 no splitk_cnt", 2, B16, cnt=False),
          k(f"gen2/{B16} B=16 no splitk_cnt", 16, B16, cnt=False), k(f"gen2/{B16} B=2 no ln_parts, no splitk_cnt", 2, B16, ln=False, cnt=False),
          k(f"gen2/{B16} B=16 no scratch", 16, B16, ws=False, cnt=False), k(f"gen2/{B16} B=1 no scratch", 1, B16, ln=False, ws=False, cnt=False),
          k(f"gen2/{F32} B=2 no scratch", 2, F32, ln=False, ws=False, cnt=False)]
    r += [k(f"gen2/{B16} B=2 L=2", 2, B16, L=2), k(f"gen2/{B16} B=2 L=0", 2, B16, L=0), k(f"gen2/{B16} B=1 L=0", 1, B16, L=0),
          k("gen2/lo planes B=2 L=0 emb_table", 2, F16, L=0, lo="all", H=2, Fp=64)]
    # ---- first generation ----
    r += [k(f"gen1/{w} B={B}", B, w, **g1) for w, B in ((F32, 1), (F32, 8), (B16, 1), (B16, 3), (F16, 2))]
    r += [k(f"gen1/{B16} B=3 kv16", 3, B16, kv16=1, **g1), k(f"gen1/{F16} B=2 kv16", 2, F16, kv16=1, **g1),
          k("gen1/lo planes fp16 B=2", 2, F16, lo="all", **g1), k("gen1/lo planes fp32 B=2", 2, F32, lo="all", **g1),
          k("gen1/lo planes fp16 B=1 no head", 1, F16, lo="all", head=False, **g1),
          k(f"gen1/{B16} B=2 no head", 2, B16, head=False, **g1), k(f"gen1/{B16} B=2 no advance", 2, B16, adv=False, **g1),
          k(f"gen1/{B16} B=2 no emb_table", 2, B16, emb=False, **g1), k(f"gen1/{B16} B=2 L=2", 2, B16, L=2, **g1),
          k(f"gen1/{B16} B=2 D=1056", 2, B16, D=1056), k(f"gen1/{B16} B=2 D=96 H=2", 2, B16, D=96, H=2, Fp=64)]
    # ---- refusals ----
    r += [k("refused/null argument block", 1, B16, null="args"), k("refused/B=0", 0, B16), k("refused/B=65", 65, B16),
          k("refused/B=9 fp32 weights", 9, F32), k("refused/B=9 no ln_parts", 9, B16, ln=False), k("refused/B=9 Fp=3104", 9, B16, Fp=3104),
          k("refused/B=9 first generation", 9, B16, **g1), k("refused/B=17 no splitk_ws", 17, B16, ws=False),
          k("refused/B=17 no splitk_cnt", 17, B16, cnt=False), k("refused/D=1028", 2, B16, D=1028), k("refused/Fp=68", 2, B16, Fp=68),
          k("refused/no pos_dev", 2, B16, null="pos_dev"), k("refused/no parts", 2, B16, null="parts"), k("refused/H=0", 2, B16, H=0),
          k("refused/H=17", 2, B16, H=17), k("refused/nsplit=0", 2, B16, nsplit=0),
          k("refused/LDS budget B=8 Fp=4800", 8, B16, D=64, H=1, Fp=4800), k("refused/no ids", 2, B16, null="ids"),
          k("refused/kv16 fp32 weights", 2, F32, kv16=1), k("refused/kv16 round_bf16=0", 2, B16, kv16=1, round=0),
          k("refused/kv16 no k_new", 2, B16, kv16=1, null="k_new"),
          k("refused/lo planes fp32 weights", 2, F32, lo="all", emb=False), k("refused/lo planes no head_W_lo", 2, F16, lo="no_head", emb=False),
          k("refused/lo planes B=2 no ln_parts", 2, F16, lo="all", ln=False, emb=False),
          k("refused/lo planes B=1 Fp=3104", 1, F16, lo="all", Fp=3104, emb=False),
          k("refused/lo planes head without partials L=0", 2, F16, lo="all", L=0, H=2, Fp=64, emb=False),
          k("refused/lo planes first generation no W2p_lo", 2, F16, lo="no_w2", **g1),
          # the two that come after the embedding gather has been launched
          k("refused/late: lo planes no W2p_lo, emb_table", 2, F16, lo="no_w2"),
          k("refused/late: lo planes B=2 L=0 no ln_parts, emb_table", 2, F16, lo="all", L=0, H=2, Fp=64, ln=False)]
    assert len({c["id"] for c in r}) == len(r)
    return r


def issue(c, dev):
    """the call; returns None, or (return code, message) of a refusal"""
    import torch
    from open_musiclm_amd import decode, hip
    L = hip.lib()
    tw = getattr(torch, c["w"])
    B, D, H, Fp, nl, Nmax, V1 = max(c["B"], 1), c["D"], max(c["H"], 1), c["Fp"], c["L"], c["Nmax"], c["V1"]
    HD, nsplit = H * 64, max(c["nsplit"], 1)
    z = lambda *s, t=torch.float32: torch.zeros(*s, dtype=t, device=dev)
    keep = []

    def arr(make):
        ts = [make() for _ in range(max(nl, 1))]
        a = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        keep.extend([ts, a])
        return C.cast(a, C.POINTER(C.c_void_p))
    a = decode.DecodeArgs()
    a.B, a.D, a.H, a.L, a.F, a.Fp, a.Nmax, a.nsplit = c["B"], D, c["H"], nl, Fp, Fp, Nmax, c["nsplit"]
    a.w_dtype = {F32: 0, B16: 1, F16: 2}[c["w"]]
    a.round_bf16, a.eps, a.scale = c["round"], 1e-5, 8.0
    tc = tw if c["kv16"] else torch.float32
    a.Wq, a.Wkv, a.Wo = arr(lambda: z(HD, D, t=tw)), arr(lambda: z(128, D, t=tw)), arr(lambda: z(D, HD, t=tw))
    a.W1p, a.W2p = arr(lambda: z(2 * Fp, D, t=tw)), arr(lambda: z(D, Fp, t=tw))
    a.attn_gamma, a.ffin_gamma, a.mid_gamma = arr(lambda: z(D)), arr(lambda: z(D)), arr(lambda: z(Fp))
    a.q_scale, a.k_scale, a.convw = arr(lambda: z(64)), arr(lambda: z(64)), arr(lambda: z(3, 2 * Fp))
    a.Kc, a.Vc, a.hist = arr(lambda: z(B, Nmax, 64, t=tc)), arr(lambda: z(B, Nmax, 64, t=tc)), arr(lambda: z(B, 2, 2 * Fp))
    t = dict(pos_dev=z(1, t=torch.int32), bias=z(Nmax, 24), final_gamma=z(D), head_W=z(V1, D, t=tw), emb=z(32, D), x=z(B, D), x1=z(B, D),
             q=z(B, HD), parts=z(B, nsplit, H, 66), u=z(B, Fp), logits=z(B, 24), adv=z(1, t=torch.int32), k_new=z(B, 64),
             ids=z(B, t=torch.int64), head_W_lo=z(V1, D, t=tw))
    sizes = decode.scratch_sizes(B, D, Fp)
    t.update(ln=z(sizes["ln_parts"]), ws=z(sizes["splitk_ws"]), cnt=z(sizes["splitk_cnt"], t=torch.int32))
    null = c["null"]
    p = lambda name, on=True: t[name].data_ptr() if on and null != name else None
    a.pos_dev, a.bias_table, a.bias_ld, a.final_gamma = p("pos_dev"), p("bias"), 24, p("final_gamma")
    a.head_W, a.V1, a.ldV = p("head_W", c["head"]), V1, 24
    a.emb_table, a.emb_row_offset, a.emb_rows = p("emb", c["emb"]), 0, 32
    a.x, a.x1, a.q, a.parts, a.u, a.logits = p("x"), p("x1"), p("q"), p("parts"), p("u"), p("logits")
    a.advance_pos, a.advance_step = p("adv", c["adv"]), None
    a.ln_parts, a.splitk_ws, a.splitk_cnt = p("ln", c["ln"]), p("ws", c["ws"]), p("cnt", c["cnt"])
    if c["lo"]:
        a.W1p_lo = arr(lambda: z(2 * Fp, D, t=tw))
        if c["lo"] != "no_w2":
            a.W2p_lo = arr(lambda: z(D, Fp, t=tw))
        a.head_W_lo = p("head_W_lo", c["head"] and c["lo"] != "no_head")
    a.kv16, a.k_new = c["kv16"], p("k_new", bool(c["kv16"]))
    torch.cuda.synchronize()
    MARK()
    try:
        rc = L.omlm_decode_step(None if null == "args" else C.addressof(a), p("ids"), hip.stream_ptr())
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
        r = issue(c, dev)
        if r is not None:
            c["refused"] = dict(rc=r[0], message=r[1])
        torch.cuda.empty_cache()
        print(c["id"], "refused" if r else "served", flush=True)
    json.dump(dict(calls=done), open(out, "w"), indent=0)
    print(f"{len(done)} calls issued")


def merge(calls_json, trace_csv, out, source):
    done = json.load(open(calls_json))["calls"]
    segs = cut_trace(trace_csv, lambda name: "dec" in name)
    assert len(segs) == 2 * len(done), (len(segs), len(done))
    segs = segs[0::2]                                          # a sentinel in front of each call and one behind it
    for c, seg in zip(done, segs):
        # (a refused call keeps what it launched before it refused)
        c["launches"] = [dict(kernel=r["Kernel_Name"], workgroup=int(r["Workgroup_Size_X"]),
                              grid=[int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XY"]) for r in seg]
    json.dump(dict(source=source, rows=done), open(out, "w"), indent=0)
    print(f"{len(done)} rows, {sum(len(s) for s in segs)} launches -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(*sys.argv[2:6])
    else:
        run(sys.argv[1])
