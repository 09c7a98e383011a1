"""What the weight EMA in the fused optimizer step costs, measured on the MI355X (profiles/optim_ema.md is written from this).

  python tools/optim_ema_probe.py [--parent-lib PATH/libomlm_hip.so] [--rounds 9] [--iters 40] [--train-steps 12] [--out FILE.json]

Part 1, the optimizer launch at the flat length of the coarse musiclm_small model (dim 1024, depth 6, heads 8: the bench's model), both
weight-decay groups, fp16 shadow, clipping on, gradients cleared in the pass -- one optimizer step's launches, `iters` of them between
two device events, the variants interleaved round after round in ONE process:

  a   the parent commit's library (--parent-lib: a build of the parent's csrc), omlm_adamw_clip_step; run TWICE per round, so that
      its own spread stands beside everything else
  b   this library, omlm_adamw_clip_step (EMA off)
  c   this library, omlm_adamw_clip_step_ema (EMA on)
  d   this library, omlm_adamw_clip_step followed by E.lerp_(P, 1 - d) (the hand-made EMA)

The only bar: the median of b lies within [min, max] of the a samples.  c and d are recorded.

Part 2, the coarse training step of bench.py (its TrainLeg: captured micro-step + fused optimizer step, batch 32, fp16ff) with the
optimizer built with and without ema_decay, alternating windows of --train-steps steps."""
import argparse
import ctypes as C
import functools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def flat_layout(dev):
    """(total, ranges) of FusedAdam's flat buffers for the bench's coarse model; the model itself is dropped again."""
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.optimizer import get_optimizer
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, attn_dropout=0.0, ff_dropout=0.1, num_coarse_quantizers=3,
                                        precision="fp16ff").to(dev)
    opt = get_optimizer(model.parameters(), lr=3e-4, wd=0.01)
    opt.zero_grad()
    return opt._flat["total"], list(opt._flat["ranges"])


def bind_parent(path):
    from open_musiclm_amd import hip
    lib = C.CDLL(path)
    fn = lib.omlm_adamw_clip_step
    fn.argtypes, fn.restype = hip.SIGNATURES["omlm_adamw_clip_step"], C.c_int
    return fn


def launch_part(args, dev):
    from open_musiclm_amd import hip, ops
    from open_musiclm_amd.ema import ema_decay_at
    total, ranges = flat_layout(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    P = torch.randn(total, device=dev, generator=g) * 0.02
    G = torch.randn(total, device=dev, generator=g) * 1e-3
    M_, V = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    E, P16 = P.clone(), P.to(torch.float16)
    nsq = (G.double() ** 2).sum().float().reshape(1)
    hp = dict(lr=3e-4, beta1=0.9, beta2=0.99, eps=1e-8, step=100, gscale=1.0, gnorm_sq=nsq, max_norm=0.5, decoupled=True, zero_grad=True)
    wds = (0.01, 0.0)
    d = ema_decay_at(100, 0.999, 0, True)
    parent = bind_parent(args.parent_lib) if args.parent_lib else None

    def step_parent():
        for (a, b), wd in zip(ranges, wds):
            rc = parent(hip.ptr(P[a:b]), hip.ptr(G[a:b]), hip.ptr(M_[a:b]), hip.ptr(V[a:b]), hip.ptr(P16[a:b]), b - a, hp["lr"], hp["beta1"],
                        hp["beta2"], hp["eps"], wd, hp["step"], hp["gscale"], hip.ptr(nsq), hp["max_norm"], 1, 1, ops.dcode(torch.float16),
                        None, hip.stream_ptr())
            assert rc == 0

    def step_new(ema):
        for (a, b), wd in zip(ranges, wds):
            kw = dict(ema=E[a:b], ema_decay=0.999) if ema else {}
            ops.adamw_clip_step(P[a:b], G[a:b], M_[a:b], V[a:b], P16[a:b], wd=wd, **hp, **kw)

    def step_lerp():
        step_new(False)
        E.lerp_(P, 1.0 - d)

    variants = {"b_this_ema_off": lambda: step_new(False), "c_this_ema_on": lambda: step_new(True), "d_old_entry_plus_lerp": step_lerp}
    order = ["b_this_ema_off", "c_this_ema_on", "d_old_entry_plus_lerp"]
    if parent is not None:
        variants["a_parent"] = step_parent
        order = ["a_parent"] + order + ["a_parent"]

    def window(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / args.iters      # us per optimizer step (both groups)

    for name in set(order):                                    # warm-up: code objects loaded, clocks up
        window(variants[name])
    samples = {name: [] for name in variants}
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            samples[name].append(window(variants[name]))
    n_real = sum(b - a for a, b in ranges)
    out = dict(flat_elements=total, group_elements=[b - a for a, b in ranges], iters=args.iters, rounds=args.rounds, us_per_step={})
    for name, s in sorted(samples.items()):
        out["us_per_step"][name] = dict(median=statistics.median(s), min=min(s), max=max(s), n=len(s), samples=[round(x, 2) for x in s])
    bytes_per = dict(a_parent=34, b_this_ema_off=34, c_this_ema_on=42, d_old_entry_plus_lerp=46)
    out["tb_per_s_at_median"] = {k: n_real * bytes_per[k] / (v["median"] * 1e-6) / 1e12 for k, v in out["us_per_step"].items()}
    if parent is not None:
        a, b = out["us_per_step"]["a_parent"], out["us_per_step"]["b_this_ema_off"]
        out["b_within_spread_of_a"] = bool(a["min"] <= b["median"] <= a["max"])
    return out


def train_part(args, dev):
    import bench
    import open_musiclm_amd.optimizer as O
    from open_musiclm_amd.parallel import DataParallel
    dp = DataParallel(device=dev)
    kw = dict(stage="coarse", dim=1024, depth=6, heads=8, precision="fp16ff", batch=32, accum=1, use_graph=True)
    plain_get = O.get_optimizer
    legs = {"ema_off": bench.TrainLeg(dev, dp, **kw)}
    O.get_optimizer = functools.partial(plain_get, ema_decay=0.999)          # TrainLeg takes the factory from the module when it is built
    try:
        legs["ema_on"] = bench.TrainLeg(dev, dp, **kw)
    finally:
        O.get_optimizer = plain_get
    assert legs["ema_on"].optim.ema_enabled and not legs["ema_off"].optim.ema_enabled
    samples = {k: [] for k in legs}
    for k, leg in legs.items():
        leg.timed(2, 3)
    for r in range(args.train_rounds):
        for k in (("ema_off", "ema_on") if r % 2 == 0 else ("ema_on", "ema_off")):
            dt, loss = legs[k].timed(args.train_steps, 0)
            samples[k].append(dt / args.train_steps * 1e3)
    return dict(steps_per_window=args.train_steps, ms_per_step={k: dict(median=statistics.median(s), min=min(s), max=max(s),
                                                                          samples=[round(x, 3) for x in s]) for k, s in samples.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--train-steps", type=int, default=12)
    ap.add_argument("--train-rounds", type=int, default=4)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_ema_probe needs the MI355X: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), launch=launch_part(args, dev))
    if not args.no_train:
        res["train_step"] = train_part(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
