"""GPU: the attention kernels at tile edges and under sparse key masks, element by element (tests/attn_edge_ref.py).

Every case of attn_edge_ref.CASES (B = 3; N on and next to the 32 / 64 / 128 / 256 seams; H = 1, 3, 8, 9, 16; key masks with whole dead tiles,
right-padded batches, at most ten live keys) runs through ops.attn_fwd and ops.attn_bwd on each route of attn_edge_ref.ROUTES -- which kernel
families those reach is asserted by tests/test_attn_edge_host.py from the route plan -- and is compared with the fp64 reference PER ELEMENT:
|got - ref| over the sum of the absolute values of the terms that make the element.  The tolerances are the project's own
(test_attention_fwd_bwd); the host test shows that the kernels' stated roundings stay under half of them and that a dropped key, a distance
off by one, a shifted mask, a wrong head column or a lost d(bias) block lands over ten times them.

Every input is a view in front of NaNs and every output a view between two 4 KiB margins of a sentinel pattern, so a read past the last
sample or a store past row N shows.  The gather probe makes the softmax one-hot at one distance, which turns any wrong key offset, bias
window or head column into a wrong ROW of v, whatever the rounding.  Rows without a live key follow the contract of include/omlm.h.
Every metric goes to the kernel report of tests/test_gpu_kernels.py (its REPORT file) under its case name, with the index where it is
reached."""
import json
import math
import os

import pytest
import torch

import attn_edge_ref as R
from test_gpu_kernels import REPORT          # the one kernel report, next to the other kernel tests' entries

pytestmark = pytest.mark.gpu

SCALE = 8.0
MARGIN = 4096                  # bytes of sentinel on each side of an output (a multiple of 256: vector accesses stay aligned)
SENT = 0x7FA5                  # a NaN as bf16 and as fp16; two of them (0x7FA57FA5) a NaN as fp32


def report_all(entries):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    data = {}
    if os.path.exists(REPORT):
        try:
            data = json.load(open(REPORT))
        except Exception:
            data = {}
    data.update(entries)
    json.dump(data, open(REPORT, "w"), indent=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from open_musiclm_amd import ops as o
    from open_musiclm_amd import hip
    hip.lib()       # fail loudly if the extension is missing
    return o


class Guarded:
    """Outputs between sentinel margins, inputs in front of NaNs."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def out(self, name, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        total = MARGIN + (nbytes + 255) // 256 * 256 + MARGIN
        raw = torch.full((total // 2,), SENT, dtype=torch.int16, device=self.dev)
        self.bufs.append((name, raw, MARGIN // 2, (MARGIN + nbytes) // 2))
        return raw.view(torch.uint8)[MARGIN:MARGIN + nbytes].view(dtype).view(shape)

    def inp(self, t):
        """t (CPU) on the device, followed by 4 KiB of NaN (uint8: of live-key bytes)"""
        tail = MARGIN // t.element_size()
        fill = 1 if t.dtype == torch.uint8 else float("nan")
        buf = torch.full((t.numel() + tail,), fill, dtype=t.dtype, device=self.dev)
        view = buf[:t.numel()].view(t.shape)
        view.copy_(t)
        return view

    def broken(self):
        """names of the outputs whose margins no longer hold the sentinel bit for bit"""
        return [name for name, raw, lo, hi in self.bufs if not (bool((raw[:lo] == SENT).all()) and bool((raw[hi:] == SENT).all()))]


_INPUTS, _REFS = {}, {}


def inputs_of(case, dtype):
    key = (case, dtype)
    if key not in _INPUTS:
        _INPUTS[key] = R.make_inputs(case, dtype)
    return _INPUTS[key]


def table_of(route, dtype, inp):
    """the fp32 table the route's softmax sees (None: no bias)"""
    if route.table == "none":
        return None
    return inp["bias"] * R.FIXED_TABLE_SCALE[dtype] if route.table == "fixed" else inp["bias"]


def reference_of(case, dtype, route, dev):
    """one fp64 reference per (case, operand type, table), computed on the GPU and shared by the routes that see the same problem"""
    inp = inputs_of(case, dtype)
    scale = 0.0 if route.table == "none" else R.FIXED_TABLE_SCALE[dtype] if route.table == "fixed" else 1.0
    key = (case, dtype, scale)
    if key not in _REFS:
        table = table_of(route, dtype, inp)
        on = lambda t: None if t is None else t.to(dev)
        _REFS[key] = R.reference(on(inp["q"]), on(inp["k"]), on(inp["v"]), on(table), on(inp["keymask"]), on(inp["dout"]), case.H, SCALE, route.P)
    return _REFS[key]


def fixed_flag(ab, H):
    return float(ab.tableT.view(-1, ab.tableT.numel() // ((H + 7) // 8 * 8))[0, -2])


def run_attention(ops, dev, route, dtype, N, H, q, k, v, dout, table, keymask, fixed_bound=1.0):
    """forward, then the backward on its own out and lse, every buffer guarded.  q, k, v, dout [B, N, ..] of `dtype`, table fp32 [N, ld] or
    None, keymask [B, N] bool or None (CPU tensors).  Returns (results by name, problems found outside the numbers)."""
    B = q.shape[0]
    M = B * N
    G = Guarded(dev)
    qd, kd, vd, dod = (G.inp(t.reshape(M, -1)) for t in (q, k, v, dout))
    km = None if keymask is None else G.inp(keymask.to(torch.uint8))
    tab = None if table is None else G.inp(table)
    problems = []
    bias = tab
    if route.table == "fixed":
        bias = ops.AttnBias(tab, N, H, dev, qk_bound=fixed_bound, scale=SCALE, half=dtype == torch.float16)
        if fixed_flag(bias, H) != 1.0:
            problems.append("the prepared table does not select the fixed reference point")
    out, lse, delta = G.out("out", (M, H * 64), dtype), G.out("lse", (B, H, N), torch.float32), G.out("delta", (B, H, N), torch.float32)
    dq, dk, dv = G.out("dq", (M, H * 64), torch.float32), G.out("dk", (M, 64), torch.float32), G.out("dv", (M, 64), torch.float32)
    dbias = prefill = None
    if table is not None:
        dbias = G.out("dbias", tuple(table.shape), torch.float32)
        dbias.zero_()
        if not route.ws:                       # the atomic form accumulates on top of what is there
            prefill = torch.zeros(table.shape)
            prefill[:, :H] = torch.randn(table.shape[0], H, generator=torch.Generator().manual_seed(N + H))
            prefill = prefill.to(dev)
            dbias.copy_(prefill)
    ops.attn_fwd(qd, kd, vd, bias, km, out, lse, B, N, H, SCALE, P=route.P)
    ops.attn_bwd(qd, kd, vd, bias, km, out, dod, lse, delta, dq, dk, dv, dbias, B, N, H, SCALE, P=route.P, workspace=route.ws)
    torch.cuda.synchronize()
    problems += [f"guard band of {n} overwritten" for n in G.broken()]
    got = dict(out=out.view(B, N, -1), lse=lse, delta=delta, dq=dq.view(B, N, -1), dk=dk.view(B, N, 64), dv=dv.view(B, N, 64))
    if dbias is not None:
        got["dbias"] = (dbias - prefill if prefill is not None else dbias)[:, :H]
        if float((dbias[:, H:] - (prefill[:, H:] if prefill is not None else 0.0)).abs().max() if dbias.shape[1] > H else 0.0) != 0.0:
            problems.append("dbias[:, H:] written")
    problems += [f"NaN in {n}" for n, t in got.items() if bool(torch.isnan(t.float()).any())]
    if keymask is not None:
        deadkey = ~keymask.to(dev)
        for n in ("dk", "dv"):
            if float(got[n][deadkey].abs().max() if bool(deadkey.any()) else 0.0) != 0.0:
                problems.append(f"{n} rows of masked keys are not exactly zero")
    return got, problems


def compare(got, ref, dtype, with_dbias=True):
    """({tensor: metric, tensor_at: index}, [tensor over its tolerance])"""
    names = tuple(n for n in R.TENSORS if with_dbias or n != "dbias")
    full = dict(got)
    if not with_dbias:
        full["dbias"] = ref.val["dbias"]
    w = R.worst_ratio(full, ref, dtype)
    metrics, over = {}, []
    for n in names + ("lse",):
        ratio, metric, at = w[n]
        metrics[n], metrics[n + "_at"] = metric, list(at)
        if not ratio <= 1.0:
            over.append(f"{n} {metric:.3e} > {R.tol_of(n, dtype):.0e} at {at}")
    return metrics, over


ROUTE_RUNS = [(r, d) for r in R.ROUTES for d in r.dtypes]


@pytest.mark.parametrize("route,dtype", ROUTE_RUNS, ids=[f"{r.name}-{str(d).replace('torch.', '')}" for r, d in ROUTE_RUNS])
def test_edge_cases_per_element(ops, dev, route, dtype):
    entries, failures = {}, []
    for case in route.cases:
        inp = inputs_of(case, dtype)
        ref = reference_of(case, dtype, route, dev)
        got, problems = run_attention(ops, dev, route, dtype, case.N, case.H, inp["q"], inp["k"], inp["v"], inp["dout"],
                                      table_of(route, dtype, inp), inp["keymask"])
        metrics, over = compare(got, ref, dtype, with_dbias=route.table != "none")
        entries[f"attn_edge[{route.name},{dtype},{case.name}]"] = dict(metrics, problems=problems + over)
        failures += [f"{case.name}: {p}" for p in problems + over]
    report_all(entries)
    assert not failures, f"{len(failures)} findings, the first: " + "; ".join(failures[:12])


# ---- the gather probe -----------------------------------------------------------------------------------------------------------------------
PROBE_ROUTES = [(r, d) for r in R.ROUTES if r.name in ("fp32", "online", "fixed", "prefix1") for d in r.dtypes]
PROBE_SHAPES = ((33, 3), (129, 9), (257, 3))
PROBE_R0 = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128)          # and N - 1


def _bf16_values(t):
    return t.to(torch.bfloat16).to(t.dtype)


@pytest.mark.parametrize("route,dtype", PROBE_ROUTES, ids=[f"{r.name}-{str(d).replace('torch.', '')}" for r, d in PROBE_ROUTES])
def test_gather_probe(ops, dev, route, dtype):
    """q = 0 and a table that is 0 at ONE distance r0 and far below it elsewhere: for every row i >= r0 whose key i - r0 is live the softmax
    is one-hot up to N e^-gap < 2^-14, so out[b, i, h] IS v[b, i - r0] -- bit for bit on the online 16-bit routes, within one unit in the
    last place on the fixed-reference route, to 2e-5 for fp32 -- and dv[b, j] is sum_h dout[b, j + r0, h].

    The rows with i < r0 or a masked target key are NOT one-hot (every score they have is the far-below one: they average their live keys),
    so they do reach dv, dq and d(bias): the closed forms are asserted for the keys, rows and distances those rows do not touch, to 1e-6 /
    1e-5 of the term sums, and everything else against the fp64 reference at the ordinary tolerances.
    fp32 operands: the backward kernels round q, k, v and dO to bf16 (include/omlm.h), so v and dout are drawn as bf16 values there, or
    dP - delta of the one-hot pair would be dO . (bf16(v) - v) and not zero.
    The fixed reference point of half operands is taken while the table's range stays under 28 octaves: its gap is 19, not 24
    (N e^-19 < 2^-14 still).  On that route the one-hot probability itself, 2^-m, is rounded to the type before the denominator sums it,
    so O is v within one unit in the last place, the backward's P = 2^(s - lse) is 1 within one, and dP - delta = dO . (v - O) is within
    one of the term sum: the closed forms hold to one unit in the last place of the type there (eps), not to 1e-6 / 1e-5."""
    fixed16 = route.table == "fixed" and dtype == torch.float16
    gap = 19.0 if fixed16 else 24.0
    tol_dv, tol_zero = (torch.finfo(dtype).eps,) * 2 if route.table == "fixed" else (1e-6, 1e-5)
    entries, failures = {}, []
    for N, H in PROBE_SHAPES:
        g = torch.Generator().manual_seed(7 * N + H)
        v = torch.randn(R.B_CASES, N, 64, generator=g).to(dtype)
        dout = torch.randn(R.B_CASES, N, H * 64, generator=g).to(dtype)
        if dtype == torch.float32:
            v, dout = _bf16_values(v), _bf16_values(dout)
        q = torch.zeros(R.B_CASES, N, H * 64, dtype=dtype)
        k = torch.nn.functional.normalize(torch.randn(R.B_CASES, N, 64, generator=g), dim=-1).to(dtype)
        ldb = (H + 7) // 8 * 8
        for pattern in ("none", "rpad"):
            keymask = R.make_keymask(R.Case("probe", N, H, pattern), g)
            alive = torch.ones(R.B_CASES, N, dtype=torch.bool) if keymask is None else keymask
            for r0 in sorted({r for r in PROBE_R0 + (N - 1,) if r < N}):
                name = f"attn_probe[{route.name},{dtype},N{N}-H{H}-{pattern}-r{r0}]"
                table = torch.zeros(N, ldb)
                table[:, :H] = -gap
                table[r0, :H] = 0.0
                got, problems = run_attention(ops, dev, route, dtype, N, H, q, k, v, dout, table, keymask,
                                              fixed_bound=1e-3 if fixed16 else 1.0)
                on = lambda t: None if t is None else t.to(dev)
                ref = R.reference(on(q), on(k), on(v), on(table), on(keymask), on(dout), H, SCALE, route.P)
                # ---- the one-hot rows: i >= r0 with a live target
                rows = torch.arange(N)
                onehot = (rows[None, :] >= r0) & torch.cat([torch.zeros(R.B_CASES, r0, dtype=torch.bool), alive[:, :N - r0]], 1)     # [B, N]
                avg = ~onehot                                                             # [B, N] rows that average their live keys
                causal = rows[None, :] <= rows[:, None]                                   # [i, j]
                touched = (avg[:, :, None] & causal[None] & alive[:, None, :])            # [B, i, j]: pairs of the averaging rows
                clean_key = ~touched.any(1)                                               # [B, N]
                # dv of the keys no averaging row reaches has its closed form below; against the reference only the others are measured
                # (what is left of a clean key without a target row is N far-below probabilities, under any 16-bit type's smallest number)
                mixed = dict(got, dv=torch.where(clean_key.to(dev)[:, :, None], ref.val["dv"].float(), got["dv"]))
                metrics, over = compare(mixed, ref, dtype)
                n_dead = int((~alive).sum(1).max())
                if int(onehot.sum(1).min()) < N - r0 - n_dead:
                    problems.append("the probe checked too few rows")
                want = torch.zeros(R.B_CASES, N, 64, dtype=dtype)
                want[:, r0:] = v[:, :N - r0]
                want = want[:, :, None, :].expand(R.B_CASES, N, H, 64).to(dev)
                o = got["out"].view(R.B_CASES, N, H, 64)
                sel = onehot.to(dev)
                if dtype == torch.float32:
                    bad = (o - want).abs() > 2e-5 * want.abs().amax(-1, keepdim=True)
                elif route.table == "fixed":        # one unit in the last place of the type, on top of what the other keys can add:
                    # |sum_j p_j (v_j - v_t)| / P_t <= 2 N e^-gap max |v|, which is over a unit only for the smallest elements of v
                    ulp = torch.finfo(dtype).eps * torch.exp2(torch.floor(torch.log2(want.float().abs().clamp(min=torch.finfo(dtype).tiny))))
                    bad = (o.float() - want.float()).abs() > ulp + 2 * N * math.exp(-gap) * float(v.float().abs().max())
                else:
                    bad = o.view(torch.int16) != want.contiguous().view(torch.int16)
                    bad &= ~((o == 0) & (want == 0))              # (+0 and -0 are the same value)
                bad = bad & sel[:, :, None, None]
                if bool(bad.any()):
                    at = [int(x) for x in bad.nonzero()[0]]
                    problems.append(f"out row is not v[i - {r0}] at (b, i, h, d) = {at}")
                # ---- closed forms where no averaging row reaches
                dsum = dout.double().view(R.B_CASES, N, H, 64).sum(2)
                dabs = dout.double().abs().view(R.B_CASES, N, H, 64).sum(2)
                want_dv = torch.zeros(R.B_CASES, N, 64, dtype=torch.float64)
                want_dv[:, :N - r0] = dsum[:, r0:]
                want_dv[~alive] = 0.0
                bound = torch.full((R.B_CASES, N, 64), float(dabs.max()), dtype=torch.float64)
                bound[:, :N - r0] = dabs[:, r0:]
                bound[~alive] = float(dabs.max())
                e_dv = ((got["dv"].double().cpu() - want_dv).abs() / bound)[clean_key]
                metrics["probe_dv"] = float(e_dv.max()) if e_dv.numel() else 0.0
                if metrics["probe_dv"] > tol_dv:
                    problems.append(f"dv is not sum_h dout[j + {r0}]: {metrics['probe_dv']:.2e}")
                floor = lambda t: t.clamp(min=max(1e-6 * float(t.max()), 1e-30))       # (q = 0: dk has no terms at all and must be 0)
                e_dk = float((got["dk"].double().abs() / floor(ref.term["dk"])).max())
                e_dq = (got["dq"].double().abs() / floor(ref.term["dq"]))[sel]
                dist_touched = torch.zeros(N, dtype=torch.bool)
                dist_touched[(rows[:, None] - rows[None, :]).clamp(min=0)[touched.any(0)]] = True
                e_db = (got["dbias"].double().abs() / floor(ref.term["dbias"]))[(~dist_touched).to(dev)]
                metrics.update(probe_dk=e_dk, probe_dq=float(e_dq.max()) if e_dq.numel() else 0.0,
                               probe_dbias=float(e_db.max()) if e_db.numel() else 0.0, rows_checked=int(onehot.sum()))
                for n in ("probe_dk", "probe_dq", "probe_dbias"):
                    if metrics[n] > tol_zero:
                        problems.append(f"{n} {metrics[n]:.2e} > {tol_zero:.0e} of the term sums")
                entries[name] = dict(metrics, problems=problems + over)
                failures += [f"{name}: {p}" for p in problems + over]
    report_all(entries)
    assert not failures, f"{len(failures)} findings, the first: " + "; ".join(failures[:12])


# ---- rows without a live key ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,dtype", PROBE_ROUTES, ids=[f"{r.name}-{str(d).replace('torch.', '')}" for r, d in PROBE_ROUTES])
def test_rows_without_a_live_key(ops, dev, route, dtype):
    """include/omlm.h: a query row without any live key has out = 0, lse = 1e30 and dq = 0 and adds nothing to dk, dv or d(bias); nothing is
    NaN or Inf; every other row meets the ordinary tolerances."""
    entries, failures = {}, []
    for N in (65, 129):
        for s in (1, 33, 64):
            case = R.Case(f"N{N}-H3-dead{s}", N, 3, "dense")
            inp = R.make_inputs(case, dtype, seed=100 * N + s)
            keymask = inp["keymask"].clone()
            keymask[:, :s] = False
            keymask[:, s] = True
            table = table_of(route, dtype, inp)
            got, problems = run_attention(ops, dev, route, dtype, N, 3, inp["q"], inp["k"], inp["v"], inp["dout"], table, keymask)
            on = lambda t: None if t is None else t.to(dev)
            ref = R.reference(on(inp["q"]), on(inp["k"]), on(inp["v"]), on(table), on(keymask), on(inp["dout"]), 3, SCALE, route.P)
            assert bool(ref.dead[:, :s].all()) and not bool(ref.dead[:, s:].any())
            metrics, over = compare(got, ref, dtype)
            problems += [f"Inf in {n}" for n, t in got.items() if bool(torch.isinf(t.float()).any())]
            if float(got["out"][:, :s].float().abs().max()) != 0.0:
                problems.append("out of a row without a live key is not zero")
            if not bool((got["lse"][:, :, :s] == 1.0e30).all()):
                problems.append("lse of a row without a live key is not 1e30")
            if float(got["dq"][:, :s].abs().max()) != 0.0:
                problems.append("dq of a row without a live key is not zero")
            name = f"attn_dead_rows[{route.name},{dtype},{case.name}]"
            entries[name] = dict(metrics, problems=problems + over)
            failures += [f"{name}: {p}" for p in problems + over]
    report_all(entries)
    assert not failures, f"{len(failures)} findings, the first: " + "; ".join(failures[:12])
