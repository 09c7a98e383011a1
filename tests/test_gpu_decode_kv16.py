"""The decode K/V cache in the 16-bit operand type (CachedDecoder(kv_cache="operand"), omlm_decode_args::kv16) on the GPU.

The step kernels round every key and value to the operand type before they store them, so the 16-bit cache must hold the fp32 cache's
numbers and give the same logits BIT FOR BIT on every route: the first-generation kernels (dim != 1024), dec3 (dim 1024, B = 1), dec4
(matrix cores, B >= 2), the wide call (B > 16: groups of 16 with a per-group cache offset) and dec2 (dim 1024 where dec4 refuses the
geometry).

Prompts are those of test_gpu_decode_wide._prompt with 60 prompt rows and 8 teacher-forced steps, the caches hold Nmax = 70 rows (no
multiple of 64): pos runs 60..67, i.e. from the first 64-key range into the second; at pos = 64 the second range holds the new key only
(nk = 1) and the first is full without a new key in it."""
import ctypes as C

import pytest
import torch

from test_gpu_model import TOL, relerr, report

pytestmark = pytest.mark.gpu

V1 = 1025
NMAX = 70
PROMPT_ROWS = 60
STEPS = 8
_MODELS = {}
_RUNS = {}

# name: (model key, precision, B, wide, route)
CASES = {
    "gen1-bf16-B1": ("small", "bf16", 1, False, "gen1"),
    "gen1-bf16-B3": ("small", "bf16", 3, False, "gen1"),
    "gen1-fp16-B1": ("small", "fp16", 1, False, "gen1"),
    "gen1-fp16-B3": ("small", "fp16", 3, False, "gen1"),
    "dec3-bf16-B1": ("d1024", "bf16", 1, False, "dec3"),
    "dec3-fp16ff-B1": ("d1024", "fp16ff", 1, False, "dec3"),
    "dec4-bf16-B3": ("d1024", "bf16", 3, False, "dec4"),
    "dec4-fp16-B3": ("d1024", "fp16", 3, False, "dec4"),
    "dec4-fp16ff-B3": ("d1024", "fp16ff", 3, False, "dec4"),
    "wide-fp16ff-B17": ("d1024", "fp16ff", 17, True, "dec4"),
    "dec2-fp16-B2": ("plainff", "fp16", 2, False, "dec2"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from open_musiclm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _model(dev, key, precision):
    """One depth-2 coarse model per (geometry, precision), shared by the tests of this file and never modified.  small: dim 128, 2 heads
    (first-generation step kernels); d1024: dim 1024, 8 heads; plainff: dim 1024 with a plain FeedForward (F = Fp = 4096 > 3072: the
    second-generation kernels without the matrix cores)."""
    from open_musiclm_amd import open_musiclm as M
    if (key, precision) not in _MODELS:
        geo = {"small": dict(dim=128, heads=2), "d1024": dict(dim=1024, heads=8), "plainff": dict(dim=1024, heads=8, use_conv_ff=False)}[key]
        torch.manual_seed(0)
        m = M.create_coarse_transformer(depth=2, ff_dropout=0.0, num_coarse_quantizers=3, precision=precision, **geo).to(dev)
        m.eval()
        _MODELS[(key, precision)] = (m, M.TokenConditionedTransformerWrapper(transformer=m, unique_consecutive=False))
    return _MODELS[(key, precision)]


def _prompt(wrapper, dev, B, n=STEPS + 1, seed=3):
    """test_gpu_decode_wide._prompt with 43 instead of 40 semantic ids: (12 + 2) + (43 + 2) + 1 = 60 prompt rows."""
    from open_musiclm_amd.utils import append_eos_id
    g = torch.Generator().manual_seed(seed)
    cond = [torch.randint(0, 1024, (B, 12, 1), generator=g), torch.randint(0, 1024, (B, 43), generator=g)]
    flat = torch.randint(0, 1024, (B, n), generator=g)
    condx = [append_eos_id(t.reshape(B, -1).long(), e) for t, e in zip(cond, wrapper.eos_ids)]
    assert sum(t.shape[-1] + 1 for t in condx) + 1 == PROMPT_ROWS
    return [t.to(dev) for t in condx], flat.to(dev)


def _steps(model, condx, flat, precision, B, wide, kv_cache):
    """prefill + 8 teacher-forced steps: the decoder and the list of [B, V1] logits (clones); pos of the steps = 60..67."""
    from open_musiclm_amd import decode
    dec = decode.CachedDecoder(model, B, NMAX, precision, wide=wide, kv_cache=kv_cache)
    got = [dec.prefill(condx + [flat[:, :0]])[:, :V1].clone()]
    assert dec.rows == PROMPT_ROWS
    for k in range(flat.shape[1] - 1):
        got.append(dec.step(flat[:, k].contiguous(), k)[:, :V1].clone())
    assert dec.rows == PROMPT_ROWS + STEPS and int(dec.pos_dev.item()) == dec.rows
    return dec, got


def _run(dev, case):
    """Both decoders of a case, run once and shared by the tests below (nothing modifies them afterwards)."""
    if case not in _RUNS:
        key, precision, B, wide, _ = CASES[case]
        model, wrapper = _model(dev, key, precision)
        condx, flat = _prompt(wrapper, dev, B)
        with torch.no_grad():
            dec32, got32 = _steps(model, condx, flat, precision, B, wide, None)
            dec16, got16 = _steps(model, condx, flat, precision, B, wide, "operand")
        _RUNS[case] = dict(model=model, condx=condx, flat=flat, dec32=dec32, dec16=dec16, got32=got32, got16=got16)
    return _RUNS[case]


def _assert_route(case):
    from open_musiclm_amd import decode
    key, precision, B, wide, route = CASES[case]
    model = _MODELS[(key, precision)][0]
    D, H, Fp = decode._geometry(model)
    assert decode.step_route(B, D, H, Fp, True, wide) == route          # (every precision of CASES has 16-bit weights)
    if route == "gen1":
        assert D != 1024
    elif route == "dec3":
        assert D == 1024 and B == 1
    elif route == "dec4":
        assert D == 1024 and B >= 2
        assert (B > decode.DEC4_NB) == wide
    else:
        assert route == "dec2" and B >= 2 and D == 1024 and Fp > 3072


@pytest.mark.parametrize("case", list(CASES))
def test_same_bits_on_every_route(dev, case):
    """1. The logits of the prefill and of every step are equal bit for bit between the fp32 and the 16-bit cache."""
    r = _run(dev, case)
    _assert_route(case)
    assert r["dec32"].kv_dtype == torch.float32 and r["dec16"].kv_dtype == r["dec16"].T and r["dec16"].T != torch.float32
    assert len(r["got32"]) == len(r["got16"]) == STEPS + 1
    for k, (x, y) in enumerate(zip(r["got32"], r["got16"])):
        assert torch.isfinite(x).all() and torch.isfinite(y).all(), (case, k)
        assert torch.equal(x, y), (case, k, float((x - y).abs().max()))
    # the steps did something: consecutive logits differ
    assert not torch.equal(r["got16"][-1], r["got16"][-2])


@pytest.mark.parametrize("case", list(CASES))
def test_the_cache_is_the_fp32_cache_narrowed(dev, case):
    """2. After the steps every cached key and value equals the fp32 cache's, in 2-byte elements, and every ticket counter is zero again."""
    r = _run(dev, case)
    dec32, dec16 = r["dec32"], r["dec16"]
    n = dec16.rows
    assert n == PROMPT_ROWS + STEPS
    for l in range(dec16.L):
        assert dec16.Kc[l].element_size() == 2 and dec16.Vc[l].element_size() == 2 and dec32.Kc[l].element_size() == 4
        assert dec16.Kc[l].dtype == dec16.T and dec16.Kc[l].shape == dec32.Kc[l].shape == (dec16.B, NMAX, 64)
        assert torch.equal(dec16.Kc[l][:, :n].float(), dec32.Kc[l][:, :n]), (case, l, "K")
        assert torch.equal(dec16.Vc[l][:, :n].float(), dec32.Vc[l][:, :n]), (case, l, "V")
        assert float(dec16.Kc[l][:, PROMPT_ROWS:n].float().abs().max()) > 0          # the steps' keys are there (unit rows x k_scale)
        assert float(dec16.Kc[l][:, n:].float().abs().max()) == 0 and float(dec16.Vc[l][:, n:].float().abs().max()) == 0   # and nothing past them
    assert int(dec16.splitk_cnt.abs().sum()) == 0 and int(dec32.splitk_cnt.abs().sum()) == 0


def test_operand_cache_against_the_reforward(dev):
    """3. fp16ff, B = 3: the 16-bit-cache logits against model.last_logits of the growing sequence, under the mode's own bar."""
    case = "dec4-fp16ff-B3"
    r = _run(dev, case)
    flat = r["flat"]
    with torch.no_grad():
        want = [r["model"].last_logits(r["condx"] + [flat[:, :k]])[:, :V1].clone() for k in range(flat.shape[1])]
    err = max(relerr(x, y) for x, y in zip(r["got16"], want))
    print(f"kv16 steps vs re-forward [fp16ff, B=3]: max rel err {err:.3e}")
    report("decode_kv16_vs_reforward[fp16ff,B=3]", max_rel_err=err, steps=len(want))
    assert r["dec16"].planes
    assert err < TOL["fp16ff"]["logits"], err


def _spies(monkeypatch):
    """Record the cache dtype of every CachedDecoder and every SamplingLoop that generate() builds."""
    from open_musiclm_amd import decode
    decs, loops = [], []
    orig_dec, orig_loop = decode.CachedDecoder, decode.SamplingLoop

    class DecSpy(orig_dec):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            decs.append(self)

    class LoopSpy(orig_loop):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            loops.append(self)
    monkeypatch.setattr(decode, "CachedDecoder", DecSpy)
    monkeypatch.setattr(decode, "SamplingLoop", LoopSpy)
    return decs, loops


def _cond(B, g, dev):
    return [torch.randint(0, 1024, (B, 12, 1), generator=g).to(dev), torch.randint(0, 1024, (B, 40), generator=g).to(dev)]


@pytest.mark.parametrize("name", ["B3", "B17-top_p", "counter", "counter-graph"])
def test_generate_gives_the_same_ids(dev, monkeypatch, name):
    """4. wrapper.generate(kv_cache="operand") equals the default call id for id (dim 1024, depth 2, fp16ff, 3 quantizers; 57 prompt rows,
    so the 12 or 18 ids cross row 64).  counter-graph: 6 time steps with use_graph=True -- every quantizer phase is captured and replayed."""
    precision, Q = "fp16ff", 3
    model, wrapper = _model(dev, "d1024", precision)
    decs, loops = _spies(monkeypatch)
    g = torch.Generator().manual_seed(31)
    B, steps, extra = {"B3": (3, 4, {}), "B17-top_p": (17, 4, dict(top_p=0.9)), "counter": (3, 4, dict(sampler_rng="counter", sampler_seed=1234)),
                       "counter-graph": (3, 6, dict(sampler_rng="counter", sampler_seed=99, use_graph=True))}[name]
    kw = dict(conditioning_token_ids=_cond(B, g, dev), max_time_steps=steps, **extra)
    if "sampler_rng" not in extra:
        kw["uniforms"] = torch.rand(steps * Q, B, V1, generator=g)
    want = wrapper.generate(**kw)
    got = wrapper.generate(kv_cache="operand", **kw)
    assert [d.kv_dtype for d in decs] == [torch.float32, torch.float16] and [d.B for d in decs] == [B, B]
    assert decs[1].Kc[0].dtype == torch.float16 and decs[1].args.kv16 == 1 and decs[0].args.kv16 == 0
    assert want.shape == (B, steps, Q) and int(want.min()) >= 0 and int(want.max()) < 1024
    assert torch.equal(got, want), (name, int((got != want).sum()))
    if extra.get("use_graph"):
        assert all(len(lp.graphs) == Q and lp.use_graph for lp in loops), "the cycles were not captured"
    assert int(decs[1].splitk_cnt.abs().sum()) == 0
    # a valid value on the re-forward route (no cache) has no effect
    if name == "B3":
        short = dict(kw, max_time_steps=1, uniforms=kw["uniforms"][:Q], use_cache=False)
        assert torch.equal(wrapper.generate(kv_cache="operand", **short), wrapper.generate(**short))


def test_bf16x3_keeps_its_fp32_cache(dev):
    """5. "bf16x3": the operand type is fp32, so kv_cache="operand" allocates what the default allocates and gives the same logits."""
    precision, B = "bf16x3", 2
    model, wrapper = _model(dev, "small", precision)
    condx, flat = _prompt(wrapper, dev, B)
    with torch.no_grad():
        dec32, got32 = _steps(model, condx, flat, precision, B, False, None)
        dec16, got16 = _steps(model, condx, flat, precision, B, False, "operand")
    assert dec16.kv_dtype == torch.float32 and dec16.Kc[0].dtype == torch.float32 and dec16.k_new is None and dec16.args.kv16 == 0
    for k, (x, y) in enumerate(zip(got32, got16)):
        assert torch.equal(x, y), k
    for l in range(dec16.L):
        assert torch.equal(dec16.Kc[l], dec32.Kc[l]) and torch.equal(dec16.Vc[l], dec32.Vc[l])


def test_kv16_is_refused_at_the_c_boundary(dev):
    """6. omlm_decode_step with kv16 set returns the library's argument error when the cached values would not be 16-bit numbers
    (round_bf16 = 0, or fp32 weights) or when k_new is NULL; no kernel runs: the row index, the logits and the caches are untouched."""
    from open_musiclm_amd import decode, hip
    r = _run(dev, "gen1-bf16-B1")
    dec = r["dec16"]
    ids = r["flat"][:, 0].contiguous()
    before = dict(pos=int(dec.pos_dev.item()), logits=dec.logits.clone(), K=[t.clone() for t in dec.Kc], k_new=dec.k_new.clone())
    step = hip.lib().omlm_decode_step
    for change in (dict(round_bf16=0), dict(k_new=None), dict(w_dtype=0)):
        a = decode.DecodeArgs()
        C.memmove(C.addressof(a), C.addressof(dec.args), C.sizeof(a))
        assert a.kv16 == 1 and a.k_new == dec.k_new.data_ptr()
        a.emb_table, a.head_W = dec.emb.data_ptr(), dec.pw.heads[-1][0].data_ptr()
        for n, v in change.items():
            setattr(a, n, v)
        rc = step(C.addressof(a), hip.ptr(ids), hip.stream_ptr())
        assert rc == -1, (change, rc)
        assert b"kv16" in hip.lib().omlm_last_error(), change
    torch.cuda.synchronize()
    assert int(dec.pos_dev.item()) == before["pos"] and torch.equal(dec.logits, before["logits"]) and torch.equal(dec.k_new, before["k_new"])
    assert all(torch.equal(x, y) for x, y in zip(dec.Kc, before["K"]))
