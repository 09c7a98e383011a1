"""Per-row sampling parameters, host side (no GPU): the per_row_* normalisers of ops.py, every refusal generate() and SamplingLoop make
before any device work, and the ctypes mirror of omlm_sample_row_params against include/omlm.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny():
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_coarse_transformer(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                                       acoustic_codebook_size=16, num_clap_quantizers=3, ff_dropout=0.0)


def _wrapper_and_cond(B=3):
    from open_musiclm_amd import open_musiclm as M
    w = M.TokenConditionedTransformerWrapper(transformer=_tiny(), unique_consecutive=False)
    return w, [torch.zeros(B, 1, 3, dtype=torch.long), torch.zeros(B, 3, dtype=torch.long)]


# argument of generate() -> (normaliser, good sequence of 3, bad entries)
def _cases():
    from open_musiclm_amd import ops
    return {
        "temperature": (ops.per_row_temperature, [0.4, 1, 1.7], [0, -1.0, float("nan"), float("inf"), "1", True, 1e-50]),
        "filter_thres": (ops.per_row_filter_thres, [0.0, 0.9, 1], [-0.1, 1.01, float("nan"), "0.9", True]),
        "top_p": (ops.per_row_top_p, [0.05, 0.5, 1.0], [0, -0.5, 1.0001, float("nan"), "0.5", True]),
        "cond_scale": (ops.per_row_cond_scale, [0, 1, 3.5], [-1, float("nan"), float("inf"), "3", 1e39, True]),
        "sampler_seed": (ops.per_row_seed, [0, -1, 2 ** 70 + 5], [1.5, "7", True]),
    }


def test_scalars_come_back_as_they_always_did():
    from open_musiclm_amd import ops
    for x in (0.7, 1, np.float32(0.5), torch.tensor(0.25)):
        for f in (ops.per_row_temperature, ops.per_row_filter_thres):
            got = f(x, 4)
            assert got is x and type(got) is type(x)
    for x in (None, 7, -3, 2 ** 64 + 1):
        assert ops.per_row_seed(x, 4) is x
    assert ops.per_row_top_p(None, 4) == 1.0 and ops.per_row_top_p(0.3, 4) == 0.3 and ops.per_row_top_p(1, 4) == 1.0
    assert ops.per_row_cond_scale(None, 4) is None and ops.per_row_cond_scale(1, 4) is None and ops.per_row_cond_scale(3, 4) == 3.0
    for bad, f in ((0, ops.per_row_top_p), (1.5, ops.per_row_top_p), (-1, ops.per_row_cond_scale)):       # today's checks, today's names
        with pytest.raises(ValueError, match="top_p" if f is ops.per_row_top_p else "cond_scale"):
            f(bad, 4)


@pytest.mark.parametrize("name", ["temperature", "filter_thres", "top_p", "cond_scale", "sampler_seed"])
def test_good_sequences_become_lists_of_checked_numbers(name):
    f, good, _ = _cases()[name]
    want = [v & 0xFFFFFFFFFFFFFFFF for v in good] if name == "sampler_seed" else [float(v) for v in good]
    for seq in (list(good), tuple(good)):
        got = f(seq, 3)
        assert isinstance(got, list) and got == want
        assert all(type(v) is (int if name == "sampler_seed" else float) for v in got)
    if name != "sampler_seed":
        assert f(torch.tensor(want, dtype=torch.float64), 3) == want and f(np.array(want), 3) == want
    else:
        assert f(torch.tensor([1, 2, -3]), 3) == [1, 2, 2 ** 64 - 3] and f(np.array([1, 2, 3]), 3) == [1, 2, 3]
    # cond_scale: a row of scale 1 stays in the list (guidance is on for the whole call)
    if name == "cond_scale":
        assert f([1, 1, 1], 3) == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("name", ["temperature", "filter_thres", "top_p", "cond_scale", "sampler_seed"])
def test_wrong_length_names_the_argument_and_both_lengths(name):
    f, good, _ = _cases()[name]
    for seq, batch in ((good[:2], 3), (good, 2), ([], 1), (torch.tensor([1, 2, 3, 4]), 3)):
        with pytest.raises(ValueError) as e:
            f(seq, batch)
        msg = str(e.value)
        assert name in msg and re.search(r"\b%d\b" % len(seq), msg) and re.search(r"\b%d\b" % batch, msg), msg
    with pytest.raises(ValueError, match=name):
        f(torch.ones(3, 1), 3)                                         # not 1-D


@pytest.mark.parametrize("name", ["temperature", "filter_thres", "top_p", "cond_scale", "sampler_seed"])
def test_bad_entry_names_the_argument_and_the_index(name):
    f, good, bad = _cases()[name]
    for b in bad + [None]:
        for i in range(3):
            seq = list(good)
            seq[i] = b
            with pytest.raises(ValueError, match=re.escape(f"{name}[{i}]")):
                f(seq, 3)


def test_topk_count_is_generates_expression():
    from open_musiclm_amd import ops
    for V1 in (41, 1025, 2049):
        for t in (0.0, 0.5, 0.9, 0.999, 1.0):
            assert ops.topk_count(t, V1) == max(int((1 - t) * V1), 1)
        assert ops.topk_count([0.0, 0.9, 1.0], V1) == [V1, max(int((1 - 0.9) * V1), 1), 1]


def test_generate_refuses_bad_sequences_before_touching_a_device():
    w, cond = _wrapper_and_cond(3)
    for name, (_, good, bad) in _cases().items():
        kw = dict(conditioning_token_ids=cond, max_time_steps=1)
        with pytest.raises(ValueError, match=name):
            w.generate(**kw, **{name: good[:2]})                       # length
        with pytest.raises(ValueError, match=re.escape(f"{name}[1]")):
            w.generate(**kw, **{name: [good[0], bad[0], good[2]]})
        with pytest.raises(ValueError, match=re.escape(f"{name}[2]")):
            w.generate(**kw, **{name: [good[0], good[1], None]})
        for route in (dict(), dict(use_cache=False)):                  # a good sequence gets as far as the device requirement
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                w.generate(**kw, **route, **{name: good})


def test_per_row_seeds_need_the_counter_stream():
    w, cond = _wrapper_and_cond(2)
    kw = dict(conditioning_token_ids=cond, max_time_steps=1, sampler_seed=[1, 2])
    for src in (dict(sampler_rng="buffer"), dict(uniforms=torch.rand(2, 2, 17)), dict(sampler_rng="counter", uniforms=torch.rand(2, 2, 17))):
        with pytest.raises(ValueError) as e:
            w.generate(**kw, **src)
        assert "sampler_seed" in str(e.value) and ("sampler_rng" in str(e.value) or "uniforms" in str(e.value)), str(e.value)
    with pytest.raises(ValueError, match="sampler_seed.*sampler_rng.*uniforms"):
        w.generate(**kw, sampler_rng="buffer")
    with pytest.raises(ValueError, match="sampler_rng must be"):       # an unknown choice is refused as in a call with one seed
        w.generate(**kw, sampler_rng="bogus")
    for src in (dict(), dict(sampler_rng="counter")):                   # None chooses the counter stream
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            w.generate(**kw, **src)
    with pytest.raises(ValueError, match="cond_scale"):                 # score keeps its scalar
        w.score(conditioning_token_ids=cond, pred_token_ids=torch.zeros(2, 1, 2, dtype=torch.long), cond_scale=[2.0, 3.0])


def test_ops_sample_refuses_wrong_row_tensors_by_name():
    from open_musiclm_amd import ops
    lg, out = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    bad = dict(row_k=torch.ones(4, dtype=torch.int64), row_temperature=torch.ones(4, dtype=torch.float64), row_top_p=torch.ones(3),
               row_seed=torch.ones(4, dtype=torch.int32), row_sample=torch.ones(4, 1, dtype=torch.int32))
    for name, t in bad.items():
        with pytest.raises(ValueError, match=name):
            ops.sample(lg, out, 8, 2, 1.0, False, seed=1, **{name: t})
    assert ops.sample_row_params(4, k=None, temperature=None, top_p=None, seed=None, sample=None) is None
    assert ops.row_tensor([0, 2 ** 63, 2 ** 64 - 1], "seed", "cpu").tolist() == [0, -2 ** 63, -1]
    assert ops.row_tensor([1, 5], "k", "cpu").dtype == torch.int32 and ops.row_tensor(None, "k", "cpu") is None
    assert ops.row_tensor([0.5, 3], "scale", "cpu").dtype == torch.float32


def test_settings_cut_slices_lists_and_keeps_scalars():
    from open_musiclm_amd import ops
    temps, scales, seeds = [0.5 + 0.1 * r for r in range(9)], [float(r) for r in range(9)], list(range(100, 109))
    s = ops.SamplerSettings.checked(9, 41, temperature=temps, filter_thres=0.5, top_p=None, cond_scale=scales, sampler_seed=seeds, logprobs=True)
    assert s == ops.SamplerSettings(9, 20, temps, 1.0, scales, seeds, True)
    head, tail = s.cut(0, 8), s.cut(8, 9)
    assert head == ops.SamplerSettings(8, 20, temps[:8], 1.0, scales[:8], seeds[:8], True)
    assert tail == ops.SamplerSettings(1, 20, temps[8:], 1.0, scales[8:], seeds[8:], True)
    assert s.temperature == temps and s.rows == 9                       # the whole is untouched
    t = ops.SamplerSettings.checked(9, 41, temperature=0.8, filter_thres=[0.0] * 8 + [1.0], top_p=[0.7] * 9, cond_scale=3, sampler_seed=None)
    assert t.cut(8, 9) == ops.SamplerSettings(1, [1], 0.8, [0.7], 3.0, None, False) and t.cut(0, 8).k == [41] * 8
    with pytest.raises(AttributeError):
        s.k = 1                                                         # immutable
    # the checks run in generate()'s order, with the caller's own between the guidance and the rest
    order = []
    with pytest.raises(ValueError, match="top_p"):
        ops.SamplerSettings.checked(2, 41, temperature=[0, 0], filter_thres=0.9, top_p=2, cond_scale=3, sampler_seed=None,
                                    after_guidance=order.append)
    assert order == [3.0]
    with pytest.raises(ValueError, match="cond_scale"):
        ops.SamplerSettings.checked(2, 41, temperature=1, filter_thres=0.9, top_p=2, cond_scale=-1, sampler_seed=None, after_guidance=order.append)
    assert order == [3.0]


@pytest.fixture
def recorded_calls(monkeypatch):
    """ops.call replaced by a recorder; no device: tensors count as resident and the stream is 0."""
    from open_musiclm_amd import hip, ops
    calls = []
    monkeypatch.setattr(ops, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "stream_ptr", lambda: 0)
    monkeypatch.setattr(hip, "require_gpu", lambda t, what="tensor": None)
    return calls


def test_one_place_picks_the_sampler_entry(recorded_calls, monkeypatch):
    from open_musiclm_amd import ops
    B, V = 4, 8
    lg, out, lpm, lps = torch.zeros(B, V), torch.zeros(B, dtype=torch.long), torch.zeros(B), torch.zeros(B)
    arrays = dict(row_k=torch.ones(B, dtype=torch.int32), row_temperature=torch.ones(B), row_top_p=torch.ones(B),
                  row_seed=torch.ones(B, dtype=torch.int64), row_sample=torch.zeros(B, dtype=torch.int32))
    lp_forms = (dict(), dict(lp_model=lpm), dict(lp_sampled=lps), dict(lp_model=lpm, lp_sampled=lps))

    blocks = []           # the row block as the call sees it (it lives as long as the call)

    def snapshot(name, *a):
        recorded_calls.append((name, a))
        if name == "omlm_sample_rows":
            block = ops.SampleRowParams.from_address(a[1])
            blocks.append({n: getattr(block, n) for n, _ in block._fields_})
    monkeypatch.setattr(ops, "call", snapshot)

    def entry(**kw):
        del recorded_calls[:]
        ops.sample(lg, out, V, 2, 1.0, False, seed=1, **kw)
        (name, args), = recorded_calls
        return name, args
    assert entry()[0] == "omlm_sample" and len(entry()[1]) == 2            # the block and the stream
    for lp in lp_forms[1:]:
        name, args = entry(**lp)
        assert name == "omlm_sample_lp" and args[1:] == (ops.ptr(lp.get("lp_model")), ops.ptr(lp.get("lp_sampled")), 0)
    for row, lp in ((r, lp) for r in arrays for lp in lp_forms):             # any one row array, with or without lp
        name, args = entry(**{row: arrays[row]}, **lp)
        assert name == "omlm_sample_rows" and args[2:] == (ops.ptr(lp.get("lp_model")), ops.ptr(lp.get("lp_sampled")), 0), (row, lp)
        assert blocks[-1] == {n: arrays[row].data_ptr() if "row_" + n == row else None for n, _ in ops.SampleRowParams._fields_}
    # the pure form SamplingLoop resolves once: the same table, the stream left to the caller
    sa, rows = ops.SampleArgs(), ops.sample_row_params(B, k=arrays["row_k"], temperature=None, top_p=None, seed=None, sample=None)
    assert ops.sampler_call(sa, None) == ("omlm_sample", (C.addressof(sa),))
    assert ops.sampler_call(sa, None, lpm, None) == ("omlm_sample_lp", (C.addressof(sa), lpm.data_ptr(), None))
    assert ops.sampler_call(sa, rows) == ("omlm_sample_rows", (C.addressof(sa), C.addressof(rows), None, None))
    assert ops.sampler_call(sa, rows, lpm, lps) == ("omlm_sample_rows", (C.addressof(sa), C.addressof(rows), lpm.data_ptr(), lps.data_ptr()))


def test_one_place_picks_the_guide_entry(recorded_calls):
    from open_musiclm_amd import ops
    cond, null = torch.zeros(3, 8), torch.ones(3, 8)
    ptrs = (cond.data_ptr(), null.data_ptr(), cond.data_ptr(), 3, 5, 8)
    for given, scale in ((2.5, 2.5), (None, 1.0), (1, 1.0), (0, 0.0)):       # a number: the scalar entry (off is scale 1)
        del recorded_calls[:]
        ops.guide_logits(cond, null, cond, 5, given)
        assert recorded_calls == [("omlm_guide_logits", ptrs + (scale, 0))]
    up = ops.SamplerSettings(3, 1, 1.0, 1.0, [0.0, 1.0, 2.5], None).upload("cpu")       # a list: the row entry
    assert up.guidance.dtype == torch.float32 and up.guidance.tolist() == [0.0, 1.0, 2.5]
    del recorded_calls[:]
    ops.guide_logits(cond, null, cond, 5, up.guidance)
    assert recorded_calls == [("omlm_guide_logits_rows", ptrs + (up.guidance.data_ptr(), 0))]
    assert ops.guide_call(*ptrs, 2.5) == ("omlm_guide_logits", ptrs + (2.5,))
    assert ops.guide_call(*ptrs, up.guidance) == ("omlm_guide_logits_rows", ptrs + (up.guidance.data_ptr(),))
    assert ops.SamplerSettings(3, 1, 1.0, 1.0, 2.5, None).upload("cpu").guidance == 2.5
    assert ops.SamplerSettings(3, 1, 1.0, 1.0, None, None).upload("cpu").guidance is None


def test_upload_puts_placeholders_exactly_where_an_array_stands_in(recorded_calls):
    from open_musiclm_amd import ops
    given = dict(k=[1, 5, 9], temperature=[0.5, 1.0, 1.5], top_p=[0.25, 0.5, 1.0])
    number, placeholder = dict(k=7, temperature=0.75, top_p=0.5), dict(k=1, temperature=1.0, top_p=1.0)
    for lists in ((), ("k",), ("temperature",), ("top_p",), ("k", "top_p"), ("k", "temperature", "top_p")):
        s = ops.SamplerSettings(3, **{m: given[m] if m in lists else number[m] for m in given}, guidance=None, seed=11)
        up = s.upload("cpu")
        for m in given:
            assert getattr(up, m) == (placeholder[m] if m in lists else number[m]) and type(getattr(up, m)) is type(number[m]), (lists, m)
            assert (up.tensors[m].tolist() == given[m] and up.tensors[m].dtype == ops._ROW_DTYPES[m]) if m in lists else up.tensors[m] is None
        assert up.seed == 11 and up.tensors["seed"] is None and up.tensors["sample"] is None and up.rows == 3
        block = up.block()
        assert (block is None) == (not lists)
        if lists:
            assert {n for n, _ in block._fields_ if getattr(block, n)} == set(lists)
    # a seed per row: the seeds as int64 bits, a zero sample index for every row, and no scalar seed
    up = ops.SamplerSettings(3, 7, 0.75, 0.5, None, [0, 2 ** 63, 2 ** 64 - 1]).upload("cpu")
    assert up.seed is None and up.tensors["seed"].tolist() == [0, -2 ** 63, -1] and up.tensors["sample"].tolist() == [0, 0, 0]
    assert up.tensors["sample"].dtype == torch.int32 and (up.k, up.temperature, up.top_p) == (7, 0.75, 0.5)
    block = up.block()
    assert {n for n, _ in block._fields_ if getattr(block, n)} == {"seed", "sample"}


def test_ctypes_mirror_matches_the_header():
    from open_musiclm_amd import hip, ops
    text = open(os.path.join(ROOT, "include", "omlm.h")).read()
    body = re.search(r"typedef struct omlm_sample_row_params \{(.*?)\} omlm_sample_row_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in ops.SampleRowParams._fields_] == ["k", "temperature", "top_p", "seed", "sample"]
    assert all(t is C.c_void_p for _, t in ops.SampleRowParams._fields_) and all("*" in d for d in body.split(";") if d.strip())
    assert C.sizeof(ops.SampleRowParams) == 5 * C.sizeof(C.c_void_p)
    assert set(ops._ROW_DTYPES) == set(fields)
    # the two entry points: declared in the header with the argument counts of the signature table
    for name in ("omlm_sample_rows", "omlm_guide_logits_rows"):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(hip.SIGNATURES[name]), name


def test_sampling_loop_takes_per_row_settings():
    from open_musiclm_amd import decode
    assert decode._guided([1.0, 1.0]) and decode._guided((0.0,)) and decode._guided(torch.ones(2)) and decode._guided(3)
    assert not decode._guided(None) and not decode._guided(1) and not decode._guided(1.0)
    assert decode._per_row_topk(5, 3, 41) == 5 and decode._per_row_topk([1, 41, 7], 3, 41) == [1, 41, 7]
    for bad in (0, 42, 1.0, True, None):
        with pytest.raises(ValueError, match=re.escape("topk[1]")):
            decode._per_row_topk([1, bad, 7], 3, 41)
    with pytest.raises(ValueError, match="topk"):
        decode._per_row_topk([1, 2], 3, 41)
