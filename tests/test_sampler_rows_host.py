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
