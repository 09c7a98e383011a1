"""The sampler's counter-based uniform stream without a GPU: quality of the stream as restated in tests/sampler_stream_ref.py, the law of
the ids it samples, the rule that chooses between buffer and stream, the header / binding surface of the three new entry points, and
the width refusal before any device work on the stream's ways into the sampler."""
import os
import re
import types

import numpy as np
import pytest
import torch

import loss_optim_sampler_ref as R
import sampler_stream_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 0x9E3779B97F4A7C15]
T_, B_, C_ = 64, 16, 4096                              # 2^22 draws per seed
CHI2_1023_BOUND = 1023 + 6 * (2 * 1023) ** 0.5         # mean + 6 standard deviations of chi^2 with 1023 degrees of freedom: 1294.4
CHI2_15_BOUND = 15 + 6 * 30 ** 0.5                     # the same for 15 degrees of freedom: 47.9

_WORDS = {}


def _words(seed):
    if seed not in _WORDS:
        w = S.words(seed, T_, B_, C_)
        w.setflags(write=False)
        _WORDS[seed] = w
    return _WORDS[seed]


def _chi2(cells, n_cells):
    counts = np.bincount(np.asarray(cells, dtype=np.int64).ravel(), minlength=n_cells).astype(np.float64)
    assert counts.shape[0] == n_cells
    e = counts.sum() / n_cells
    return float(((counts - e) ** 2).sum() / e)


def _pair(a, b):
    """1024 cells from the top 5 bits of two words."""
    return (a >> np.uint64(27)) * np.uint64(32) + (b >> np.uint64(27))


@pytest.mark.parametrize("seed", SEEDS)
def test_stream_is_uniform_and_unlinked_along_every_axis(seed):
    """chi^2 over 1024 cells of the top 10 bits, of bits 8-17 (the low end of the 24 bits a uniform keeps) and of the top 5 bits of
    neighbouring draws along c, t, b and the seed: each below mean + 6 sigma of chi^2_1023.  (Measured with the header's formula:
    939 .. 1151 over the three seeds.)"""
    w = _words(seed)
    assert w.shape == (T_, B_, C_) and int(w.max()) < 2 ** 32
    got = {
        "top10": _chi2(w >> np.uint64(22), 1024),
        "bits8_17": _chi2((w >> np.uint64(8)) & np.uint64(1023), 1024),
        "pair_c": _chi2(_pair(w[:, :, :-1], w[:, :, 1:]), 1024),
        "pair_t": _chi2(_pair(w[:-1], w[1:]), 1024),
        "pair_b": _chi2(_pair(w[:, :-1], w[:, 1:]), 1024),
        "pair_seed": _chi2(_pair(w, S.words(seed + 1, T_, B_, C_)), 1024),
    }
    print(f"sampler stream chi2 (seed {seed:#x}): " + ", ".join(f"{k} {v:.0f}" for k, v in got.items()))
    for name, v in got.items():
        assert v < CHI2_1023_BOUND, (name, v)


def test_seeds_0_and_1_share_no_step():
    """The defect of the first formula (key = h(t ^ seed_lo) ...): seeds s and s ^ 1 were one stream with steps swapped pairwise.  No
    step of seed 0 holds the same set of draws as any step of seed 1."""
    a, b = _words(0), _words(1)
    digest = lambda w: {np.sort(w[t].ravel()).tobytes() for t in range(T_)}          # noqa: E731
    da, db = digest(a), digest(b)
    assert len(da) == T_ and len(db) == T_ and not (da & db)


def test_uniforms_are_the_24_bit_grid():
    u = S.uniforms(3, 2, 3, 257, row0=5, t0=7)
    assert u.dtype == np.float32 and u.shape == (2, 3, 257) and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal(u.astype(np.float64) * 2 ** 24, np.floor(u.astype(np.float64) * 2 ** 24))
    # row0 / t0 shift the coordinates: a slice of a larger call is the smaller call
    big = S.uniforms(3, 9, 8, 257)
    assert np.array_equal(big[7:9, 5:8], u)


@pytest.mark.parametrize("seed", SEEDS)
def test_sampling_law(seed):
    """Ids sampled by the sampler's rule (loss_optim_sampler_ref) from the stream's uniforms follow softmax(l / T) over the kept set:
    64 logits, k = 16, T = 0.7, 4096 steps x 16 rows; chi^2 with 15 degrees of freedom below mean + 6 sigma = 47.9 (measured 24.5, 19.3,
    23.9); smallest expected count 455."""
    logits = np.float32(np.random.default_rng(0).standard_normal(64) * 2)
    k, T, steps, B = 16, 0.7, 4096, 16
    u = torch.from_numpy(S.uniforms(seed, steps, B, 64)).reshape(steps * B, 64)
    lg = torch.from_numpy(logits)[None].expand(steps * B, 64)
    ids = R.sample(lg, u, k, T, False).numpy()
    kept = R.kept_mask(lg[:1], k, False)[0].numpy()
    assert int(kept.sum()) == k
    p = np.where(kept, np.exp((logits.astype(np.float64) - logits.max()) / T), 0.0)
    p /= p.sum()
    expected = p * steps * B
    counts = np.bincount(ids, minlength=64).astype(np.float64)
    assert counts[~kept].sum() == 0
    chi2 = float((((counts - expected) ** 2)[kept] / expected[kept]).sum())
    print(f"sampler stream law (seed {seed:#x}): chi2_15 {chi2:.1f}, smallest expected count {expected[kept].min():.0f}")
    assert expected[kept].min() > 400
    assert chi2 < CHI2_15_BOUND, chi2


def test_sampler_rng_choice():
    from open_musiclm_amd import decode
    choose = decode.sampler_rng_choice
    assert decode.UNIFORM_BUFFER_MAX_BYTES == 1 << 30
    # the shipped coarse stage at B = 64 (590 MB) keeps the buffer; V1 = 8193 at B = 64 (4.7 GB) moves to the stream
    assert choose(None, 2250, 64, 1025, False) == "buffer"
    assert choose(None, 2250, 64, 8193, False) == "counter"
    # the line itself: 2^28 floats are 1 GiB
    assert choose(None, 1 << 14, 1 << 4, 1 << 10, False) == "buffer"
    assert choose(None, (1 << 14) + 1, 1 << 4, 1 << 10, False) == "counter"
    # injected draws are a buffer whatever their size; explicit requests hold on both sides of the line
    assert choose(None, 2250, 64, 8193, True) == "buffer"
    assert choose("buffer", 2250, 64, 8193, False) == "buffer"
    assert choose("buffer", 2250, 64, 8193, True) == "buffer"
    assert choose("counter", 4, 1, 65, False) == "counter"
    with pytest.raises(ValueError, match="counter"):
        choose("counter", 4, 1, 65, True)
    for bad in ("philox", "", "Counter"):
        with pytest.raises(ValueError, match="sampler_rng"):
            choose(bad, 4, 1, 65, False)


def test_header_declares_the_stream_entry_points():
    """include/omlm.h declares the three entry points with the stream's definition beside them; hip.SIGNATURES binds as many arguments."""
    from open_musiclm_amd import hip
    text = open(os.path.join(ROOT, "include", "omlm.h")).read()
    want = {
        "omlm_sample_topk_gumbel_rng": "const float* logits, unsigned seed_lo, unsigned seed_hi, int step, int row0, long long* out, int B, "
                                       "int V, int ld, int k, float temperature, int forbid_last, void* stream",
        "omlm_sample_topk_gumbel_at_rng": "const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0, "
                                          "long long* out, long long* hist, int B, int V, int ld, int k, float temperature, "
                                          "int forbid_last, void* stream",
        "omlm_sample_embed_at_rng": "const float* logits, unsigned seed_lo, unsigned seed_hi, const int* step_dev, int row0, long long* out, "
                                    "long long* hist, int B, int V, int ld, int k, float temperature, int forbid_last, "
                                    "const float* emb_table, long long emb_row_offset, long long emb_rows, float* x, int D, void* stream",
    }
    first = None
    for name, params in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        assert len(hip.SIGNATURES[name]) == params.count(",") + 1, name
        first = m.start() if first is None else min(first, m.start())
    comment = text[text.rindex("/*", 0, first):first]
    for piece in ("lowbias32", "s0", "h(h(seed_lo) ^ seed_hi)", "h(h(s0 + t * 0x9E3779B9) ^ (b * 0x85EBCA6B))", "h(key(t, b) ^ (c * 0x9E3779B9))",
                  "(r >> 8) * 2^-24", "row0"):
        assert piece in comment, piece


@pytest.fixture
def no_device_calls(monkeypatch):
    """Any call into the library (or an attempt to load it) fails the test."""
    from open_musiclm_amd import decode, hip, ops

    def refuse(*a, **k):
        raise AssertionError(f"device call before the width check: {a[:1]}")
    for mod in (hip, ops, decode):
        monkeypatch.setattr(mod, "call", refuse)
    monkeypatch.setattr(hip, "lib", refuse)


def test_sample_topk_gumbel_rng_refuses_before_any_launch(no_device_calls):
    from open_musiclm_amd import ops
    V = 65537
    out = torch.full((2,), -7, dtype=torch.long)
    with pytest.raises(ValueError, match="65536"):
        ops.sample_topk_gumbel_rng(torch.zeros(2, V), 0, 0, 0, out, V, 10, 1.0, True)
    assert out.tolist() == [-7, -7]


def test_sampling_loop_on_the_stream_refuses_before_any_launch(no_device_calls):
    from open_musiclm_amd import decode
    dec = types.SimpleNamespace(V1=65537)
    with pytest.raises(ValueError, match="65536"):
        decode.SamplingLoop(dec, None, None, 0, 4, 10, 1.0, [True], rng=(0, 0))


def test_sampling_loop_wants_exactly_one_source(no_device_calls):
    from open_musiclm_amd import decode
    dec = types.SimpleNamespace(V1=65, B=1)
    with pytest.raises(ValueError, match="either"):
        decode.SamplingLoop(dec, None, None, 0, 4, 6, 1.0, [True])
    with pytest.raises(ValueError, match="either"):
        decode.SamplingLoop(dec, None, torch.zeros(4, 1, 65), 0, 4, 6, 1.0, [True], rng=(0, 0))


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_on_the_stream_refuses_a_codebook_of_65536_entries(no_device_calls, use_cache):
    from open_musiclm_amd import open_musiclm as M
    model = M.create_semantic_transformer(dim=64, depth=1, heads=1, clap_codebook_size=32, num_clap_quantizers=2,
                                          semantic_codebook_size=65536, ff_dropout=0.0, precision="bf16x3")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    with pytest.raises(ValueError) as e:
        wrapper.generate(conditioning_token_ids=[torch.zeros(1, 2, 2, dtype=torch.long)], max_time_steps=2, use_cache=use_cache,
                         sampler_rng="counter", sampler_seed=0)
    assert "65536" in str(e.value) and "codebook" in str(e.value)


def test_split_seed():
    from open_musiclm_amd import ops
    assert ops.split_seed(0x9E3779B97F4A7C15) == (0x7F4A7C15, 0x9E3779B9)
    assert ops.split_seed(-1) == (0xFFFFFFFF, 0xFFFFFFFF) and ops.split_seed(1) == (1, 0)
