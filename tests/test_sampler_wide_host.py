"""Host side of the wide sampler: the width limit (ops.SAMPLER_MAX_V), its refusal before any device work on every way into the
sampler, and the unchanged C ABI of the three sampler entry points.  No GPU."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parameter lists of include/omlm.h as they were before the wide kernel (whitespace-normalised)
SAMPLER_ABI = {
    "omlm_sample_topk_gumbel": "const float* logits, const float* uniform, long long* out, int B, int V, int ld, int k, float temperature, "
                               "int forbid_last, void* stream",
    "omlm_sample_topk_gumbel_at": "const float* logits, const float* uniform_base, const int* step_dev, long long* out, long long* hist, "
                                  "int B, int V, int ld, int k, float temperature, int forbid_last, void* stream",
    "omlm_sample_embed_at": "const float* logits, const float* uniform_base, const int* step_dev, long long* out, long long* hist, int B, "
                            "int V, int ld, int k, float temperature, int forbid_last, const float* emb_table, long long emb_row_offset, "
                            "long long emb_rows, float* x, int D, void* stream",
}


@pytest.fixture
def no_device_calls(monkeypatch):
    """Any call into the library (or an attempt to load it) fails the test."""
    from open_musiclm_amd import decode, hip, ops

    def refuse(*a, **k):
        raise AssertionError(f"device call before the width check: {a[:1]}")
    for mod in (hip, ops, decode):
        monkeypatch.setattr(mod, "call", refuse)
    monkeypatch.setattr(hip, "lib", refuse)


def test_limit_constant_and_message():
    from open_musiclm_amd import ops
    assert ops.SAMPLER_MAX_V == 65536
    ops.check_sampler_width(65536)
    ops.check_sampler_width(1)
    with pytest.raises(ValueError) as e:
        ops.check_sampler_width(65537)
    assert "65536" in str(e.value) and "codebook" in str(e.value)


def test_sample_topk_gumbel_refuses_before_any_launch(no_device_calls):
    from open_musiclm_amd import ops
    V = 65537
    out = torch.full((2,), -7, dtype=torch.long)
    with pytest.raises(ValueError, match="65536"):
        ops.sample_topk_gumbel(torch.zeros(2, V), torch.zeros(2, V), out, V, 10, 1.0, True)
    assert out.tolist() == [-7, -7]


def test_sampling_loop_refuses_before_any_launch(no_device_calls):
    """SamplingLoop checks the decoder's row width first: nothing of the decoder but V1 is touched."""
    from open_musiclm_amd import decode
    dec = types.SimpleNamespace(V1=65537)
    with pytest.raises(ValueError, match="65536"):
        decode.SamplingLoop(dec, None, None, 0, 4, 10, 1.0, [True])


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_refuses_a_codebook_of_65536_entries_on_a_cpu_only_box(no_device_calls, use_cache):
    """A model whose predicted codebook has 65536 entries (V = 65537) builds and trains, and generate() says at once why it cannot
    sample -- a ValueError naming codebook size and limit, not the no-GPU RuntimeError that the first device call would raise."""
    from open_musiclm_amd import open_musiclm as M
    model = M.create_semantic_transformer(dim=64, depth=1, heads=1, clap_codebook_size=32, num_clap_quantizers=2,
                                          semantic_codebook_size=65536, ff_dropout=0.0, precision="bf16x3")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    with pytest.raises(ValueError) as e:
        wrapper.generate(conditioning_token_ids=[torch.zeros(1, 2, 2, dtype=torch.long)], max_time_steps=2, use_cache=use_cache)
    assert "65536" in str(e.value) and "codebook" in str(e.value)


def test_sampler_abi_is_unchanged():
    """include/omlm.h declares the three sampler entry points with the parameter lists they have always had, hip.py binds as many
    arguments, and the header states the limit."""
    from open_musiclm_amd import hip
    text = open(os.path.join(ROOT, "include", "omlm.h")).read()
    for name, params in SAMPLER_ABI.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        got = re.sub(r"\s+", " ", m.group(1)).strip()
        assert got == params, (name, got)
        assert len(hip.SIGNATURES[name]) == params.count(",") + 1, name
    assert "65536" in text[text.index("AR sampler"):text.index("int omlm_sample_topk_gumbel(")]
