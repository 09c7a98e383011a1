"""Host side of the decode K/V cache's element type (no GPU): decode.kv_cache_choice, decode.cache_bytes, and generate()'s refusal of an
unknown ``kv_cache`` before any device work."""
import pytest
import torch

from open_musiclm_amd import decode
from open_musiclm_amd import open_musiclm as M

PRECISIONS = ("bf16", "fp16", "fp16ff", "bf16x3")
OPERAND = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp16ff": torch.float16, "bf16x3": torch.float32}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_kv_cache_choice(precision):
    assert decode.kv_cache_choice(None, precision) is torch.float32
    assert decode.kv_cache_choice("fp32", precision) is torch.float32
    assert decode.kv_cache_choice("operand", precision) is OPERAND[precision]


@pytest.mark.parametrize("bad", ["fp8", "", 16])
def test_kv_cache_choice_names_the_accepted_values(bad):
    for precision in PRECISIONS:
        with pytest.raises(ValueError) as e:
            decode.kv_cache_choice(bad, precision)
        text = str(e.value)
        assert "None" in text and "'fp32'" in text and "'operand'" in text and repr(bad) in text, text


def test_cache_bytes():
    """dim 1024, depth 6, B = 64, 1116 rows: K + V of 64 dims per row and layer, 4 bytes each in fp32 and 2 in the fp16 operand type."""
    model = M.create_coarse_transformer(dim=1024, depth=6, heads=8, num_coarse_quantizers=3, precision="fp16ff")
    full = 64 * 1116 * 64 * 2 * 6 * 4
    assert decode.cache_bytes(model, 64, 1116, "fp16ff") == full
    assert decode.cache_bytes(model, 64, 1116, "fp16ff", kv_cache="fp32") == full
    assert decode.cache_bytes(model, 64, 1116, "fp16ff", kv_cache="operand") * 2 == full
    assert decode.cache_bytes(model, 64, 1116, "bf16", kv_cache="operand") * 2 == full
    assert decode.cache_bytes(model, 64, 1116, "bf16x3", kv_cache="operand") == decode.cache_bytes(model, 64, 1116, "bf16x3") == full
    with pytest.raises(ValueError):
        decode.cache_bytes(model, 64, 1116, "fp16ff", kv_cache="fp8")


def test_decode_args_end_with_the_cache_type_members():
    """kv16 / k_new are appended: every member that existed keeps its offset (the layout tests compare the whole struct with the header)."""
    names = [f[0] for f in decode.DecodeArgs._fields_]
    assert names[-2:] == ["kv16", "k_new"] and names[-4:-2] == ["splitk_ws", "splitk_cnt"]


def _tiny_cpu():
    torch.manual_seed(0)
    model = M.create_coarse_transformer(dim=64, depth=1, heads=1, num_coarse_quantizers=3, clap_codebook_size=16, semantic_codebook_size=16,
                                        acoustic_codebook_size=16, precision="fp16")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    cond = [torch.randint(0, 16, (2, 12, 1)), torch.randint(0, 16, (2, 5))]
    return model, wrapper, cond


@pytest.mark.parametrize("bad", ["fp8", "", 16])
def test_generate_refuses_an_unknown_kv_cache_before_any_device_work(bad):
    """A CPU model: the ValueError comes before anything asks for the GPU (the next thing a valid call on it meets is hip.require_gpu)."""
    _, wrapper, cond = _tiny_cpu()
    with pytest.raises(ValueError) as e:
        wrapper.generate(conditioning_token_ids=cond, max_time_steps=2, kv_cache=bad)
    assert "'operand'" in str(e.value) and "'fp32'" in str(e.value)


def test_musiclm_forward_refuses_an_unknown_kv_cache_before_any_stage_runs():
    kw = dict(dim=64, depth=1, heads=1, precision="fp16")
    mlm = M.MusicLM(semantic_transformer=M.create_semantic_transformer(**kw), coarse_transformer=M.create_coarse_transformer(**kw),
                    fine_transformer=M.create_fine_transformer(**kw))
    called = []
    mlm.semantic.generate = lambda **k: called.append(k)
    with pytest.raises(ValueError) as e:
        mlm(clap_token_ids=torch.zeros(1, 12, 1, dtype=torch.long), kv_cache="fp8", return_tokens=True)
    assert "'operand'" in str(e.value) and not called
