"""Non-causal prefix (non_causal_prefix_size = P > 0), host side: the rel-pos table rows of negative distances against the oracle, the
cached decoder's eligibility by prompt rows, and a JSON stage config reaching the Transformer."""
import json
import types

import pytest
import torch

from oracle import musiclm_oracle as O


def test_relpos_rows_layout():
    from open_musiclm_amd.engine import relpos_rows
    assert relpos_rows(77, 0) == (77, 0)
    assert relpos_rows(77, 1) == (77, 0)                        # one prefix row: no key above the diagonal is live
    assert relpos_rows(77, 33) == (109, -32)
    assert relpos_rows(77, 77) == (153, -76)
    assert relpos_rows(77, 200) == (153, -76)                    # P >= N: every row sees every key


@pytest.mark.parametrize("n,P", [(77, 33), (300, 216), (40, 45)])
def test_t5_buckets_of_negative_distances_match_the_oracle(n, P):
    from open_musiclm_amd.engine import relpos_rows
    from open_musiclm_amd.transformer import t5_bucket_of_distance
    rows, x0 = relpos_rows(n, P)
    r = torch.arange(x0, n)
    got = t5_bucket_of_distance(r)
    assert torch.equal(got, O.t5_bucket(r))
    assert int(got[0]) > 0 if x0 < 0 else True                  # future keys inside the prefix leave bucket 0
    # the table row for distance x sits at x - x0: the same entries as the oracle's [h, 2n - 1] table (distance x at x + n - 1)
    sd = {"rel_pos_bias.relative_attention_bias.weight": torch.randn(32, 4)}
    ref = O.rel_pos_table_t5(sd, "rel_pos_bias.", n)                          # [h, 2n - 1]
    mine = sd["rel_pos_bias.relative_attention_bias.weight"][got]            # [rows, h]
    assert torch.equal(mine.t(), ref[:, x0 + n - 1:])


@pytest.mark.parametrize("n,P", [(50, 14), (90, 90)])
def test_continuous_rows_of_negative_distances_match_the_oracle(n, P):
    """The MLP evaluated at x = x0 + row (omlm_relpos_mlp_fwd / omlm_relpos_first_fwd with x0) is the oracle's table over x0 .. n - 1."""
    from open_musiclm_amd.engine import relpos_rows
    rows, x0 = relpos_rows(n, P)
    g = torch.Generator().manual_seed(3)
    Hd, H = 32, 3
    sd = {"p.net.0.0.weight": torch.randn(Hd, 1, generator=g), "p.net.0.0.bias": torch.randn(Hd, generator=g),
          "p.net.1.0.weight": torch.randn(Hd, Hd, generator=g) / 6, "p.net.1.0.bias": torch.randn(Hd, generator=g),
          "p.net.2.0.weight": torch.randn(Hd, Hd, generator=g) / 6, "p.net.2.0.bias": torch.randn(Hd, generator=g),
          "p.net.3.weight": torch.randn(H, Hd, generator=g), "p.net.3.bias": torch.randn(H, generator=g)}
    x = (x0 + torch.arange(rows, dtype=torch.float32))[:, None]
    silu = torch.nn.functional.silu
    for i in range(3):
        x = silu(x @ sd[f"p.net.{i}.0.weight"].t() + sd[f"p.net.{i}.0.bias"])
    mine = x @ sd["p.net.3.weight"].t() + sd["p.net.3.bias"]                  # [rows, H]
    ref = O.rel_pos_table_continuous(sd, "p.", n)                              # [H, 2n - 1]
    torch.testing.assert_close(mine.t(), ref[:, x0 + n - 1:], rtol=1e-5, atol=1e-5)
    # negative distances are MLP outputs of their own, not a mirror of the positive ones
    if x0 < 0:
        assert not torch.allclose(mine[:-x0 - 1], mine[-x0 + 1:][:-x0 - 1].flip(0))


def _semantic(P, **kw):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_semantic_transformer(dim=128, depth=1, heads=2, clap_codebook_size=64, semantic_codebook_size=64,
                                         non_causal_prefix_size=P, precision="bf16", **kw)


def test_attention_refuses_an_attn_bias_of_another_prefix():
    """An AttnBias is the prepared table of ONE layout (its P): attn_fwd / attn_bwd refuse it for another P before any launch."""
    from open_musiclm_amd import ops
    B, N, H = 1, 40, 2
    q, out = torch.zeros(B * N, H * 64), torch.zeros(B * N, H * 64)
    k = v = torch.zeros(B * N, 64)
    lse = torch.zeros(B, H, N)
    for made, used in ((0, 14), (14, 0), (14, 13)):
        ab = ops.AttnBias(torch.zeros(N + min(made, N) - 1 if made else N, 8), N, H, _tableT=torch.zeros(1), _P=made)
        with pytest.raises(ValueError, match="prepared for P"):
            ops.attn_fwd(q, k, v, ab, None, out, lse, B, N, H, 8.0, P=used)
        with pytest.raises(ValueError, match="prepared for P"):
            ops.attn_bwd(q, k, v, ab, None, out, out, lse, lse, out, k, v, None, B, N, H, 8.0, P=used)


def test_attention_entries_refuse_bad_prefix_and_dropout_args():
    """P < 0 and p outside [0, 1) are refused by the C entries before anything is launched (null tensors here: no GPU needed)."""
    import os
    import __graft_entry__ as G
    from open_musiclm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        G.build()
    lib = hip.lib()
    for dtype in (0, 1, 2):
        for P, p in ((-1, 0.0), (0, 1.0), (3, -0.1), (0, float("nan"))):
            assert lib.omlm_mqa_attn_fwd(*[None] * 8, 1, 77, 2, 8.0, 8, dtype, P, p, 0, None, None) != 0, (dtype, P, p)
            assert lib.omlm_mqa_attn_bwd(*[None] * 15, 1, 77, 2, 8.0, 8, dtype, P, p, 0, None, None) != 0, (dtype, P, p)
    assert lib.omlm_attn_bias_prepare_group(None, None, 1, 77, 2, 8, None, None, 0.0, 8.0, 0, -1, None) != 0
    assert lib.omlm_attn_bias_table_floats(77, 2, 17) > lib.omlm_attn_bias_table_floats(77, 2, 0)


def test_decode_supports_by_prompt_rows():
    from open_musiclm_amd import decode
    causal, pre = _semantic(0), _semantic(14)
    assert decode.supports(causal, 1) and decode.supports(causal, 1, prompt_rows=3)
    assert not decode.supports(pre, 1)                           # backward-compatible call: no prompt known, no cache
    assert not decode.supports(pre, 1, prompt_rows=13)           # a generated row would sit inside the prefix
    assert decode.supports(pre, 1, prompt_rows=14) and decode.supports(pre, 1, prompt_rows=15)
    assert decode.supports(pre, 1, "bf16", prompt_rows=15) == decode.supports(causal, 1, "bf16", prompt_rows=15)


def test_json_stage_config_reaches_the_transformer(tmp_path):
    from open_musiclm_amd import config as C
    cfg = {"dim": 128, "depth": 1, "heads": 2, "non_causal_prefix_size": 14, "relative_position_bias_type": "t5", "ff_dropout": 0.0}
    path = tmp_path / "semantic.json"
    path.write_text(json.dumps(cfg))
    sc = C.SemanticConfig(**json.loads(path.read_text()))
    mc = types.SimpleNamespace(semantic_cfg=sc, clap_rvq_cfg=types.SimpleNamespace(codebook_size=64, rq_num_quantizers=12),
                               hubert_kmeans_cfg=types.SimpleNamespace(codebook_size=64))
    model = C.create_semantic_transformer_from_config(mc, None, "cpu")
    assert model.transformer.non_causal_prefix_size == 14
    assert all(a.non_causal_prefix == 14 for a, _, _ in model.transformer.layers)
    from open_musiclm_amd.engine import prefix_rows
    assert prefix_rows(model.transformer) == 14
