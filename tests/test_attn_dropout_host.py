"""Attention dropout without a GPU: construction, the documented keep-mask (numpy restatement) and the seed bookkeeping."""
import numpy as np
import pytest
import torch

import attn_dropout_ref as R


def test_coarse_transformer_with_attn_dropout_constructs_and_loads_reference_state_dict(golden_dir):
    import os
    from open_musiclm_amd import open_musiclm as M
    z = np.load(os.path.join(golden_dir, "tiny_coarse.npz"))
    import ast
    kwargs = ast.literal_eval(str(z["meta.kwargs"]))
    kwargs["attn_dropout"] = 0.1
    model = M.create_coarse_transformer(**kwargs)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    model.load_state_dict(sd, strict=True)
    for attn, _, _ in model.transformer.layers:
        assert attn.attn_dropout.p == 0.1 and attn.to_out[1].p == 0.1


@pytest.mark.parametrize("bad", [1.0, -0.1])
def test_attn_dropout_outside_unit_interval_is_refused(bad):
    from open_musiclm_amd import open_musiclm as M
    with pytest.raises(ValueError):
        M.create_coarse_transformer(dim=128, depth=1, heads=2, attn_dropout=bad, num_coarse_quantizers=3, clap_codebook_size=32,
                                    semantic_codebook_size=32, acoustic_codebook_size=32)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_drops_fraction_p(p):
    keep = R.attn_keep(4, 1024, 3, p, seed=12345, salt=7)          # 1.26e7 draws
    assert abs((1.0 - keep.mean()) - p) < 0.005, keep.mean()
    keep = R.resid_keep(4096, 1024, p, seed=999, salt=3)
    assert abs((1.0 - keep.mean()) - p) < 0.005, keep.mean()


def _agreement(a, b):
    """fraction of equal entries of two 0/1 masks, and what independent masks of the same density would give"""
    pa, pb = a.mean(), b.mean()
    return float((a == b).mean()), float(pa * pb + (1 - pa) * (1 - pb))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_masks_of_neighbours_are_independent(p):
    base = R.attn_keep(2, 512, 2, p, seed=42, salt=5)
    pairs = {
        "i": (base[:, :, 1:, :], base[:, :, :-1, :]),
        "j": (base[..., 1:], base[..., :-1]),
        "h": (base[:, 1:], base[:, :-1]),
        "b": (base[1:], base[:-1]),
        "salt": (base, R.attn_keep(2, 512, 2, p, seed=42, salt=6)),
        "seed": (base, R.attn_keep(2, 512, 2, p, seed=43, salt=5)),
        "j_pair": (base[..., 0::2], base[..., 1::2]),                # the two halves of one hash word
    }
    for name, (a, b) in pairs.items():
        got, chance = _agreement(a, b)
        assert abs(got - chance) < 0.004, (name, got, chance)
    r = R.resid_keep(2048, 512, p, seed=77, salt=5)
    for name, (a, b) in {"row": (r[1:], r[:-1]), "col": (r[:, 1:], r[:, :-1]),
                         "salt": (r, R.resid_keep(2048, 512, p, seed=77, salt=6))}.items():
        got, chance = _agreement(a, b)
        assert abs(got - chance) < 0.004, (name, got, chance)


def test_keep_mask_depends_on_coordinates_only():
    """a sub-block computed with offset coordinates equals the same block of a larger mask (no dependence on N or tiling)"""
    big = R.attn_keep(3, 200, 4, 0.3, seed=5, salt=9)
    part = R.attn_keep(1, 60, 2, 0.3, seed=5, salt=9, b0=2, h0=1, i0=100, j0=100)
    assert np.array_equal(big[2:3, 1:3, 100:160, 100:160], part)


def _tiny(attn_dropout, ff_dropout=0.1):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_coarse_transformer(dim=128, depth=3, heads=2, attn_dropout=attn_dropout, ff_dropout=ff_dropout,
                                       num_coarse_quantizers=3, clap_codebook_size=32, semantic_codebook_size=32,
                                       acoustic_codebook_size=32)


def test_dropout_state_ff_seeds_are_the_ones_drawn_before_attention_dropout():
    from open_musiclm_amd import engine
    tr = _tiny(0.1).transformer
    torch.manual_seed(1234)
    st = engine.dropout_state(tr)
    # the FF seeds as the generator has always drawn them: the first L draws of the rank-mixed generator
    g = torch.Generator().manual_seed((int(torch.initial_seed()) + 0) & 0x7FFFFFFF)
    ff = [int(v) for v in torch.randint(1, 2 ** 62, (3,), generator=g)]
    assert st["ff"] == ff
    a = [int(v) for v in torch.randint(1, 2 ** 62, (6,), generator=g)]
    assert st["attn"] == a[:3] and st["out"] == a[3:]
    assert st["salt"] is None
    assert len(set(st["ff"] + st["attn"] + st["out"])) == 9
