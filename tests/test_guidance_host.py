"""CPU: classifier-free guidance on the condition -- the restatement (tests/guidance_ref.py) against plain loops and against the oracle,
the refusals that come before any device work, the declarations of the two new entry points, and the defaults that keep today's runs
what they are."""
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import guidance_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(**kw):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    base = dict(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                acoustic_codebook_size=16, num_clap_quantizers=3, ff_dropout=0.0)
    base.update(kw)
    return M.create_coarse_transformer(**base)


def _single():
    from open_musiclm_amd import open_musiclm as M
    return M.TokenConditionedTransformer(token_sequences=[M.TokenSequenceInfo(16, 2, False)], dim=64, depth=1, heads=1, ff_dropout=0.0)


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_guide_rule_is_three_float32_roundings_in_the_stated_order():
    g = torch.Generator().manual_seed(1)
    l, n = (torch.randn(5, 37, generator=g) * 7).numpy(), (torch.randn(5, 37, generator=g) * 7).numpy()
    for s in (0.0, 0.5, 3.0, 1.0, 7.25):
        got = G.guide(l, n, s)
        assert got.dtype == np.float32
        for r in range(5):
            for c in range(37):
                d = _f32(float(l[r, c]) - float(n[r, c]))          # a double difference of two floats rounds once to float32
                m = _f32(_f32(s) * d)
                assert got[r, c] == _f32(float(n[r, c]) + m), (s, r, c)
    assert np.array_equal(G.guide(l, n, 0.0), n)                    # s = 0: the null row, bit for bit
    assert not np.array_equal(G.guide(l, n, 1.0), l)                # s = 1 is NOT the conditional row bit for bit: callers do not launch
    assert np.abs(G.guide(l, n, 1.0) - l).max() < 1e-5
    # the combination itself, against fp64
    want = G.guide64(torch.from_numpy(l), torch.from_numpy(n), 3.0)
    assert float((torch.from_numpy(G.guide(l, n, 3.0)).double() - want).abs().max()) < 1e-4
    assert G.factor(3) == 5 and G.factor(0.5) == 1 and G.factor(0) == 1


def test_null_raw_ids_are_minus_one_after_the_offset():
    from open_musiclm_amd import open_musiclm as M
    for cb, Q, n in ((16, 3, 7), (1024, 12, 24), (8, 1, 5)):
        raw = G.null_raw_ids(cb, Q, n)
        off = cb * (torch.arange(n) % Q) if Q > 1 else torch.zeros(n, dtype=torch.long)
        assert torch.equal(raw + off, torch.full((n,), -1))
        assert torch.equal(M.null_condition_ids(M.TokenSequenceInfo(cb, Q, False), n), raw)
    x = torch.arange(10).reshape(2, 5)
    tw = G.null_twin(x, 16, 3, 4)
    assert tw[:, 4].tolist() == [4, 9] and torch.equal(tw[:, :4], G.null_raw_ids(16, 3, 4).expand(2, 4))
    assert torch.equal(M.null_twin(x, M.TokenSequenceInfo(16, 3, False), 4), tw)


def test_oracle_on_the_null_raw_ids_equals_a_zeroed_clap_table():
    """Pins 'null = zero rows' to the oracle: its unmodified forward on the null raw ids is its forward with embeddings.0 zeroed."""
    from oracle import musiclm_oracle as O
    spec = O.ModelSpec([O.SeqInfo(16, 3), O.SeqInfo(16, 1), O.SeqInfo(16, 2)], dim=64, depth=2, heads=2)
    sd = O.init_state_dict(spec, seed=2)
    ids = O.synthetic_ids(spec, 2, [2, 5, 3], seed=5)
    B = 2
    pred = ids[2].reshape(B, -1)
    zeroed = dict(sd)
    zeroed["embeddings.0.weight"] = torch.zeros_like(sd["embeddings.0.weight"])
    # the bare condition (no eos appended): every position of sequence 0 is an id position, so the whole table may be zeroed
    bare = [ids[0].reshape(B, -1).long(), ids[1].reshape(B, -1).long()]
    got = O.token_conditioned_forward(sd, spec, [G.null_twin(bare[0], 16, 3, bare[0].shape[1]), bare[1], pred])
    want = O.token_conditioned_forward(zeroed, spec, bare + [pred])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(O.token_conditioned_forward(sd, spec, bare + [pred])[-1], got[-1])       # the condition matters
    # generate's conditioning (eos appended): the eos keeps its own row, so its embedding is that of the unmodified call; the id positions
    # are zero rows
    cond0 = O.append_eos(bare[0], spec.eos_ids[0])
    twin = G.null_twin(cond0, 16, 3, bare[0].shape[1])
    x_twin, _ = O.embed_sequences(sd, [twin, bare[1], pred], spec)
    x_cond, _ = O.embed_sequences(sd, [cond0, bare[1], pred], spec)
    n = bare[0].shape[1]
    assert float(x_twin[:, 1:1 + n].abs().max()) == 0.0 and float(x_cond[:, 1:1 + n].abs().min()) > 0.0
    assert torch.equal(x_twin[:, 1 + n:], x_cond[:, 1 + n:]) and torch.equal(x_twin[:, 0], x_cond[:, 0])


def test_oracle_training_inputs_key_mask_a_raw_minus_one():
    """Why the GPU training test composes the oracle's pieces instead of calling wrapper_forward_loss on the null raw ids: the oracle's
    build_training_inputs (the reference's rule, open_musiclm.py:359-366) treats a RAW id of -1 -- the null raw id wherever p mod Q == 0 --
    as padding: it key-masks the position and embeds id 0.  The drop rule keeps every condition position attended, so the oracle value
    it is compared with takes the key mask of the real ids and the null raw ids as ids (both forms differ by ~3e-4 of the loss on the
    tiny model, between the fp16 / bf16x3 loss bars and bf16's)."""
    from oracle import musiclm_oracle as O
    spec = O.ModelSpec([O.SeqInfo(16, 3), O.SeqInfo(16, 1), O.SeqInfo(16, 2)], dim=64, depth=2, heads=2)
    ids = O.synthetic_ids(spec, 2, [2, 5, 3], seed=5)
    null0 = G.null_raw_ids(16, 3, 6).expand(2, 6)
    _, _, mask = O.build_training_inputs([null0] + list(ids[1:]), spec)
    assert mask[:, 1:7].tolist() == [[False, True, True, False, True, True]] * 2
    _, _, real = O.build_training_inputs(ids, spec)
    assert bool(real[:, 1:7].all())


def test_drop_rule_on_prepare_outputs(monkeypatch):
    """_prepare with null_cond_prob against apply_drop on the outputs of _prepare without it: same forgetful mask, u injected."""
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    model = _tiny()
    B, p = 4, _f32(0.3)
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(0, 16, (B, 2, 3), generator=g), torch.randint(0, 16, (B, 5), generator=g), torch.randint(0, 16, (B, 3, 2), generator=g)]
    ids[0][0, 0, 1] = -1                                             # a pad among the condition ids of a sample that is dropped
    u = torch.tensor([0.0, float(np.nextafter(np.float32(p), np.float32(0))), p, 0.99])
    noise = torch.randn(B, 7 + 1 + 6 + 1 + 6 + 1, generator=g)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: u.clone())
    for mask_prob in (0.0, 0.25):
        monkeypatch.setattr(M, "generate_mask_with_prob", lambda shape, pr, device: O.forgetful_mask_from_noise(noise, pr))
        plain = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=mask_prob).train()
        drop = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=mask_prob, null_cond_prob=p).train()
        i0, l0, m0 = plain._prepare(ids, True, False)
        i1, l1, m1 = drop._prepare(ids, True, False)
        forget = O.forgetful_mask_from_noise(noise, mask_prob) if mask_prob > 0 else None
        want_ids, want_mask, dropped = G.apply_drop(i0[0], m0, forget, u, p, 16, 3, 6)
        assert dropped.tolist() == [True, True, False, False]        # the boundary is <
        assert torch.equal(i1[0], want_ids) and torch.equal(m1, want_mask)
        assert all(torch.equal(a, b) for a, b in zip(i1[1:], i0[1:])) and all(torch.equal(a, b) for a, b in zip(l1, l0))
        assert torch.equal(i1[0][:, 6], i0[0][:, 6])                 # the appended eos position (masked to 0 by the reference rule) is untouched
        if mask_prob == 0.0:                                         # a padded condition id (key mask 0 without the drop) is attended too
            assert not bool(m0[0, 1:7].all()) and bool(m1[:2, 1:7].all())
        # eval never drops
        e = drop.eval()._prepare(ids, True, False)
        pe = plain.eval()._prepare(ids, True, False)
        assert torch.equal(e[0][0], pe[0][0]) and torch.equal(e[2], pe[2])


def test_no_draw_at_probability_zero(monkeypatch):
    from open_musiclm_amd import open_musiclm as M
    model = _tiny()
    w = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=0.15).train()
    assert w.null_cond_prob == 0.0
    ids = [torch.zeros(2, 1, 3, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 2, 2, dtype=torch.long)]

    def boom(*a, **k):
        raise AssertionError("torch.rand must not be called with null_cond_prob == 0")
    torch.manual_seed(5)
    want = w._prepare(ids, True, False)[2]
    state = torch.get_rng_state()
    monkeypatch.setattr(torch, "rand", boom)
    torch.manual_seed(5)
    got = w._prepare(ids, True, False)[2]
    assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)


# ---- refusals before device work -------------------------------------------------------------------------------------------------------
BAD_SCALES = [-1, float("nan"), float("inf"), "3", -0.0001, 1e39, True]


@pytest.mark.parametrize("bad", BAD_SCALES)
def test_bad_cond_scale_is_refused_by_name(bad):
    from open_musiclm_amd import decode, ops
    from open_musiclm_amd import open_musiclm as M
    w = M.TokenConditionedTransformerWrapper(transformer=_tiny(), unique_consecutive=False)
    cond = [torch.zeros(1, 1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long)]
    with pytest.raises(ValueError, match="cond_scale"):
        w.generate(conditioning_token_ids=cond, max_time_steps=1, cond_scale=bad)
    with pytest.raises(ValueError, match="cond_scale"):
        w.score(conditioning_token_ids=cond, pred_token_ids=torch.zeros(1, 1, 2, dtype=torch.long), cond_scale=bad)
    with pytest.raises(ValueError, match="cond_scale"):
        M.stage_cond_scale(bad)
    with pytest.raises(ValueError, match=r"cond_scale\['coarse'\]"):
        M.stage_cond_scale({"coarse": bad})
    with pytest.raises(ValueError, match="scale"):
        ops.check_cond_scale(bad, "scale")
    assert "guidance" in inspect.signature(decode.SamplingLoop.__init__).parameters


def test_valid_cond_scale_meets_the_gpu_requirement_next():
    from open_musiclm_amd import ops
    from open_musiclm_amd import open_musiclm as M
    w = M.TokenConditionedTransformerWrapper(transformer=_tiny(), unique_consecutive=False)
    cond = [torch.zeros(1, 1, 3, dtype=torch.long), torch.zeros(1, 3, dtype=torch.long)]
    for s in (0, 0.5, 3, 3.0, np.float32(2.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            w.generate(conditioning_token_ids=cond, max_time_steps=1, cond_scale=s)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            w.generate(conditioning_token_ids=cond, max_time_steps=1, cond_scale=s, use_cache=False)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            w.score(conditioning_token_ids=cond, pred_token_ids=torch.zeros(1, 1, 2, dtype=torch.long), cond_scale=s)
    assert ops.check_cond_scale(None) is None and ops.check_cond_scale(1) is None and ops.check_cond_scale(1.0) is None      # off
    assert ops.check_cond_scale(0) == 0.0 and ops.check_cond_scale(3) == 3.0


@pytest.mark.parametrize("bad", [-0.1, 1.0001, float("nan"), "0.1", None, 2])
def test_bad_null_cond_prob_is_refused_by_name(bad):
    from open_musiclm_amd import open_musiclm as M
    model = _tiny()
    with pytest.raises(ValueError, match="null_cond_prob"):
        M.TokenConditionedTransformerWrapper(transformer=model, null_cond_prob=bad)
    with pytest.raises(ValueError, match="null_cond_prob"):
        M.CoarseStage(coarse_transformer=model, null_cond_prob=bad)


def test_valid_null_cond_prob_travels_through_stages_trainer_and_config():
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.config import SingleStageTrainerConfig
    from open_musiclm_amd.trainer import SingleStageTrainer
    model = _tiny()
    for p in (0, 0.15, 0.999, 1.0):
        assert M.TokenConditionedTransformerWrapper(transformer=model, null_cond_prob=p).null_cond_prob == float(p)
    assert M.CoarseStage(coarse_transformer=model, null_cond_prob=0.2).transformer_wrapper.null_cond_prob == 0.2
    assert M.FineStage(fine_transformer=model, null_cond_prob=0.2).transformer_wrapper.null_cond_prob == 0.2
    sem = M.create_semantic_transformer(dim=64, depth=1, heads=1, clap_codebook_size=16, semantic_codebook_size=16, num_clap_quantizers=3)
    assert M.SemanticStage(semantic_transformer=sem, null_cond_prob=0.2).transformer_wrapper.null_cond_prob == 0.2
    assert M.CoarseStage(coarse_transformer=model).transformer_wrapper.null_cond_prob == 0.0
    fields = SingleStageTrainerConfig.__dataclass_fields__
    assert fields["null_cond_prob"].default == 0.0
    assert inspect.signature(SingleStageTrainer.__init__).parameters["null_cond_prob"].default == 0.0
    src = inspect.getsource(SingleStageTrainer)
    assert "self._make_stage(transformer, null_cond_prob)" in src and "self._make_stage(self._ema_twin).eval()" in src      # the twin never drops


def test_single_sequence_model_refuses_guidance_and_drop_by_name():
    from open_musiclm_amd import open_musiclm as M
    model = _single()
    with pytest.raises(ValueError, match="null_cond_prob.*single token sequence"):
        M.TokenConditionedTransformerWrapper(transformer=model, null_cond_prob=0.1)
    w = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    with pytest.raises(ValueError, match="cond_scale.*single token sequence"):
        w.generate(conditioning_token_ids=[], max_time_steps=1, cond_scale=3)
    with pytest.raises(ValueError, match="cond_scale.*single token sequence"):
        w.score(conditioning_token_ids=[], pred_token_ids=torch.zeros(1, 1, 2, dtype=torch.long), cond_scale=3)


def test_musiclm_forward_takes_a_number_or_a_stage_mapping():
    from open_musiclm_amd import open_musiclm as M
    assert M.stage_cond_scale(None) == (None, None, None) and M.stage_cond_scale(3) == (3, 3, 3)
    assert M.stage_cond_scale({"coarse": 2.5}) == (None, 2.5, None)
    assert M.stage_cond_scale({"semantic": 3, "coarse": 1, "fine": 0}) == (3, 1, 0)
    with pytest.raises(ValueError, match=r"cond_scale: unknown stage\(s\) \['corase'\]"):
        M.stage_cond_scale({"corase": 3})
    sem = M.create_semantic_transformer(dim=64, depth=1, heads=1, clap_codebook_size=16, semantic_codebook_size=16, num_clap_quantizers=3)
    coarse = _tiny()
    fine = M.create_fine_transformer(dim=64, depth=1, heads=1, clap_codebook_size=16, acoustic_codebook_size=16, num_clap_quantizers=3,
                                     num_coarse_quantizers=2, num_fine_quantizers=2)
    lm = M.MusicLM(semantic_transformer=sem, coarse_transformer=coarse, fine_transformer=fine)
    clap = torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="unknown stage"):
        lm(clap_token_ids=clap, return_tokens=True, cond_scale={"corase": 3})
    with pytest.raises(ValueError, match="cond_scale"):
        lm(clap_token_ids=clap, return_tokens=True, cond_scale=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm(clap_token_ids=clap, return_tokens=True, cond_scale={"coarse": 3}, output_seconds=1)
    assert "cond_scale=None" in inspect.getsource(M.MusicLM)         # (forward is wrapped by decorators)


# ---- declarations ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_with_the_function_beside_them():
    """Fails before the two entries exist."""
    from open_musiclm_amd import hip, ops
    hdr = open(os.path.join(ROOT, "include", "omlm.h")).read()
    src = open(os.path.join(ROOT, "open_musiclm_amd", "csrc", "sampler.hip")).read()
    m = re.search(r"int omlm_guide_logits\(([^)]*)\);", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)) == ("const float* cond, const float* null, float* out, int rows, int V, int ld, float scale, "
                                                      "void* stream")
    assert len(hip.SIGNATURES["omlm_guide_logits"]) == m.group(1).count(",") + 1 == 8
    t = re.search(r"int omlm_decode_twin\(([^)]*)\);", hdr)
    assert t and re.sub(r"\s+", " ", t.group(1)) == ("const long long* ids, long long* ids_twin, const float* x, float* x_twin, int rows, int D, "
                                                      "void* stream")
    assert len(hip.SIGNATURES["omlm_decode_twin"]) == t.group(1).count(",") + 1 == 7
    before = hdr[hdr.index("int omlm_guide_logits(") - 2500:hdr.index("int omlm_guide_logits(")]
    for word in ("g_c = n_c + (s * (l_c - n_c))", "__fadd_rn(n_c, __fmul_rn(s, __fsub_rn(l_c, n_c)))", "three roundings", "log-softmax of g",
                 "-1 - codebook (p mod Q)", "out may alias cond", "are not written"):
        assert word in before, word
    for name in ("omlm_guide_logits", "omlm_decode_twin"):
        assert f'extern "C" int {name}(' in src
    assert "__fadd_rn(n, __fmul_rn(s, __fsub_rn(l, n)))" in src
    p = re.search(r"int omlm_prepare_train_batch\(([^)]*)\);", hdr)
    assert p and re.sub(r"\s+", " ", p.group(1)).endswith("int N, const float* null_u, float null_p, void* stream")
    assert len(hip.SIGNATURES["omlm_prepare_train_batch"]) == p.group(1).count(",") + 1 == 17
    prep = inspect.signature(ops.prepare_train_batch).parameters
    assert [k for k, v in prep.items() if v.kind is v.KEYWORD_ONLY] == ["null_u", "null_p"]
    assert prep["null_u"].default is None and prep["null_p"].default == 0.0
    assert len([v for v in prep.values() if v.kind is v.POSITIONAL_OR_KEYWORD]) == 8
