"""CPU: decode under the training key mask (generate(mask_conditioning=True)) -- the rule stated once (open_musiclm.live_conditioning) against
_prepare and the oracle, the null twin's rule, the refusals that come before any device work, the masked plan of csrc/decode_plan.h against
the unmasked one over test_decode_plan_host's calls, and the declaration of omlm_decode_step_masked beside an unchanged argument block."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import test_decode_plan_host as P
from test_decode_plan_host import plan  # noqa: F401  (the fixture: the header behind its test ABI, built by the host c++)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = -1


def _tiny(**kw):
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    base = dict(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                acoustic_codebook_size=16, num_clap_quantizers=3, ff_dropout=0.0)
    base.update(kw)
    return M.create_coarse_transformer(**base)


def _ids(seed, B=3, pads=True, runs=False):
    """[clap [B, 2, 3], semantic [B, 9], coarse [B, 3, 2]]; pads: pad_id entries in the semantic ids; runs: repeated ids (unique_consecutive
    then shortens the rows and pads them itself)"""
    g = torch.Generator().manual_seed(seed)
    clap, sem, coarse = torch.randint(0, 16, (B, 2, 3), generator=g), torch.randint(0, 16, (B, 9), generator=g), torch.randint(0, 16, (B, 3, 2), generator=g)
    if runs:
        sem = torch.randint(0, 3, (B, 9), generator=g)
    if pads:
        sem = sem.masked_fill(torch.rand(B, 9, generator=g) < 0.3, PAD)
    return [clap, sem, coarse]


# ---- 1. the rule, stated once --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("pads", [False, True])
def test_helper_equals_prepare_and_the_oracle(seed, pads):
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.utils import append_eos_id
    from oracle import musiclm_oracle as O
    model = _tiny()
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=0.0).eval()
    ids = _ids(seed, pads=pads)
    B = ids[0].shape[0]
    p_ids, _, p_mask = wrapper._prepare(ids, False, False)
    spec = O.ModelSpec([O.SeqInfo(16, 3), O.SeqInfo(16, 1), O.SeqInfo(16, 2)], dim=64, depth=1, heads=1)
    o_ids, _, o_mask = O.build_training_inputs(ids, spec)
    # (the oracle's ids are those of return_loss=True: its predicted sequence has lost its last id; the conditioning is the same)
    cond = [append_eos_id(t.reshape(B, -1).long(), e) for t, e in zip(ids[:-1], wrapper.eos_ids)]
    h_ids, h_mask = M.live_conditioning(cond, wrapper.eos_ids, PAD, B, torch.device("cpu"))
    n_cond = sum(t.shape[-1] + 1 for t in cond)
    assert h_mask.dtype == torch.bool and h_mask.shape == (B, n_cond)
    for a, b, c in zip(h_ids, p_ids, o_ids):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(h_mask, p_mask[:, :n_cond]) and torch.equal(h_mask, o_mask[:, :n_cond])
    assert bool(p_mask[:, n_cond:].all()) and p_mask.shape[1] == n_cond + 1 + 7       # start token + 6 ids + the appended eos
    # the eos positions and the pads are the non-live ones, start tokens live
    assert bool(h_mask[:, 0].all()) and bool(h_mask[:, 8].all()) and not bool(h_mask[:, 7].any()) and not bool(h_mask[:, -1].any())
    assert torch.equal(~h_mask[:, 9:18], ids[1] == PAD)
    # what generate() builds from its own conditioning rows is the same thing
    c2, t2, (m2, tm2) = wrapper._masked_condition_rows(*wrapper._condition_rows(ids[:-1], True, False), True)
    assert t2 is None and tm2 is None and torch.equal(m2, h_mask) and all(torch.equal(a, b) for a, b in zip(c2, h_ids))
    assert torch.equal(wrapper._rows_mask(m2, 6), F.pad(h_mask, (0, 7), value=True))


def test_helper_on_unique_consecutive_rows_and_input_has_eos():
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.utils import append_eos_id, batch_unique_consecutive
    model = M.TokenConditionedTransformer(token_sequences=[M.TokenSequenceInfo(16, 3, False), M.TokenSequenceInfo(16, 1, True),
                                                           M.TokenSequenceInfo(16, 2, False)], dim=64, depth=1, heads=1, ff_dropout=0.0)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=True, mask_prob=0.0).eval()
    ids = _ids(4, pads=False, runs=True)
    B = ids[0].shape[0]
    p_ids, _, p_mask = wrapper._prepare(ids, False, False)
    # _prepare appends the eos and THEN collapses; generate() collapses and then appends: the rule is applied to what each of them feeds
    cond = [append_eos_id(ids[0].reshape(B, -1).long(), 16), batch_unique_consecutive(append_eos_id(ids[1].long(), 16), pad_value=PAD)]
    assert bool((cond[1] == PAD).any()), "the runs were meant to leave pads behind"
    h_ids, h_mask = M.live_conditioning(cond, wrapper.eos_ids, PAD, B, torch.device("cpu"))
    n_cond = h_mask.shape[1]
    assert all(torch.equal(a, b) for a, b in zip(h_ids, p_ids)) and torch.equal(h_mask, p_mask[:, :n_cond])
    assert torch.equal(~h_mask[:, 9:], (cond[1] == PAD) | (cond[1] == 16))
    g_cond, _ = wrapper._condition_rows(ids[:-1], True, False)
    c2, _, (m2, _) = wrapper._masked_condition_rows(g_cond, None, True)
    assert torch.equal(~m2[:, 9:], (g_cond[1] == PAD) | (g_cond[1] == 16)) and bool((c2[1][~m2[:, 9:]] == 0).all())
    # input_has_eos: the rule applies to whatever ids are given (append_eos_to_conditioning_tokens=False)
    given = [append_eos_id(ids[0].reshape(B, -1).long(), 16), torch.tensor([[3, 16, PAD, 5]] * B)]
    wrapper.unique_consecutive = False
    q_ids, _, q_mask = wrapper._prepare(given + [ids[2]], False, True)
    c3, _, (m3, _) = wrapper._masked_condition_rows(*wrapper._condition_rows(given, False, False), False)
    assert all(torch.equal(a, b) for a, b in zip(c3, q_ids)) and torch.equal(m3, q_mask[:, :m3.shape[1]])
    assert m3[:, 8:].tolist() == [[True, True, False, False, True]] * B and c3[1].tolist() == [[3, 0, 0, 5]] * B


def test_prepare_is_what_it_was():
    """_prepare's ids, labels and mask against the loop it used to hold, in training mode with the forgetful mask and the condition drop."""
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.utils import append_eos_id, generate_mask_with_prob
    model = _tiny()
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=0.15, null_cond_prob=0.5).train()
    ids = _ids(7)
    B = ids[0].shape[0]
    torch.manual_seed(17)
    got_ids, got_labels, got_mask = wrapper._prepare(ids, True, False)
    torch.manual_seed(17)
    want = [append_eos_id(t.reshape(B, -1).long(), e) for t, e in zip(ids, wrapper.eos_ids)]
    labels = [t.clone() for t in want]
    want[-1] = want[-1][:, :-1]
    pieces = []
    for i in range(2):
        live = (want[i] != PAD) & (want[i] != wrapper.eos_ids[i])
        want[i] = want[i].masked_fill(~live, 0)
        pieces.append(F.pad(live, (1, 0), value=True))
    mask = F.pad(torch.cat(pieces, dim=-1), (0, want[-1].shape[-1] + 1), value=True)
    forget = generate_mask_with_prob(mask.shape, 0.15, device=mask.device)
    dropped = torch.rand(B) < 0.5
    want[0] = torch.where(dropped[:, None] & (torch.arange(7) < 6)[None], M.null_twin(want[0], wrapper.token_sequences[0], 6), want[0])
    mask[:, 1:7] |= dropped[:, None]
    mask = mask & forget
    assert all(torch.equal(a, b) for a, b in zip(got_ids, want)) and all(torch.equal(a, b) for a, b in zip(got_labels, labels))
    assert torch.equal(got_mask, mask) and bool(dropped.any()) and not bool(mask.all())


# ---- 2. the null twin under the mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("append_eos", [True, False])
def test_twin_takes_the_prompts_mask_with_the_condition_attended(append_eos):
    from open_musiclm_amd import open_musiclm as M
    model = _tiny()
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False).eval()
    ids = _ids(5)
    ids[0][0, 0, 1] = PAD                                      # a pad INSIDE the condition: masked in the prompt, attended in the twin
    B, n0 = 3, 6
    cond, twin = wrapper._condition_rows(ids[:-1], append_eos, True)
    c, t, (m, tm) = wrapper._masked_condition_rows(cond, twin, append_eos)
    info = wrapper.token_sequences[0]
    assert not bool(m[0, 2]) and int(c[0][0, 1]) == 0
    # the training rule of a dropped sample: mask[:, 1:1 + n0] |= dropped, the null ids at those positions, everything else the prompt's
    want_mask = m.clone()
    want_mask[:, 1:1 + n0] = True
    assert torch.equal(tm, want_mask) and bool(tm[:, 1:1 + n0].all()) and torch.equal(tm[:, 1 + n0:], m[:, 1 + n0:])
    assert torch.equal(t[0][:, :n0], M.null_condition_ids(info, n0).expand(B, n0))
    assert torch.equal(t[0][:, n0:], c[0][:, n0:]) and torch.equal(t[1], c[1])
    if append_eos:
        assert c[0].shape[1] == n0 + 1 and bool((t[0][:, n0] == 0).all()) and not bool(tm[:, 1 + n0].any())      # the eos: zeroed, no key
    # against _prepare with every sample dropped
    tr = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=0.0, null_cond_prob=1.0).train()
    if append_eos:
        p_ids, _, p_mask = tr._prepare(ids, False, False)
        assert torch.equal(p_ids[0], t[0]) and torch.equal(p_ids[1], t[1]) and torch.equal(p_mask[:, :tm.shape[1]], tm)


# ---- 3. refusals before any device work -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [None, 1, 0, "yes", 1.0])
def test_a_non_bool_is_refused_before_any_device_work(bad):
    """A CPU model: the next thing a valid call on it meets is hip.require_gpu."""
    from open_musiclm_amd import open_musiclm as M
    model = _tiny(precision="fp16")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    ids = _ids(0, B=2, pads=False)
    with pytest.raises(ValueError, match="mask_conditioning must be a bool"):
        wrapper.generate(conditioning_token_ids=ids[:-1], max_time_steps=2, mask_conditioning=bad)
    with pytest.raises(ValueError, match="mask_conditioning must be a bool"):
        wrapper.score(conditioning_token_ids=ids[:-1], pred_token_ids=ids[2], mask_conditioning=bad)
    # a bool passes the check and reaches the device requirement
    for value in (True, False):
        with pytest.raises(Exception) as e:
            wrapper.score(conditioning_token_ids=ids[:-1], pred_token_ids=ids[2], mask_conditioning=value)
        assert "mask_conditioning" not in str(e.value)


def test_the_defaults_are_off(monkeypatch):
    """A call without the argument never builds a mask (the call dies at the device requirement either way: a CPU model)."""
    from open_musiclm_amd import decode, open_musiclm as M
    model = _tiny(precision="fp16")
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    ids = _ids(0, B=2, pads=False)
    built, orig = [], wrapper._masked_condition_rows
    monkeypatch.setattr(wrapper, "_masked_condition_rows", lambda *a: (built.append(1), orig(*a))[1])
    for kw, want in (({}, 0), (dict(mask_conditioning=False), 0), (dict(mask_conditioning=True), 1)):
        built.clear()
        with pytest.raises(RuntimeError, match="is on cpu"):          # generate() builds its rows, then asks for the device
            wrapper.generate(conditioning_token_ids=ids[:-1], max_time_steps=2, **kw)
        assert len(built) == want, kw
        with pytest.raises(RuntimeError, match="is on cpu"):          # (score() asks for the device first)
            wrapper.score(conditioning_token_ids=ids[:-1], pred_token_ids=ids[2], **kw)
    assert M.stage_mask_conditioning(None) == (None, None, None)
    assert inspect.signature(decode.CachedDecoder.__init__).parameters["key_mask"].default is False
    assert inspect.signature(decode.CachedDecoder.prefill).parameters["key_mask"].default is None
    assert inspect.signature(M.TokenConditionedTransformer.last_logits).parameters["self_attn_mask"].default is None


def test_a_model_without_conditioning_refuses_the_flag_by_name():
    """A single token sequence: nothing to mask.  Refused before any device work; False is the call it has always been."""
    from open_musiclm_amd import open_musiclm as M
    model = M.TokenConditionedTransformer(token_sequences=[M.TokenSequenceInfo(16, 2, False)], dim=64, depth=1, heads=1, ff_dropout=0.0)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False)
    pred = torch.randint(0, 16, (2, 3, 2))
    with pytest.raises(ValueError, match="mask_conditioning: .*single token sequence"):
        wrapper.generate(conditioning_token_ids=[], pred_token_ids=pred, max_time_steps=4, mask_conditioning=True)
    with pytest.raises(ValueError, match="mask_conditioning: .*single token sequence"):
        wrapper.score(conditioning_token_ids=[], pred_token_ids=pred, mask_conditioning=True)
    with pytest.raises(Exception) as e:
        wrapper.score(conditioning_token_ids=[], pred_token_ids=pred, mask_conditioning=False)
    assert "mask_conditioning" not in str(e.value)


def _musiclm():
    from open_musiclm_amd import open_musiclm as M
    kw = dict(dim=64, depth=1, heads=1, precision="fp16")
    return M.MusicLM(semantic_transformer=M.create_semantic_transformer(**kw), coarse_transformer=M.create_coarse_transformer(**kw),
                     fine_transformer=M.create_fine_transformer(**kw))


@pytest.mark.parametrize("bad", [{"semantic": 1}, {"coarse": "on"}, {"decoder": True}, 1, "all"])
def test_musiclm_forward_refuses_a_bad_mapping_before_any_stage_runs(bad):
    mlm = _musiclm()
    called = []
    mlm.semantic.generate = lambda **k: called.append(k)
    with pytest.raises(ValueError, match="mask_conditioning"):
        mlm(clap_token_ids=torch.zeros(1, 12, 1, dtype=torch.long), mask_conditioning=bad, return_tokens=True)
    assert not called


def test_musiclm_forward_hands_each_stage_its_value():
    from open_musiclm_amd import open_musiclm as M
    assert M.stage_mask_conditioning(None) == (None, None, None) and M.stage_mask_conditioning(True) == (True, True, True)
    assert M.stage_mask_conditioning({"coarse": True, "fine": False}) == (None, True, False)
    mlm = _musiclm()
    seen = {}

    class Stop(Exception):
        pass

    def sem(**k):
        seen.update(k)
        raise Stop
    mlm.semantic.generate = sem
    for value, want in ((None, "absent"), ({"coarse": True}, "absent"), (True, True), ({"semantic": False}, False)):
        seen.clear()
        with pytest.raises(Stop):
            mlm(clap_token_ids=torch.zeros(1, 12, 1, dtype=torch.long), mask_conditioning=value, return_tokens=True)
        assert seen.get("mask_conditioning", "absent") == want, value        # (a keyword at its default is not passed)


# ---- 4. the masked plan ----------------------------------------------------------------------------------------------------------------
KERNELS = P.KERNELS + ("attn1_masked", "attn2_masked")
UNMASKED = {"attn1_masked": "attn1", "attn2_masked": "attn2"}


def _run(lib, c, masked, key_live=True):
    out, msg = (C.c_longlong * (16 + 16 * 11))(), C.create_string_buffer(320)
    if masked:
        lib.omlm_plan_decode_masked(c, int(key_live), out, msg)
    else:
        lib.omlm_plan_decode(c, out, msg)
    head = list(out[:16])
    n = head[P.HEAD.index("n")]
    ls = [dict(zip(P.LAUNCH, out[16 + 16 * i:32 + 16 * i])) for i in range(n + 1)]
    for l in ls:
        l["kernel"] = KERNELS[l["kernel"]]
    return head, ls, msg.value.decode()


def _calls():
    """the calls of test_decode_plan_host: every recorded row, and its grids of served and refused calls"""
    for row in P.ROWS:
        if row["null"] != "args":
            yield P.call_of(row)
    for B, D, H, Fp, w16, scratch, lo in itertools.product((1, 2, 8, 9, 16, 17, 64), P.DS, P.HS, P.FPS, (0, 1), (False, True), (False, True)):
        yield P.call(B, D, H, Fp, w16, pos_dev=True, parts=True, head_W=True, ln_parts=scratch, splitk_ws=scratch, splitk_cnt=scratch,
                     W1p_lo=lo, W2p_lo=lo, head_W_lo=lo)
    for B, D, H, Fp, w16, kv16 in itertools.product((1, 3, 16, 17, 64, 65), (128, 1024), (2, 8), (256, 2752, 4096), (0, 1), (False, True)):
        yield P.call(B, D, H, Fp, w16, L=6, Nmax=197, nsplit=4, V1=1025, kv16=kv16, pos_dev=True, parts=True, ids=True, emb_table=True, head_W=True,
                     ln_parts=True, splitk_ws=True, splitk_cnt=True, k_new=kv16, advance_pos=True)


def test_masked_plan_is_the_unmasked_plan_with_the_masked_attention_kernels(plan):  # noqa: F811
    served = refused = attn = 0
    routes = set()
    for c in _calls():
        h0, l0, m0 = _run(plan, c, False)
        h1, l1, m1 = _run(plan, c, True)
        assert h1 == h0 and m1 == m0, (list(c), m0, m1)            # route, groups, regions, flags, counts -- and every refusal, word for word
        assert not any(l["kernel"] in UNMASKED for l in l0)
        if h0[0] != 0:
            refused += 1
            assert h0[P.HEAD.index("n")] == 0
            continue
        served += 1
        routes.add(P.ROUTES[h0[1]])
        assert len(l0) == len(l1)
        for a, b in zip(l0[:-1], l1[:-1]):
            if a["kernel"] in ("attn1", "attn2"):
                assert b["kernel"] == a["kernel"] + "_masked" and P.PHASES[b["phase"]] == "attn"
                attn += 1
            assert dict(b, kernel=UNMASKED.get(b["kernel"], b["kernel"])) == a          # grids, workgroup, LDS bytes, every scalar
        assert l1[-1] == l0[-1]                                                          # q_rest: no attention launch
        assert (c[3] > 0) == any(l["kernel"] in UNMASKED for l in l1)
    assert served > 1000 and refused > 1000 and attn > 1000 and routes == set(P.ROUTES), (served, refused, attn, routes)


def test_masked_plan_refuses_a_null_key_live_and_nothing_else_new(plan):  # noqa: F811
    ok = P.call(3, 1024, 8, 2752, 1, L=6, Nmax=197, nsplit=4, V1=1025, pos_dev=True, parts=True, ids=True, emb_table=True, head_W=True,
                ln_parts=True, splitk_ws=True, splitk_cnt=True, advance_pos=True)
    h, ls, msg = _run(plan, ok, True, key_live=False)
    assert (h[0], msg, h[P.HEAD.index("n")]) == (P.ERR_ARG, "bad argument: null key_live [key_live]", 0)
    assert _run(plan, ok, True)[0][0] == 0 and _run(plan, ok, False)[0][0] == 0
    # an earlier refusal keeps its own text with key_live missing as well
    bad = P.call(3, 1024, 8, 2752, 1, L=6, Nmax=197, nsplit=3, V1=1025, pos_dev=True, parts=True)
    assert _run(plan, bad, True, key_live=False)[2] == _run(plan, bad, False)[2] != ""
    assert "nsplit must cover Nmax keys" in _run(plan, bad, False)[2]


# ---- 5. the C interface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_masked_entry_beside_an_unchanged_argument_block(tmp_path):
    from open_musiclm_amd import decode, hip
    text = open(os.path.join(ROOT, "include", "omlm.h")).read()
    assert re.search(r"int\s+omlm_decode_step_masked\(const omlm_decode_args\*\s*args,\s*const unsigned char\*\s*key_live,\s*"
                     r"const long long\*\s*ids,\s*void\*\s*stream\);", text)
    assert re.search(r"int\s+omlm_decode_step\(const omlm_decode_args\*\s*args,\s*const long long\*\s*ids,\s*void\*\s*stream\);", text)
    for word in ("key_live", "[B, Nmax]", "-3.0e38f", "must be 1"):
        assert word in text[text.index("omlm_decode_step under a key mask"):text.index("int omlm_decode_step_masked")], word
    # the mask is an argument of the call, not a member: the struct and its mirror are what they were
    names = [f[0] for f in decode.DecodeArgs._fields_]
    assert names[-2:] == ["kv16", "k_new"] and "key_live" not in names and len(names) == 52
    body = text[text.index("typedef struct omlm_decode_args {"):text.index("} omlm_decode_args;")]
    assert "key_live" not in body
    fields = names
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "omlm.h")}"', "int main(void) {",
             '  printf("%zu\\n", sizeof(omlm_decode_args));']
    lines += [f'  printf("%zu\\n", offsetof(omlm_decode_args, {f}));' for f in fields] + ["  return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(decode.DecodeArgs) and out[1:] == [getattr(decode.DecodeArgs, f).offset for f in fields]
    assert len(hip.SIGNATURES["omlm_decode_step_masked"]) == 4 and len(hip.SIGNATURES["omlm_decode_step"]) == 3
