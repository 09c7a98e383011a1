"""Cached decode under the training key mask (CachedDecoder(key_mask=True), omlm_decode_step_masked, generate(mask_conditioning=True)) on the GPU.

The models, the cases, TOL / relerr / report are test_gpu_decode_kv16's (depth 2; gen1, dec3, dec4, the wide call, dec2; both cache types).

Prompt: 12 CLAP ids and 170 semantic ids, the eos appended -- rows: CLAP start 0, ids 1..12, eos 13; semantic start 14, ids 15..184, eos 185;
predicted start 186: 187 prompt rows, Nmax = 197, 8 teacher-forced steps at pos 187..194.  Semantic positions 45..116 are pad_id (rows
60..131), so key range 1 (rows 64..127) is FULLY masked and ranges 0 and 2 are partly masked; sample b also pads semantic position 3 + b, so
no two samples share a mask; the two eos rows (13, 185) are masked by the rule.  The steps cross row 192: from there a range holds the new
key alone, and for pos 187..191 the new key's range also holds masked keys (rows 128..131 and the eos row 185).

The cases are all eleven of test_gpu_decode_kv16.  The precondition of check 1 -- the masked and the unmasked logits differ by more than
10 x the bar, or an ignored mask could pass -- was checked ahead on the CPU with the fp32 oracle (oracle.token_conditioned_forward, this
prompt at seed 8, the models of the cases in fp32): the smallest relative difference between the masked and the unmasked last-row logits
over the 9 rows is 0.1406 (small, B = 1) and 0.1520 (small, B = 3) against 0.12 = 10 x the bf16 bar, and 0.1170 / 0.0978 / 0.1167 (dim
1024, B = 1 / 3 / 17) and 0.1296 (plain FF, B = 2) against 0.01 = 10 x the fp16 bar and 0.005 = 10 x fp16ff's.  At dim 1024 no seed of 1..9
clears the 0.12 that bf16 needs (0.08 .. 0.12), so the two bf16 cases at dim 1024 (WIDER) also pad semantic positions 117..159 (rows
132..175; range 2 stays partly masked, rows 176..184 live): the oracle then gives 0.1805 (B = 1) and 0.1678 (B = 3).  Everything said
above about the prompt holds for them as well."""
import pytest
import torch
import torch.nn.functional as F

import sampler_logprob_ref as L
from test_gpu_decode_kv16 import CASES, TOL, V1, _assert_route, _model, _spies, dev, relerr, report  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 8                          # of the prompt: chosen so that the fp32 oracle clears the precondition of check 1 (module docstring)
NMAX, PROMPT_ROWS, STEPS = 197, 187, 8
PAD = -1
KM_CASES = list(CASES)
WIDER = {"dec3-bf16-B1": (117, 160), "dec4-bf16-B3": (117, 160)}       # further padded semantic positions [lo, hi) of a case (module docstring)
_RUNS = {}


def _raw_prompt(B, seed=SEED, wider=None):
    g = torch.Generator().manual_seed(seed)
    clap, sem = torch.randint(0, 1024, (B, 12, 1), generator=g), torch.randint(0, 1024, (B, 170), generator=g)
    flat = torch.randint(0, 1024, (B, STEPS + 1), generator=g)
    sem[:, 45:117] = PAD
    if wider is not None:
        sem[:, wider[0]:wider[1]] = PAD
    for b in range(B):
        sem[b, 3 + b] = PAD
    return [clap, sem], flat


def _masked_prompt(wrapper, dev, B, seed=SEED, wider=None):  # noqa: F811
    """(zeroed conditioning rows, conditioning mask [B, 186] bool, the 9 teacher-forced ids) as generate(mask_conditioning=True) builds them"""
    cond, flat = _raw_prompt(B, seed, wider)
    rows, _, (mask, _) = wrapper._masked_condition_rows(*wrapper._condition_rows(cond, True, False), True)
    assert mask.shape == (B, PROMPT_ROWS - 1) and sum(t.shape[-1] + 1 for t in rows) + 1 == PROMPT_ROWS
    live = mask.cpu()
    assert not bool(live[:, 60:132].any()) and not bool(live[:, 13].any()) and not bool(live[:, 185].any()) and bool(live[:, [0, 14]].all())
    assert all(not bool(live[b, 15 + 3 + b]) for b in range(B)) and len({tuple(r.tolist()) for r in live}) == B
    assert int((~live).sum()) == B * (72 + 2 + 1 + (wider[1] - wider[0] if wider else 0))
    return rows, mask, flat.to(dev)


def _steps(model, rows, flat, precision, B, wide, kv_cache, key_mask, mask):
    """prefill + 8 teacher-forced steps -> the decoder, the [B, V1] logits of the prefill and of every step (clones), and parts / ticket
    state seen after the first step"""
    from open_musiclm_amd import decode
    kw = dict(key_mask=True) if key_mask else {}
    dec = decode.CachedDecoder(model, B, NMAX, precision, wide=wide, kv_cache=kv_cache, **kw)
    got = [dec.prefill(rows + [flat[:, :0]], **(dict(key_mask=F.pad(mask, (0, 1), value=True)) if mask is not None else {}))[:, :V1].clone()]
    assert dec.rows == PROMPT_ROWS
    seen = None
    for k in range(STEPS):
        got.append(dec.step(flat[:, k].contiguous(), k)[:, :V1].clone())
        if k == 0:
            seen = dict(parts=dec.parts.clone(), cnt=int(dec.splitk_cnt.abs().sum()))
    assert dec.rows == PROMPT_ROWS + STEPS and int(dec.pos_dev.item()) == dec.rows
    return dec, got, seen


def _run(dev, case):  # noqa: F811
    """The decoders of a case, run once and shared by the tests below (nothing modifies them afterwards): masked with the fp32 and with the
    operand cache, all-ones mask, no mask; and the masked / unmasked re-forward logits of the grown sequence."""
    if case not in _RUNS:
        key, precision, B, wide, _ = CASES[case]
        model, wrapper = _model(dev, key, precision)
        rows, mask, flat = _masked_prompt(wrapper, dev, B, wider=WIDER.get(case))
        with torch.no_grad():
            m32 = _steps(model, rows, flat, precision, B, wide, None, True, mask)
            m16 = _steps(model, rows, flat, precision, B, wide, "operand", True, mask)
            ones = _steps(model, rows, flat, precision, B, wide, None, True, None)
            plain = _steps(model, rows, flat, precision, B, wide, None, False, None)
            want = [model.last_logits(rows + [flat[:, :k]], self_attn_mask=F.pad(mask, (0, 1 + k), value=True))[:, :V1].clone() for k in range(STEPS + 1)]
            free = [model.last_logits(rows + [flat[:, :k]])[:, :V1].clone() for k in range(STEPS + 1)]
        _RUNS[case] = dict(model=model, wrapper=wrapper, rows=rows, mask=mask, flat=flat, m32=m32, m16=m16, ones=ones, plain=plain, want=want, free=free)
    return _RUNS[case]


@pytest.mark.parametrize("case", KM_CASES)
def test_masked_steps_against_the_masked_reforward(dev, case):  # noqa: F811
    """1. The masked prefill and every masked step against last_logits(..., self_attn_mask=...) of the grown sequence, under the mode's own
    bar -- after the precondition that the mask matters by more than 10 x that bar (measured on the re-forward logits themselves)."""
    r = _run(dev, case)
    _assert_route(case)
    precision = CASES[case][1]
    bar = TOL[precision]["logits"]
    effect = min(relerr(x, y) for x, y in zip(r["free"], r["want"]))
    err = max(relerr(x, y) for x, y in zip(r["m32"][1], r["want"]))
    print(f"key mask [{case}]: masked vs unmasked re-forward, smallest rel diff over the steps {effect:.3e} (needs > {10 * bar:.1e}); "
          f"masked steps vs masked re-forward, max rel err {err:.3e} (bar {bar:.1e})")
    report(f"decode_keymask_vs_reforward[{case}]", max_rel_err=err, mask_effect=effect, steps=STEPS + 1)
    assert effect > 10 * bar, (effect, bar)
    assert len(r["m32"][1]) == STEPS + 1 and all(bool(torch.isfinite(x).all()) for x in r["m32"][1])
    assert err < bar, err
    assert r["m32"][0].key_live is not None and r["m32"][0].key_live.dtype == torch.uint8 and r["m32"][0].key_live.shape == (CASES[case][2], NMAX)
    assert torch.equal(r["m32"][0].key_live[:, :PROMPT_ROWS - 1].bool(), r["mask"]) and bool(r["m32"][0].key_live[:, PROMPT_ROWS - 1:].all())


def test_final_rows_only_honours_a_mask(dev):  # noqa: F811
    """last_logits (final_rows_only) under a mask equals the last row of the full masked forward."""
    r = _run(dev, "gen1-bf16-B3")
    model, k = r["model"], 4
    full = F.pad(r["mask"], (0, 1 + k), value=True)
    with torch.no_grad():
        all_rows = model(all_token_ids=r["rows"] + [r["flat"][:, :k]], self_attn_mask=full, return_only_final_seq_logits=True)[-1]
    assert relerr(r["want"][k], all_rows[:, -1, :V1]) < 1e-6


def test_masked_steps_against_the_oracle(dev):  # noqa: F811
    """2. The tiny bf16x3 model (gen1, fp32 weights): cached masked logits against oracle.token_conditioned_forward(self_attn_mask=...)."""
    from oracle import musiclm_oracle as O
    B, precision = 3, "bf16x3"
    model, wrapper = _model(dev, "small", precision)
    rows, mask, flat = _masked_prompt(wrapper, dev, B)
    with torch.no_grad():
        dec, got, _ = _steps(model, rows, flat, precision, B, False, None, True, mask)
    spec = O.ModelSpec([O.SeqInfo(1024, 12), O.SeqInfo(1024, 1), O.SeqInfo(1024, 3)], dim=128, depth=2, heads=2)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    c_rows, c_mask, c_flat = [t.cpu() for t in rows], mask.cpu(), flat.cpu()
    errs, effects = [], []
    for k in (0, 1, 4, 5, 8):                                  # pos 186 (prefill), 187, 190 (masked keys beside the new one), 191 -> 192 crossing, 194
        full = F.pad(c_mask, (0, 1 + k), value=True)
        want = O.token_conditioned_forward(sd, spec, c_rows + [c_flat[:, :k]], self_attn_mask=full, only_final=True)[-1][:, -1]
        free = O.token_conditioned_forward(sd, spec, c_rows + [c_flat[:, :k]], only_final=True)[-1][:, -1]
        errs.append(relerr(got[k], want[:, :V1]))
        effects.append(relerr(free[:, :V1], want[:, :V1]))
    print(f"key mask vs oracle [bf16x3, B=3]: max rel err {max(errs):.3e}; the mask's effect in the oracle {min(effects):.3e}")
    report("decode_keymask_vs_oracle[bf16x3,B=3]", max_rel_err=max(errs), mask_effect=min(effects))
    assert min(effects) > 10 * TOL["bf16"]["logits"], effects
    assert max(errs) < TOL["bf16x3"]["logits"], errs


@pytest.mark.parametrize("case", KM_CASES)
def test_a_mask_of_all_ones_is_the_unmasked_decoder(dev, case):  # noqa: F811
    """3. key_live all ones: the unmasked decoder's logits bit for bit, for the prefill and for every step."""
    r = _run(dev, case)
    assert r["plain"][0].key_live is None and bool(r["ones"][0].key_live.all())
    for k, (x, y) in enumerate(zip(r["ones"][1], r["plain"][1])):
        assert torch.equal(x, y), (case, k, float((x - y).abs().max()))
    for l in range(r["plain"][0].L):
        assert torch.equal(r["ones"][0].Kc[l], r["plain"][0].Kc[l]) and torch.equal(r["ones"][0].Vc[l], r["plain"][0].Vc[l])
    assert not torch.equal(r["m32"][1][-1], r["plain"][1][-1])


@pytest.mark.parametrize("case", KM_CASES)
def test_both_caches_give_the_same_bits_under_the_mask(dev, case):  # noqa: F811
    """4a. Under the mask the fp32 and the operand cache give the same bits."""
    r = _run(dev, case)
    assert r["m16"][0].kv_dtype == r["m16"][0].T != torch.float32 and r["m32"][0].kv_dtype == torch.float32
    for k, (x, y) in enumerate(zip(r["m32"][1], r["m16"][1])):
        assert torch.equal(x, y), (case, k, float((x - y).abs().max()))


def test_the_wide_calls_first_group_is_the_16_sample_call(dev):  # noqa: F811
    """4b. Rows 0..15 of the B = 17 call equal the B = 16 call's (the first 16 samples of the same prompt, each with its own mask)."""
    r = _run(dev, "wide-fp16ff-B17")
    key, precision, _, _, _ = CASES["wide-fp16ff-B17"]
    model, wrapper = _model(dev, key, precision)
    rows, mask, flat = [t[:16].contiguous() for t in r["rows"]], r["mask"][:16].contiguous(), r["flat"][:16].contiguous()
    with torch.no_grad():
        _, got, _ = _steps(model, rows, flat, precision, 16, False, None, True, mask)
    for k, (x, y) in enumerate(zip(got, r["m32"][1])):
        assert torch.equal(x, y[:16]), (k, float((x - y[:16]).abs().max()))


@pytest.mark.parametrize("case", KM_CASES)
def test_a_fully_masked_range_leaves_an_empty_partial(dev, case):  # noqa: F811
    """5. After a step, parts[:, 1] (rows 64..127: fully masked) has l == 0 and o == 0 for every head, every logit is finite and the
    tickets are zero again."""
    r = _run(dev, case)
    for which in ("m32", "m16"):
        dec, got, seen = r[which]
        p = seen["parts"]                                      # [B, nsplit, H, 66]: max, sum, o[64]
        assert p.shape[1] == 4 and bool((p[:, 1, :, 1] == 0).all()) and bool((p[:, 1, :, 2:] == 0).all())
        assert bool((p[:, 1, :, 0] == -3.0e38).all())
        assert bool((p[:, [0, 2], :, 1] > 0).all()) and bool(torch.isfinite(p[:, :3]).all())        # the partly masked ranges carry weight
        assert seen["cnt"] == 0 and int(dec.splitk_cnt.abs().sum()) == 0
        assert all(bool(torch.isfinite(x).all()) for x in got)
    # the unmasked decoder's range 1 is not empty: the check above sees the mask
    assert bool((r["plain"][2]["parts"][:, 1, :, 1] > 0).all())


def _gen_kw(dev, B, steps, seed=31):  # noqa: F811
    g = torch.Generator().manual_seed(seed)
    cond, _ = _raw_prompt(B, seed)
    return dict(conditioning_token_ids=[t.to(dev) for t in cond], max_time_steps=steps, uniforms=torch.rand(steps * 3, B, V1, generator=g))


def test_generate_under_the_mask(dev, monkeypatch):  # noqa: F811
    """6. generate(mask_conditioning=True) with injected uniforms (dim 1024, depth 2, fp16ff, 3 quantizers, B = 3): the same ids with and
    without use_graph, with and without kv_cache="operand"; they differ from the unmasked call's; the decoders carry the mask."""
    model, wrapper = _model(dev, "d1024", "fp16ff")
    decs, loops = _spies(monkeypatch)
    B, steps, Q = 3, 6, 3
    kw = _gen_kw(dev, B, steps)
    want = wrapper.generate(mask_conditioning=True, **kw)
    graph = wrapper.generate(mask_conditioning=True, use_graph=True, **kw)
    op = wrapper.generate(mask_conditioning=True, kv_cache="operand", **kw)
    assert want.shape == (B, steps, Q) and int(want.min()) >= 0 and int(want.max()) < 1024
    assert torch.equal(graph, want) and torch.equal(op, want)
    assert len(decs) == 3 and all(d.key_live is not None and not bool(d.key_live[:, 60:132].any()) and bool(d.key_live[:, 186:].all()) for d in decs)
    assert len(loops[1].graphs) == Q and loops[1].use_graph, "the cycles were not captured"
    assert all(int(d.splitk_cnt.abs().sum()) == 0 for d in decs)
    plain = wrapper.generate(**kw)
    assert not torch.equal(plain, want)
    # the re-forward route: every forward runs under the mask, one attended column more per id (one time step: 3 ids)
    seen, orig = [], model.last_logits
    monkeypatch.setattr(model, "last_logits", lambda ids, self_attn_mask=None: (seen.append(self_attn_mask), orig(ids, self_attn_mask))[1])
    short = dict(kw, max_time_steps=1, uniforms=kw["uniforms"][:Q])
    ref = wrapper.generate(mask_conditioning=True, use_cache=False, **short)
    assert ref.shape == (B, 1, Q) and [tuple(m.shape) for m in seen] == [(B, 187 + j) for j in range(Q)]
    assert all(not bool(m[:, 60:132].any()) and bool(m[:, 186:].all()) for m in seen)
    assert torch.equal(ref[:, 0, 0], want[:, 0, 0])           # the first id is sampled from the prefill's logits on both routes


def test_guided_generate_under_the_mask_matches_its_graph_replay(dev, monkeypatch):  # noqa: F811
    """6. cond_scale = 2: the call runs (prompts beside their null twins, the twins' condition attended) and equals its own graph replay."""
    model, wrapper = _model(dev, "d1024", "fp16ff")
    decs, _ = _spies(monkeypatch)
    B, steps = 2, 6
    kw = _gen_kw(dev, B, steps)
    want = wrapper.generate(mask_conditioning=True, cond_scale=2.0, **kw)
    graph = wrapper.generate(mask_conditioning=True, cond_scale=2.0, use_graph=True, **kw)
    assert want.shape == (B, steps, 3) and torch.equal(graph, want)
    d = decs[0]
    assert d.B == 2 * B and torch.equal(d.key_live[B:, 13:], d.key_live[:B, 13:]) and bool(d.key_live[B:, :13].all())
    assert not bool(d.key_live[:, 13].any())


def test_logprobs_under_the_mask_agree_with_score(dev):  # noqa: F811
    """6. generate(return_logprobs=True, mask_conditioning=True).model against score(mask_conditioning=True) of the ids it returned, within
    the bound the log-probability tests use for that pair: 2 TOL max|logit| + sampler_logprob_ref.tol."""
    precision = "fp16ff"
    model, wrapper = _model(dev, "d1024", precision)
    B, steps = 3, 4
    kw = _gen_kw(dev, B, steps, seed=37)
    ids, lps = wrapper.generate(mask_conditioning=True, return_logprobs=True, **kw)
    sc = wrapper.score(conditioning_token_ids=kw["conditioning_token_ids"], pred_token_ids=ids, mask_conditioning=True)
    free = wrapper.score(conditioning_token_ids=kw["conditioning_token_ids"], pred_token_ids=ids)
    assert sc.shape == ids.shape == lps.model.shape and sc.dtype == torch.float32
    rows, _, (mask, _) = wrapper._masked_condition_rows(*wrapper._condition_rows(kw["conditioning_token_ids"], True, False), True)
    flat = ids.reshape(B, -1)
    worst = 0.0
    with torch.no_grad():
        for j in range(flat.shape[1]):
            x = model.last_logits(rows + [flat[:, :j]], self_attn_mask=F.pad(mask, (0, 1 + j), value=True))[:, :V1]
            slack = 2 * TOL[precision]["logits"] * float(x.abs().max())
            s = flat[:, j]
            ls = x.double().gather(1, s[:, None])[:, 0]
            bound = slack + L.tol(ls, L.largest_kept(x, True), 1.0)
            got = lps.model.reshape(B, -1)[:, j].double()
            worst = max(worst, float(((got - sc.reshape(B, -1)[:, j].double()).abs() / bound).max()),
                        float(((got - L.lp_model(x, s, True)).abs() / bound).max()))
    print(f"masked logprobs: worst error / bound {worst:.3f}; masked vs unmasked score, max abs diff {float((sc - free).abs().max()):.3e}")
    assert worst <= 1.0, worst
    assert float((sc - free).abs().max()) > 1e-2          # the mask changes the distribution that is scored


def test_the_default_is_unchanged(dev, monkeypatch):  # noqa: F811
    """7. A call without the argument builds decoders whose key_live is None and reaches omlm_decode_step only."""
    from open_musiclm_amd import decode
    model, wrapper = _model(dev, "d1024", "fp16ff")
    decs, _ = _spies(monkeypatch)
    names = []
    orig = decode.call
    monkeypatch.setattr(decode, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    kw = _gen_kw(dev, 3, 3)
    wrapper.generate(**kw)
    assert decs and all(d.key_live is None for d in decs)
    assert "omlm_decode_step" in names and "omlm_decode_step_masked" not in names
    names.clear()
    wrapper.generate(mask_conditioning=True, **kw)
    assert "omlm_decode_step_masked" in names and "omlm_decode_step" not in names


def test_a_null_mask_is_refused_at_the_c_boundary(dev):  # noqa: F811
    """omlm_decode_step_masked without key_live: the library's argument error, before any launch."""
    import ctypes as C
    from open_musiclm_amd import hip
    from open_musiclm_amd import decode
    model, wrapper = _model(dev, "small", "bf16")
    rows, mask, flat = _masked_prompt(wrapper, dev, 1)
    dec = decode.CachedDecoder(model, 1, NMAX, "bf16", key_mask=True)           # (a decoder of its own: the shared ones stay untouched)
    with torch.no_grad():
        dec.prefill(rows + [flat[:, :0]], key_mask=F.pad(mask, (0, 1), value=True))
    before = (int(dec.pos_dev.item()), dec.logits.clone())
    dec.args.emb_table, dec.args.head_W = dec.emb.data_ptr(), dec.pw.heads[-1][0].data_ptr()
    rc = hip.lib().omlm_decode_step_masked(C.addressof(dec.args), None, hip.ptr(flat[:, 0].contiguous()), hip.stream_ptr())
    assert rc == -1 and b"null key_live" in hip.lib().omlm_last_error()
    torch.cuda.synchronize()
    assert int(dec.pos_dev.item()) == before[0] and torch.equal(dec.logits, before[1])
