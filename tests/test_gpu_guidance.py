"""GPU: classifier-free guidance on the condition -- omlm_guide_logits and omlm_decode_twin (csrc/sampler.hip), the condition drop of
omlm_prepare_train_batch (csrc/embed_ce.hip), TokenConditionedTransformerWrapper(null_cond_prob=), decode.SamplingLoop(guidance=),
generate(cond_scale=) on its three routes, score(cond_scale=) and MusicLM.forward(cond_scale=).

Against tests/guidance_ref.py (the float32 guide rule bit for bit, the null raw ids, the drop rule) and the CPU oracle on the null raw
ids.  Everything that compares the product with itself (replay, cuts, routes, off) is exact."""
import numpy as np
import pytest
import torch

import guidance_ref as G
import sampler_logprob_ref as L
from test_gpu_kernels import dev, ops, report  # noqa: F401  (the shared fixtures)
from test_gpu_model import TOL, relerr

pytestmark = pytest.mark.gpu

POISON = 12345.0
SEED = 0x9E3779B97F4A7C15
_MODELS = {}


def _small(dev, precision="fp16ff"):
    """dim 64, 2 heads, depth 2, CLAP Q = 3, predicted Q = 3, V1 = 41: the first-generation step kernels (B = 2 for one pair)."""
    from open_musiclm_amd import open_musiclm as M
    key = ("small", precision)
    if key not in _MODELS:
        torch.manual_seed(1)
        m = M.create_coarse_transformer(dim=64, depth=2, heads=2, ff_dropout=0.0, num_coarse_quantizers=3, num_clap_quantizers=3,
                                        clap_codebook_size=32, semantic_codebook_size=48, acoustic_codebook_size=40, precision=precision).to(dev)
        m.eval()
        _MODELS[key] = (m, M.TokenConditionedTransformerWrapper(transformer=m, unique_consecutive=False))
    return _MODELS[key]


def _wide(dev, precision):
    """dim 1024, depth 1, 8 heads, Q = 3, V1 = 1025: the matrix-core step route for B >= 2 on the 16-bit precisions."""
    from open_musiclm_amd import open_musiclm as M
    key = ("wide", precision)
    if key not in _MODELS:
        torch.manual_seed(0)
        m = M.create_coarse_transformer(dim=1024, depth=1, heads=8, ff_dropout=0.0, num_coarse_quantizers=3, precision=precision).to(dev)
        m.eval()
        _MODELS[key] = (m, M.TokenConditionedTransformerWrapper(transformer=m, unique_consecutive=False))
    return _MODELS[key]


def _cond(model, B, dev, n_clap=2, n_sem=7, seed=5):
    g = torch.Generator().manual_seed(seed)
    s0, s1 = model.token_sequences[0], model.token_sequences[1]
    return [torch.randint(0, s0.codebook_size, (B, n_clap, s0.num_quantizers), generator=g).to(dev),
            torch.randint(0, s1.codebook_size, (B, n_sem), generator=g).to(dev)]


def _stacked(wrapper, cond):
    """generate's 2P-row prompt: (condx of the prompts, condx of the null twins) stacked, and the count of rows they take."""
    from open_musiclm_amd.utils import append_eos_id
    info = wrapper.token_sequences[0]
    condx = [append_eos_id(t.reshape(t.shape[0], -1).long(), e) for t, e in zip(cond, wrapper.eos_ids)]
    twin0 = G.null_twin(condx[0], info.codebook_size, info.num_quantizers, condx[0].shape[1] - 1)
    return condx, [twin0] + condx[1:], sum(t.shape[-1] + 1 for t in condx) + 1


# ---- 1. the guide kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1025, 2049])
def test_guide_kernel_is_bit_equal_to_the_restatement(ops, dev, V):
    gen = torch.Generator().manual_seed(V)
    for rows in (1, 3, 64):
        for ld in (V, (V + 7) // 8 * 8 + 8):
            l = torch.full((rows, ld), POISON)
            n = torch.full((rows, ld), POISON)
            l[:, :V] = torch.randn(rows, V, generator=gen) * 9
            n[:, :V] = torch.randn(rows, V, generator=gen) * 9
            n[0, 0] = l[0, 0]                                          # an exact zero difference
            ld_, nd_ = l.to(dev), n.to(dev)
            for s in (0.0, 0.5, 3.0):
                want = G.guide(l[:, :V], n[:, :V], s)
                out = torch.full((rows, ld), POISON, device=dev)
                ops.guide_logits(ld_, nd_, out, V, s)
                got = out.cpu().numpy()
                assert np.array_equal(got[:, :V].view(np.uint32), want.view(np.uint32)), (V, rows, ld, s)
                assert bool((out[:, V:] == POISON).all()), (V, rows, ld, s)                    # the pad columns are not written
                alias = ld_.clone()
                ops.guide_logits(alias, nd_, alias, V, s)                                       # out may be cond
                assert torch.equal(alias, out.where(torch.arange(ld, device=dev)[None] < V, ld_)), (V, rows, ld, s)
    # a view whose base is not 16-byte aligned takes the scalar path and gives the same bits
    base = torch.full((3 * 72 + 1,), POISON, device=dev)
    lv, nv, ov = (base.clone()[1:].view(3, 72) for _ in range(3))
    lv[:, :64], nv[:, :64] = torch.randn(3, 64, device=dev), torch.randn(3, 64, device=dev)
    ops.guide_logits(lv, nv, ov, 64, 3.0)
    assert np.array_equal(ov[:, :64].cpu().numpy(), G.guide(lv[:, :64], nv[:, :64], 3.0)) and bool((ov[:, 64:] == POISON).all())
    with pytest.raises(ValueError, match="scale"):
        ops.guide_logits(lv, nv, ov, 64, -1.0)


# ---- 2. the twin kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(1, 64), (5, 1024), (3, 6), (64, 1024)])
def test_twin_kernel_copies_ids_and_rows(ops, dev, rows, D):
    g = torch.Generator().manual_seed(rows)
    ids = torch.randint(-5, 2 ** 40, (2 * rows,), generator=g).to(dev)
    x = torch.randn(2 * rows, D, generator=g).to(dev)
    i0, x0 = ids.clone(), x.clone()
    ops.decode_twin(ids[:rows], ids[rows:], x[:rows], x[rows:])
    assert torch.equal(ids[rows:], i0[:rows]) and torch.equal(ids[:rows], i0[:rows])
    assert torch.equal(x[rows:], x0[:rows]) and torch.equal(x[:rows], x0[:rows])
    ids, x = i0.clone(), x0.clone()
    ops.decode_twin(ids=ids[:rows], ids_twin=ids[rows:])                      # no rows
    assert torch.equal(ids[rows:], i0[:rows]) and torch.equal(x, x0)
    ids, x = i0.clone(), x0.clone()
    ops.decode_twin(x=x[:rows], x_twin=x[rows:])                              # no ids
    assert torch.equal(x[rows:], x0[:rows]) and torch.equal(ids, i0)
    ops.decode_twin()                                                         # nothing: no launch
    with pytest.raises(ValueError, match="decode_twin"):
        ops.decode_twin(ids=ids[:rows])


# ---- 3. the prepare kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forgetful", [False, True])
def test_prepare_kernel_drops_the_condition(ops, dev, forgetful, monkeypatch):
    from open_musiclm_amd import engine
    from open_musiclm_amd import open_musiclm as M
    from oracle import musiclm_oracle as O
    model, _ = _small(dev)
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, mask_prob=0.15 if forgetful else 0.0).train()
    B, p = 4, float(np.float32(0.3))
    g = torch.Generator().manual_seed(7)
    raw = [torch.randint(0, 32, (B, 2, 3), generator=g), torch.randint(0, 48, (B, 9), generator=g), torch.randint(0, 40, (B, 4, 3), generator=g)]
    raw[0][0, 0, 1] = -1                                             # a padded condition id in a sample that is dropped: attended all the same
    raw = [t.to(dev) for t in raw]
    flat = [t.reshape(B, -1).long().contiguous() for t in raw]
    N = sum(t.shape[1] + 1 for t in flat) + len(flat) - 1
    n_drop = min(int(N * 0.15), N - 1) if forgetful else 0
    scores = torch.randn(B, N, generator=g).to(dev) if forgetful else None
    u = torch.tensor([0.0, float(np.nextafter(np.float32(p), np.float32(0))), p, 0.99], device=dev)
    seqs = model.token_sequences
    args = (flat, [int(e) for e in wrapper.eos_ids], [s.num_quantizers for s in seqs], [s.codebook_size for s in seqs], wrapper.pad_id, scores,
            n_drop, [True] * 3)
    base = ops.prepare_train_batch(*args)
    none = ops.prepare_train_batch(*args, null_u=None, null_p=0.7)
    for a, b in zip(base[:2] + tuple(base[2]), none[:2] + tuple(none[2])):
        assert torch.equal(a, b)                                     # null_u=None: the current output, bit for bit
    ids32, keymask, labels, lens = ops.prepare_train_batch(*args, null_u=u, null_p=p)
    # the torch path on the same scores, then the host rule
    forget = O.forgetful_mask_from_noise(scores.cpu(), 0.15).to(dev) if forgetful else None
    monkeypatch.setattr(M, "generate_mask_with_prob", lambda shape, pr, device: forget)
    t_ids, t_labels, t_mask = wrapper._prepare(raw, True, False)
    want0, want_mask, dropped = G.apply_drop(t_ids[0], t_mask, forget, u, p, 32, 3, 6)
    assert dropped.tolist() == [True, True, False, False]            # u == p is kept: the boundary is <
    want32, want_lens = engine.build_ids(model, [want0] + t_ids[1:])
    assert torch.equal(ids32, want32) and list(lens) == list(want_lens)
    assert torch.equal(keymask.bool(), want_mask)
    for a, b in zip(labels, t_labels):
        assert torch.equal(a.long(), b)
    assert bool((ids32[:2, 1:7] == -1).all()) and not bool((ids32[2:, 1:7] == -1).any())
    assert torch.equal(ids32[:, 7:], base[0][:, 7:]) and torch.equal(ids32[2:], base[0][2:])      # the eos and everything behind it; kept samples
    if not forgetful:
        assert bool(keymask[:2, 1:7].all()) and int(base[1][0, 2]) == 0
    with pytest.raises(ValueError, match="null_p"):
        ops.prepare_train_batch(*args, null_u=u, null_p=1.5)
    model.eval()                                                     # (the shared model is left as it was found)


# ---- 4. training -------------------------------------------------------------------------------------------------------------------------
def _oracle_null_loss(sd, spec, ids, weights, n_ids):
    """The oracle's training loss on the null condition as the drop rule states it: build_training_inputs on the REAL ids (labels, last-id
    drop, key mask: every condition position attended), the null raw ids in place of the condition's ids, the oracle's unmodified
    forward, and wrapper_forward_loss's own weighting.  (wrapper_forward_loss cannot be handed the null raw ids themselves: its
    build_training_inputs reads the raw -1 at every position with p mod Q == 0 as padding and key-masks it --
    tests/test_guidance_host.py::test_oracle_training_inputs_key_mask_a_raw_minus_one -- which the decided drop rule does not.  On the
    golden tiny coarse model the two oracle values are 18.88728 (wrapper_forward_loss on the null raw ids: one CLAP position of twelve
    key-masked) and 18.82303 (this function), 3.4e-3 apart; the product gives the second within 4e-6 (bf16x3) and 1.9e-5 (fp16ff).)"""
    import torch.nn.functional as F
    from oracle import musiclm_oracle as O
    o_ids, labels, mask = O.build_training_inputs(ids, spec)
    s0 = spec.token_sequences[0]
    o_ids[0] = G.null_twin(o_ids[0], s0.codebook_size, s0.num_quantizers, n_ids)
    logits = [l.transpose(1, 2) for l in O.token_conditioned_forward(sd, spec, o_ids, mask)]
    total, running = 0, 0.0
    for lg, lb, w in zip(logits, labels, weights):
        if w > 0:
            running = running + F.cross_entropy(lg, lb) * lb.numel() * w
            total += lb.numel()
    return running / total, logits


def _clap_grad_off_the_eos_row(model, n_ids):
    """Largest |gradient| of the CLAP embedding table outside the one row the condition's appended eos position embeds.  That position is
    untouched by the drop: as in every training step it is key-masked and embeds id 0 of its quantizer (open_musiclm.py:359-363), row
    codebook * (n_ids mod Q), and its embedding reaches the rows behind it through the causal depthwise convolution of the feed-forward,
    which no key mask covers -- so that one row keeps a gradient.  Every id position of a dropped sample embeds the zero row and sends
    nothing to the table."""
    g = model.embeddings[0].weight.grad
    if g is None:
        return 0.0
    info = model.token_sequences[0]
    keep = torch.ones(g.shape[0], dtype=torch.bool, device=g.device)
    keep[info.codebook_size * (n_ids % info.num_quantizers) if info.num_quantizers > 1 else 0] = False
    return float(g[keep].abs().max())


@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_training_on_the_null_condition_matches_the_oracle(golden_dir, dev, precision, monkeypatch):
    """null_cond_prob = 1: every sample trains on the null condition.  Loss (both the torch path and the fused one-launch path) against
    the oracle within the loss bar of tests/test_gpu_model.py, the last sequence's logits within its logits bar, and no id position sends
    a gradient to the CLAP embedding table (_clap_grad_off_the_eos_row: exactly zero; measured with the table's whole gradient, the one
    row of the untouched eos position holds ~8e-4)."""
    from oracle import musiclm_oracle as O
    from open_musiclm_amd import open_musiclm as M
    from test_gpu_model import build_from_golden
    z, model = build_from_golden(golden_dir, "tiny_coarse", dev, precision)
    spec = O.ModelSpec([O.SeqInfo(32, 12), O.SeqInfo(48, 1), O.SeqInfo(40, 3)], dim=128, depth=2, heads=2)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ids = [torch.from_numpy(z[f"ids.{i}"]) for i in range(3)]
    weights = [0., 0., 1.]
    want, o_logits = _oracle_null_loss(sd, spec, ids, weights, 12)
    plain, _, _ = O.wrapper_forward_loss(sd, spec, ids, weights)
    assert abs(float(want) - float(plain)) > 1e-3 * float(plain)                # the condition matters to this model
    wrapper = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=weights,
                                                   mask_prob=0.0, null_cond_prob=1.).train()
    dids = [t.to(dev) for t in ids]
    tol = TOL[precision]
    errs = {}
    for path, kw in (("torch", dict()), ("fused", dict(return_logits=False))):
        model.zero_grad(set_to_none=True)
        loss, logits, _ = wrapper(all_token_ids=dids, return_loss=True, **kw)
        loss.backward()
        errs[path] = abs(float(loss.detach()) - float(want)) / float(want)
        assert _clap_grad_off_the_eos_row(model, 12) == 0.0, path
        assert float(model.embeddings[1].weight.grad.abs().max()) > 0
        if path == "torch":
            errs["logits"] = relerr(logits[-1], o_logits[-1])
    print(f"null-condition training [{precision}]: loss rel err {errs}")
    report(f"guidance_train_null[{precision}]", **errs)
    assert errs["torch"] < tol["loss"] and errs["fused"] < tol["loss"] and errs["logits"] < tol["logits"], errs
    # eval never drops
    wrapper.eval()
    with torch.no_grad():
        ev, _, _ = wrapper(all_token_ids=dids, return_loss=True)
    assert abs(float(ev) - float(plain)) < tol["loss"] * float(plain)
    # and without the drop the id positions do reach the table
    plain_w = M.TokenConditionedTransformerWrapper(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=weights, mask_prob=0.0).train()
    model.zero_grad(set_to_none=True)
    plain_w(all_token_ids=dids, return_loss=True, return_logits=False)[0].backward()
    assert _clap_grad_off_the_eos_row(model, 12) > 0.0


def test_probability_zero_is_the_wrapper_without_the_keyword(dev):
    """Loss, gradients and the device RNG state afterwards, on the fused path and the torch path, with the forgetful mask on."""
    from open_musiclm_amd import open_musiclm as M
    model, _ = _small(dev, "bf16x3")
    raw = _cond(model, 3, dev) + [torch.randint(0, 40, (3, 4, 3), generator=torch.Generator().manual_seed(2)).to(dev)]
    kw = dict(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.15)
    out = {}
    for name, w in (("without", M.TokenConditionedTransformerWrapper(**kw)), ("zero", M.TokenConditionedTransformerWrapper(null_cond_prob=0., **kw))):
        w.train()
        for path, pk in (("fused", dict(return_logits=False)), ("torch", dict())):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(77)
            loss, _, _ = w(all_token_ids=raw, return_loss=True, **pk)
            loss.backward()
            out[name, path] = (float(loss), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                               torch.cuda.get_rng_state(dev).clone())
    model.zero_grad(set_to_none=True)
    model.eval()
    for path in ("fused", "torch"):
        (la, ga, ra), (lb, gb, rb) = out["without", path], out["zero", path]
        assert torch.equal(ra, rb), path                                  # nothing was drawn
        assert abs(la - lb) <= 2e-6 * abs(la), (path, la, lb)             # (the loss sums its rows with atomics)
        assert ga.keys() == gb.keys()
        scale = max(float(v.abs().max()) for v in ga.values())
        for k in ga:                                                      # (so does the backward: equal up to the order of addition)
            # (the bar two runs of one backward are held to: test_full_size_backward_is_reproducible, bf16x3)
            assert float((ga[k] - gb[k]).abs().max()) <= 1e-3 * max(float(ga[k].abs().max()), 1e-3 * scale), (path, k)


def test_fused_and_torch_paths_drop_the_same_samples(dev, monkeypatch):
    """null_cond_prob = 0.5, one seed, forgetful mask on: both paths draw randn then rand, so they drop the same samples and give the same loss."""
    from open_musiclm_amd import open_musiclm as M
    model, _ = _small(dev, "bf16x3")
    B = 6
    raw = _cond(model, B, dev) + [torch.randint(0, 40, (B, 4, 3), generator=torch.Generator().manual_seed(2)).to(dev)]
    kw = dict(transformer=model, unique_consecutive=False, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.15)
    w = M.TokenConditionedTransformerWrapper(null_cond_prob=0.5, **kw).train()
    w0 = M.TokenConditionedTransformerWrapper(**kw).train()
    torch.manual_seed(31)
    N = sum(t[0].numel() + 1 for t in raw) + 2
    torch.randn(B, N, device=dev)
    u = torch.rand(B, device=dev)
    assert 0 < int((u < 0.5).sum()) < B, u.tolist()                       # this seed drops some samples and keeps others
    with torch.no_grad():
        torch.manual_seed(31)
        lf, _, _ = w(all_token_ids=raw, return_loss=True, return_logits=False)
        rf = torch.cuda.get_rng_state(dev).clone()
        torch.manual_seed(31)
        l0, _, _ = w0(all_token_ids=raw, return_loss=True, return_logits=False)
        monkeypatch.setenv("OMLM_FUSED_PREP", "0")
        torch.manual_seed(31)
        lt, _, _ = w(all_token_ids=raw, return_loss=True, return_logits=False)
        rt = torch.cuda.get_rng_state(dev).clone()
    model.eval()
    assert abs(float(lf) - float(lt)) < 2e-6 * abs(float(lt)), (float(lf), float(lt))
    assert torch.equal(rf, rt)                                            # the same consumption of the generator
    assert abs(float(lf) - float(l0)) > 1e-4 * abs(float(l0)), (float(lf), float(l0))      # and the drop is not a no-op


@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_graphed_and_eager_micro_steps_agree_with_the_drop(dev, precision):
    """The pattern of test_graphed_bf16x3_training_tracks_eager_over_optimizer_steps (tests/test_gpu_model.py) and its bars, on the small
    model: the captured micro-step carries the rand draw and the drop kernel.  At null_cond_prob = 1 with the forgetful mask off every
    replay drops every sample whatever it draws, so graph replays and eager calls see the same inputs and give the same losses over three
    optimizer steps -- and not the losses of a run without the drop."""
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.graph import GraphedForwardBackward
    from open_musiclm_amd.optimizer import get_optimizer
    B = 2
    g = torch.Generator().manual_seed(3)
    batches = [[torch.randint(0, 32, (B, 2, 3), generator=g).to(dev), torch.randint(0, 48, (B, 9), generator=g).to(dev),
                torch.randint(0, 40, (B, 6, 3), generator=g).to(dev)] for _ in range(3)]
    keys = ("clap_token_ids", "semantic_token_ids", "coarse_token_ids")

    def run(use_graph, p):
        torch.manual_seed(0)
        model = M.create_coarse_transformer(dim=64, depth=2, heads=2, ff_dropout=0.0, num_coarse_quantizers=3, num_clap_quantizers=3,
                                            clap_codebook_size=32, semantic_codebook_size=48, acoustic_codebook_size=40, precision=precision).to(dev)
        stage = M.CoarseStage(coarse_transformer=model, cross_entropy_loss_weights=[0., 0., 1.], mask_prob=0.0, null_cond_prob=p).train()
        opt = get_optimizer(model.parameters(), lr=3e-3, wd=0.01)
        opt.zero_grad()
        fb = GraphedForwardBackward(lambda **kw: stage(**kw, return_loss=True, return_logits=False)[0], enabled=use_graph, instances=1)

        def discard():
            opt.mark_grads_dirty()
            opt.zero_grad()
        fb.prepare(dict(zip(keys, batches[0])), after_warmup=discard)
        assert (fb.graph is not None) == use_graph, fb.capture_error
        losses = []
        for k in range(3):
            opt.zero_grad()
            loss = fb(**dict(zip(keys, batches[k])))
            opt.mark_grads_dirty()
            opt.step(max_grad_norm=0.5)
            losses.append(float(loss))
        g0 = _clap_grad_off_the_eos_row(model, 6)
        import gc
        gc.unfreeze()
        return losses, model.embeddings[1].weight.detach().clone(), g0
    le, we, ge = run(False, 1.)
    lg, wg, gg = run(True, 1.)
    l0, _, _ = run(False, 0.)
    print(f"graph vs eager with the drop [{precision}]: eager {le} graph {lg} without {l0}")
    for a, b in zip(le, lg):
        assert abs(a - b) <= (2e-4 if precision == "bf16x3" else 5e-3) * abs(a), (le, lg)
    assert abs(le[0] - l0[0]) > 1e-3 * abs(l0[0]), (le, l0)
    assert ge == 0.0 and gg == 0.0                                   # no id position sent a gradient to the CLAP table in either run


# ---- 5. guided logits against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16ff", "bf16x3"])
def test_guided_logits_against_the_oracle(ops, dev, precision):
    """dim 1024, depth 1, 8 heads, Q = 3, two prompts and their null twins in one 4-row decoder: at the prefill row and after each of 4
    teacher-forced steps g (omlm_guide_logits over the two halves of the decoder's logits) against the oracle's two forwards combined in
    fp64.  Each branch lies within the mode's logits bar e of its row (relative to the row's largest entry), and g = s l + (1 - s) n,
    so |g - g_oracle| <= (|s| + |1 - s|) e max(|l|, |n|)."""
    from open_musiclm_amd import decode
    from oracle import musiclm_oracle as O
    model, wrapper = _wide(dev, precision)
    spec = O.coarse_spec(dim=1024, depth=1, heads=8)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    P, V1, n0, steps = 2, 1025, 2, 4
    cond = _cond(model, P, dev, n_clap=1, n_sem=9)
    condx, twin, prompt_rows = _stacked(wrapper, cond)
    flat = torch.randint(0, 1024, (P, n0 + steps), generator=torch.Generator().manual_seed(9)).to(dev)
    rows = prompt_rows + n0 + steps
    worst = {}
    with torch.no_grad():
        dec = decode.CachedDecoder(model, 2 * P, rows, precision, wide=True)
        both = lambda t: torch.cat((t, t), dim=0)                     # noqa: E731
        lg = [dec.prefill([torch.cat((c, t), dim=0) for c, t in zip(condx, twin)] + [both(flat[:, :n0])]).clone()]
        for k in range(n0, n0 + steps):
            lg.append(dec.step(both(flat[:, k]).contiguous(), k).clone())
        o_c = O.token_conditioned_forward(sd, spec, [t.cpu() for t in condx] + [flat.cpu()], only_final=True)[-1]
        o_n = O.token_conditioned_forward(sd, spec, [t.cpu() for t in twin] + [flat.cpu()], only_final=True)[-1]
        for s in (0.0, 0.5, 3.0):
            errs = []
            for i, x in enumerate(lg):
                out = torch.empty(P, dec.ldV, device=dev)
                ops.guide_logits(x[:P], x[P:], out, V1, s)
                oc, on = o_c[:, n0 + i], o_n[:, n0 + i]
                want = G.guide64(oc, on, s)
                scale = max(float(oc.abs().max()), float(on.abs().max()))
                errs.append(float((out[:, :V1].cpu().double() - want).abs().max()) / (G.factor(s) * scale))
            worst[s] = max(errs)
        branch = max(max(relerr(x[:P, :V1], o_c[:, n0 + i]), relerr(x[P:, :V1], o_n[:, n0 + i])) for i, x in enumerate(lg))
        differ = float((o_c[:, n0] - o_n[:, n0]).abs().max() / o_c[:, n0].abs().max())
    print(f"guided logits vs oracle [{precision}]: error / ((|s| + |1 - s|) max|row|) {worst}; branches {branch:.2e}; cond vs null {differ:.2e}")
    report(f"guidance_logits_vs_oracle[{precision}]", branch=branch, cond_vs_null=differ, **{f"s={s}": v for s, v in worst.items()})
    assert differ > 10 * TOL[precision]["logits"]                        # the two branches are different rows
    assert max(worst.values()) < TOL[precision]["logits"], worst


# ---- 6. replay ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,precision", [("small", "fp16ff"), ("small", "bf16x3"), ("wide", "fp16ff")])
def test_guided_loop_equals_a_step_by_step_replay(ops, dev, which, precision):
    """P = 1: generate(cond_scale=s) on the cached route against a 2-row CachedDecoder driven with `step` -- the null twin prompt, the
    guide rule on the host (the restatement), ops.sample on the same uniforms.  Ids equal id for id; lp_model is the log-softmax of g.
    Fails where cond_scale is ignored: the replay at s = 3 is not the unguided call."""
    from open_musiclm_amd import decode
    model, wrapper = _small(dev, precision) if which == "small" else _wide(dev, precision)
    route = decode.step_route(2, *decode._geometry(model), precision != "bf16x3", wide=True)
    assert route == ("gen1" if which == "small" else "dec4"), route
    seq = model.token_sequences[-1]
    V1, Q, steps, T, s = seq.codebook_size + 1, seq.num_quantizers, 3, 0.9, 3.0
    n_new = steps * Q
    k = max(int((1 - 0.9) * V1), 1)
    cond = _cond(model, 1, dev, seed=8)
    U = torch.rand(n_new, 1, V1, generator=torch.Generator().manual_seed(4)).to(dev)
    ids, lps = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, uniforms=U, cond_scale=s, return_logprobs=True)
    unguided = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, uniforms=U)
    condx, twin, prompt_rows = _stacked(wrapper, cond)
    with torch.no_grad():
        dec = decode.CachedDecoder(model, 2, prompt_rows + n_new, precision, wide=True)
        logits = dec.prefill([torch.cat((c, t), dim=0) for c, t in zip(condx, twin)] + [torch.empty(2, 0, dtype=torch.long, device=dev)])
        replay, worst = [], 0.0
        out = torch.empty(1, dtype=torch.long, device=dev)
        for j in range(n_new):
            g = G.guide(logits[0:1, :V1], logits[1:2, :V1], s)
            gd = torch.zeros(1, dec.ldV, device=dev)
            gd[:, :V1] = torch.from_numpy(g).to(dev)
            ops.sample(gd, out, V1, k, T, True, uniform=U[j])
            replay.append(int(out))
            x = torch.from_numpy(g)
            want = G.log_softmax64(x)[0, int(out)]
            bound = L.tol(float(x[0, int(out)]), float(x[0, :V1 - 1].max()), 1.0)
            worst = max(worst, abs(float(lps.model.reshape(-1)[j]) - float(want)) / bound)
            if j < n_new - 1:
                logits = dec.step(out.repeat(2).contiguous(), j)
    print(f"guided replay [{which},{precision}]: ids {replay}; lp_model error / tol {worst:.3f}")
    assert ids.reshape(-1).tolist() == replay, (ids.reshape(-1).tolist(), replay)
    assert worst <= 1.0, worst
    assert not torch.equal(ids, unguided)                                  # guidance moved at least one of the ids


# ---- 7. cuts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [9, 32])
def test_guided_ids_do_not_depend_on_how_the_batch_is_cut(dev, P, monkeypatch):
    """Counter stream.  P = 9: 18 rows, two groups of the wide step, the null half [9, 18) across the group boundary; P = 32: the full wide
    call.  The ids equal those of calls that hold one pair each (row0 of the stream = the prompt's index)."""
    from open_musiclm_amd import decode
    precision = "fp16ff"
    model, wrapper = _wide(dev, precision)
    assert decode.max_call_batch(model, precision) == 64
    cond = _cond(model, P, dev, n_clap=1, n_sem=9, seed=P)
    kw = dict(conditioning_token_ids=cond, max_time_steps=2, sampler_rng="counter", sampler_seed=SEED, cond_scale=2.5)
    sizes, init = [], decode.CachedDecoder.__init__

    def recording_init(self, model_, batch, *a, **k):
        sizes.append(batch)
        init(self, model_, batch, *a, **k)
    monkeypatch.setattr(decode.CachedDecoder, "__init__", recording_init)
    whole = wrapper.generate(**kw)
    assert sizes == [2 * P]
    monkeypatch.setattr(decode, "max_call_batch", lambda *a, **k: 2)
    cut = wrapper.generate(**kw)
    assert sizes[1:] == [2] * P
    assert whole.shape == (P, 2, 3) and torch.equal(cut, whole), (cut.tolist(), whole.tolist())
    assert len({tuple(r) for r in whole.reshape(P, -1).tolist()}) > 1


# ---- 8. routes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "fp16ff"])
def test_guided_routes_agree_and_score_is_the_twin(dev, precision):
    """The small model, P = 3, 6 time steps = 18 ids (the graph loop captures at id 3): cached, captured graph and re-forward routes give
    the same ids, from a uniform buffer and from the counter stream, with a nucleus and a 16-bit cache; a primed call; and
    score(cond_scale=s) of the returned ids against generate's LogProbs.model within the score-against-generate bound of
    tests/test_gpu_sampler_logprob.py times |s| + |1 - s|."""
    model, wrapper = _small(dev, precision)
    P, steps, Q, V1, s, T = 3, 6, 3, 41, 3.0, 0.8
    cond = _cond(model, P, dev, seed=12)
    U = torch.rand(steps * Q, P, V1, generator=torch.Generator().manual_seed(11))
    routes = (("cached", dict(use_cache=True)), ("graph", dict(use_cache=True, use_graph=True)), ("uncached", dict(use_cache=False)))
    for name, src in (("buffer", dict(uniforms=U)), ("counter", dict(sampler_rng="counter", sampler_seed=SEED)),
                      ("buffer,top_p,kv16", dict(uniforms=U, top_p=0.9, kv_cache="operand"))):
        res = {}
        for route, kw in routes:
            ids, lps = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, cond_scale=s, return_logprobs=True, **src, **kw)
            plain = wrapper.generate(conditioning_token_ids=cond, max_time_steps=steps, temperature=T, cond_scale=s, **src, **kw)
            assert ids.shape == (P, steps, Q) and lps.model.shape == (P, steps, Q) and torch.equal(ids, plain), (name, route)
            res[route] = (ids, lps)
        for route in ("graph", "uncached"):
            assert torch.equal(res[route][0], res["cached"][0]), (name, route, res[route][0].tolist(), res["cached"][0].tolist())
        assert torch.equal(res["graph"][1].model, res["cached"][1].model) and torch.equal(res["graph"][1].sampled, res["cached"][1].sampled)
        ids, lps = res["cached"]
        # score: the teacher-forced twin
        sc = wrapper.score(conditioning_token_ids=cond, pred_token_ids=ids, cond_scale=s)
        sc_plain = wrapper.score(conditioning_token_ids=cond, pred_token_ids=ids)
        assert sc.shape == ids.shape and not torch.allclose(sc, sc_plain, atol=1e-3)
        big = 0.0
        with torch.no_grad():
            condx, twin, _ = _stacked(wrapper, cond)
            flat = ids.reshape(P, -1)
            for j in range(flat.shape[1]):
                big = max(big, float(model.last_logits(condx + [flat[:, :j]])[:, :V1].abs().max()), float(model.last_logits(twin + [flat[:, :j]])[:, :V1].abs().max()))
        # the existing bound is 2 e max|logit| + tol(l_s, m); |g| <= (|s| + |1 - s|) max(|l|, |n|) bounds tol's arguments
        bound = G.factor(s) * (2 * TOL[precision]["logits"] * big + L.tol(G.factor(s) * big, G.factor(s) * big, 1.0))
        err = float((sc - lps.model).abs().max()) / bound
        eu = float((res["uncached"][1].model - lps.model).abs().max()) / bound
        print(f"guided score vs generate [{precision},{name}]: worst error / bound {err:.3f}; re-forward vs cached lp_model {eu:.3f} (bound {bound:.2e})")
        report(f"guidance_score_vs_generate[{precision},{name}]", err_over_bound=err, reforward_over_bound=eu)
        assert err <= 1.0 and eu <= 1.0, (err, eu)
    # a primed call: the prompt's ids are duplicated to the twin; ids and log-probabilities cover what THIS call sampled
    first = res["cached"][0][:, :2]
    a, la = wrapper.generate(conditioning_token_ids=cond, pred_token_ids=first, max_time_steps=4, cond_scale=s, return_logprobs=True, uniforms=U)
    b = wrapper.generate(conditioning_token_ids=cond, pred_token_ids=first, max_time_steps=4, cond_scale=s, uniforms=U, use_cache=False)
    assert a.shape == (P, 4, Q) and la.model.shape == (P, 2, Q) and torch.equal(a[:, :2], first) and torch.equal(a, b)


def test_stages_trainer_and_musiclm_pass_the_scale_on(dev):
    from open_musiclm_amd import open_musiclm as M
    model, wrapper = _small(dev)
    cond = _cond(model, 2, dev)
    kw = dict(max_time_steps=3, sampler_rng="counter", sampler_seed=5)
    want = wrapper.generate(conditioning_token_ids=cond, cond_scale=3, **kw)
    plain = wrapper.generate(conditioning_token_ids=cond, **kw)
    stage = M.CoarseStage(coarse_transformer=model)
    got = stage.generate(clap_token_ids=cond[0], semantic_token_ids=cond[1], cond_scale=3, **kw)
    assert torch.equal(got, want) and not torch.equal(want, plain)
    # MusicLM.forward: a mapping guides the named stage alone; windows generated together hold half as many per decode call
    torch.manual_seed(0)
    mk = dict(dim=64, depth=1, heads=1, precision="bf16")
    lm = M.MusicLM(semantic_transformer=M.create_semantic_transformer(**mk).to(dev),
                   coarse_transformer=M.create_coarse_transformer(num_coarse_quantizers=3, **mk).to(dev),
                   fine_transformer=M.create_fine_transformer(num_coarse_quantizers=3, num_fine_quantizers=5, **mk).to(dev))
    clap = torch.randint(0, 1024, (1, 12, 1), device=dev)
    fk = dict(clap_token_ids=clap, output_seconds=2, semantic_window_seconds=1, coarse_window_seconds=1, fine_window_seconds=1,
              semantic_steps_per_second=10, acoustic_steps_per_second=6, return_tokens=True, sampler_rng="counter", fine_windows_together=True)
    outs = {}
    for name, cs in (("off", None), ("one", 1), ("coarse", {"coarse": 4.0}), ("all", 4.0)):
        torch.manual_seed(9)
        outs[name] = lm(cond_scale=cs, **fk)
    assert all(torch.equal(a, b) for a, b in zip(outs["off"], outs["one"]))
    assert torch.equal(outs["coarse"][0], outs["off"][0]) and not torch.equal(outs["coarse"][1], outs["off"][1])      # semantic unguided
    assert not torch.equal(outs["all"][0], outs["off"][0])
    assert [t.shape for t in outs["all"]] == [t.shape for t in outs["off"]]


# ---- 9. off means off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["cached", "graph", "uncached"])
def test_off_launches_what_it_always_launched(dev, route, monkeypatch):
    from open_musiclm_amd import decode, hip
    from open_musiclm_amd import ops as ops_
    model, wrapper = _small(dev)
    cond = _cond(model, 2, dev)
    kw = dict(conditioning_token_ids=cond, max_time_steps=6, sampler_rng="counter", sampler_seed=3, return_logprobs=True,
              **dict(cached=dict(use_cache=True), graph=dict(use_cache=True, use_graph=True), uncached=dict(use_cache=False))[route])
    wrapper.generate(**kw)                                          # anything built on first use is built
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    for mod in (hip, decode, ops_):
        monkeypatch.setattr(mod, "call", spy)
    want, lw = wrapper.generate(**kw)
    base = list(names)
    for off in (None, 1, 1.0):
        del names[:]
        got, lg = wrapper.generate(cond_scale=off, **kw)
        assert torch.equal(got, want) and torch.equal(lg.model, lw.model) and torch.equal(lg.sampled, lw.sampled), off
        assert names == base and "omlm_guide_logits" not in names and "omlm_decode_twin" not in names, off
    sc = wrapper.score(conditioning_token_ids=cond, pred_token_ids=want)
    del names[:]
    assert torch.equal(wrapper.score(conditioning_token_ids=cond, pred_token_ids=want, cond_scale=1), sc) and "omlm_guide_logits" not in names
    del names[:]
    on = wrapper.generate(cond_scale=3, **kw)[0]
    n_new = 18                                                       # one combine per id; one twin copy per id that is decoded (cached route)
    if route != "graph":                                             # (a captured cycle is recorded once and replayed)
        assert names.count("omlm_guide_logits") == n_new and names.count("omlm_decode_twin") == (n_new - 1 if route == "cached" else 0)
    assert "omlm_guide_logits" in names and (route == "uncached") == ("omlm_decode_twin" not in names)
    assert not torch.equal(on, want)
