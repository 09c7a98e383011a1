"""CPU: label smoothing and z-loss in the fused cross entropy -- the fp64 restatement (tests/ce_reg_ref.py) against torch, the refusals
that come before any device work, the declarations of the two new entry points and the defaults that keep today's runs what they are."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import ce_reg_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _inputs(V, seed, R=23):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g, dtype=torch.float64) * 3
    x[1] *= 10
    x[2, int(torch.randint(0, V, (1,), generator=g))] += 40
    x[3] = 0.75
    labels = torch.randint(0, V, (R,), generator=g)
    labels[0], labels[4] = 0, V - 1
    labels[5::7] = -1                                            # ignored rows
    return x, labels


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 41, 1025])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.9])
def test_restatement_against_torch_label_smoothing(V, eps):
    x, labels = _inputs(V, seed=V * 7 + 1)
    want = float(F.cross_entropy(x, labels, label_smoothing=eps, ignore_index=-1, reduction="sum"))
    got = CR.loss_sum(x, labels, eps, 0.0)
    assert _rel(got, want) <= 1e-12, (got, want)


@pytest.mark.parametrize("V", [1, 2, 41, 1025])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.9])
@pytest.mark.parametrize("zeta", [0.0, 1e-4, 1e-2])
def test_restatement_against_autograd(V, eps, zeta):
    x, labels = _inputs(V, seed=V * 13 + 5)
    live = labels >= 0
    xl = x.clone().requires_grad_(True)
    lse = torch.logsumexp(xl, 1)
    own = xl.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    rows = (1 - eps) * (lse - own) + eps * (lse - xl.mean(1)) + zeta * lse * lse
    loss = rows[live].sum()
    loss.backward()
    got = CR.loss_sum(x, labels, eps, zeta)
    assert _rel(got, float(loss.detach())) <= 1e-12, (got, float(loss.detach()))
    g = CR.grad(x, labels, eps, zeta)
    # per element: 1e-12 of the gradient's own scale |p (1 + 2 zeta lse)| + 1 <= 2 + 2 zeta max|lse|
    scale = 2.0 + 2.0 * zeta * float(lse.detach().abs().max())
    assert float((g - xl.grad).abs().max()) <= 1e-12 * scale
    assert bool((g[~live] == 0).all()) and bool((xl.grad[~live] == 0).all())
    if eps == 0.0 and zeta == 0.0:                               # the plain rule
        p = torch.softmax(x, 1)
        p[torch.arange(len(labels))[live], labels[live]] -= 1
        p[~live] = 0
        assert float((g - p).abs().max()) <= 1e-12


def test_restatement_ignores_labels_past_the_vocabulary_and_takes_a_given_lse():
    x, labels = _inputs(41, seed=3)
    labels[2] = 41
    n, s, z = CR.sums(x, labels)
    keep = (labels >= 0) & (labels < 41)
    n2, s2, z2 = CR.sums(x[keep], labels[keep])
    assert max(_rel(a, b) for a, b in zip((n, s, z), (n2, s2, z2))) <= 1e-14             # (the order of the sum)
    assert bool((CR.grad(x, labels, 0.1, 1e-2)[2] == 0).all())
    lse = torch.logsumexp(x, 1)
    assert torch.equal(CR.grad(x, labels, 0.1, 1e-2), CR.grad(x, labels, 0.1, 1e-2, lse=lse))
    assert not torch.equal(CR.grad(x, labels, 0.1, 1e-2), CR.grad(x, labels, 0.1, 1e-2, lse=lse + 1e-3))


# ---- the expected values of the model-level GPU test (tests/test_gpu_ce_reg.py), from the oracle alone --------------------------------
EPS, ZETA = 0.1, 1e-2                     # the run that is held to the oracle
EPS_SEEN = 0.5                            # the run in which the smoothing term is seen on the logit-head gradient (below)
HEAD = "logit_weights.2"
_ORACLE = {}


def oracle_regularised(golden_dir):
    """The oracle's logits of the tiny_coarse golden (forgetful mask off), the regularised loss formed from them in fp64 on the CPU and
    backpropagated through the oracle: {(eps, zeta): (loss, {parameter: gradient})} for the full rule at both eps and for each term
    left out.  Made once per process."""
    import numpy as np
    from oracle import musiclm_oracle as O
    if _ORACLE:
        return _ORACLE
    z = np.load(os.path.join(golden_dir, "tiny_coarse.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    spec = O.ModelSpec([O.SeqInfo(32, 12), O.SeqInfo(48, 1), O.SeqInfo(40, 3)], dim=128, depth=2, heads=2)
    ids = [torch.from_numpy(z[f"ids.{i}"]) for i in range(3)]
    sdo = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    _, logits, labels = O.wrapper_forward_loss(sdo, spec, ids, [0., 0., 1.])
    lg = logits[-1].transpose(1, 2).reshape(-1, logits[-1].shape[1]).double()
    lb = labels[-1].reshape(-1)
    lse = torch.logsumexp(lg, 1)
    nll, smooth, zz = lse - lg.gather(1, lb[:, None])[:, 0], lse - lg.mean(1), lse * lse
    names = [k for k, v in sdo.items() if v.requires_grad]
    for eps, zeta in ((EPS, ZETA), (EPS, 0.0), (0.0, ZETA), (EPS_SEEN, ZETA), (EPS_SEEN, 0.0)):
        loss = ((1 - eps) * nll + eps * smooth + zeta * zz).sum() / lb.numel()
        gr = torch.autograd.grad(loss, [sdo[k] for k in names], allow_unused=True, retain_graph=True)
        _ORACLE[eps, zeta] = (float(loss.detach()), {k: g.detach() for k, g in zip(names, gr) if g is not None})
    return _ORACLE


def test_each_term_is_visible_to_the_oracle(golden_dir):
    """A precondition of test_regularised_training_step_matches_the_oracle (GPU), checked on the expected values alone: no project code
    runs here.  Left out of the expected loss, the z term misses by 25 % and the smoothing term by 2.3 % at eps = 0.1 (this golden's
    logits are far from uniform: max lse 38): more than 10x the loss bars (<= 1e-4).  On the logit-head weight gradient the expected
    value without smoothing misses the full one by 6.7e-2 of the tensor's largest entry at eps = 0.1 -- under 10x the gradient bars
    (1.5e-2 bf16x3, 1e-2 fp16ff) -- and, the miss being linear in eps, by 0.34 at eps = 0.5, which clears 10x both; so the GPU test
    holds the eps = 0.1 run to the oracle and sees the smoothing term on the gradient in a second run at eps = 0.5."""
    from test_gpu_model import TOL
    o = oracle_regularised(golden_dir)
    loss_bar = max(TOL[p]["loss"] for p in ("bf16x3", "fp16ff"))
    grad_bar = max(TOL[p]["grad"] for p in ("bf16x3", "fp16ff"))
    no_eps = o[0.0, ZETA]
    miss = {}
    for eps in (EPS, EPS_SEEN):
        full, no_z = o[eps, ZETA], o[eps, 0.0]
        assert abs(no_z[0] - full[0]) > 10 * loss_bar * full[0], eps
        assert abs(no_eps[0] - full[0]) > 10 * loss_bar * full[0], eps
        gscale = max(float(v.abs().max()) for v in full[1].values())
        miss[eps] = float((no_eps[1][HEAD] - full[1][HEAD]).abs().max() / max(float(full[1][HEAD].abs().max()), 1e-3 * gscale))
    print(f"oracle alone: head gradient miss without smoothing {miss}")
    assert miss[EPS_SEEN] > 10 * grad_bar, miss
    assert abs(miss[EPS_SEEN] / miss[EPS] - EPS_SEEN / EPS) < 1.0, miss          # linear in eps up to the tensor's own scale


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_checks_return_good_values_unchanged():
    from open_musiclm_amd import ops
    for v in (0, 0.0, 0.1, 0.9, 0.999999):
        assert ops.check_label_smoothing(v) == float(v) and isinstance(ops.check_label_smoothing(v), float)
    for v in (0, 0.0, 1e-4, 1e-2, 3.0):
        assert ops.check_z_loss(v) == float(v) and isinstance(ops.check_z_loss(v), float)


@pytest.mark.parametrize("bad", [-0.1, 1, NAN, INF, "x"])
def test_bad_label_smoothing_is_refused_by_name(bad):
    from open_musiclm_amd import ops
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.check_label_smoothing(bad)
    with pytest.raises(ValueError, match="eps"):
        ops.check_label_smoothing(bad, "eps")


@pytest.mark.parametrize("bad", [-1e-4, NAN, INF, "x"])
def test_bad_z_loss_is_refused_by_name(bad):
    from open_musiclm_amd import ops
    with pytest.raises(ValueError, match="z_loss"):
        ops.check_z_loss(bad)
    with pytest.raises(ValueError, match="zeta"):
        ops.check_z_loss(bad, "zeta")


def _tiny():
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_coarse_transformer(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                                       acoustic_codebook_size=16, num_clap_quantizers=3, ff_dropout=0.0)


def test_wrapper_and_stages_refuse_bad_values_by_name():
    from open_musiclm_amd import open_musiclm as M
    model = _tiny()
    for bad in (-0.1, 1, NAN, "x"):
        with pytest.raises(ValueError, match="label_smoothing"):
            M.TokenConditionedTransformerWrapper(transformer=model, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            M.CoarseStage(coarse_transformer=model, label_smoothing=bad)
    for bad in (-1e-4, INF, "x"):
        with pytest.raises(ValueError, match="z_loss"):
            M.TokenConditionedTransformerWrapper(transformer=model, z_loss=bad)
        with pytest.raises(ValueError, match="z_loss"):
            M.FineStage(fine_transformer=model, z_loss=bad)
    with pytest.raises(ValueError, match="z_loss"):
        model.loss_and_logits([], [], None, [1.0], z_loss=-1.0)              # before any device work


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_keywords_exist_with_default_zero_and_travel():
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd import ops
    from open_musiclm_amd.config import SingleStageTrainerConfig
    from open_musiclm_amd.trainer import SingleStageTrainer
    for cls in (M.TokenConditionedTransformerWrapper, M.SemanticStage, M.CoarseStage, M.FineStage, SingleStageTrainer):
        prm = inspect.signature(cls.__init__).parameters
        assert prm["label_smoothing"].default == 0.0 and prm["z_loss"].default == 0.0, cls
    for fn in (M.TokenConditionedTransformer.loss_and_logits, ops.ce_fwd, ops.ce_bwd):
        prm = inspect.signature(fn).parameters
        assert prm["label_smoothing"].default == 0.0 and prm["z_loss"].default == 0.0, fn
    fields = SingleStageTrainerConfig.__dataclass_fields__
    assert fields["label_smoothing"].default == 0.0 and fields["z_loss"].default == 0.0
    model = _tiny()
    w = M.TokenConditionedTransformerWrapper(transformer=model)
    assert (w.label_smoothing, w.z_loss) == (0.0, 0.0)
    w = M.TokenConditionedTransformerWrapper(transformer=model, label_smoothing=0.1, z_loss=1e-2)
    assert (w.label_smoothing, w.z_loss) == (0.1, 1e-2)
    assert w.train()._loss_reg() == dict(label_smoothing=0.1, z_loss=1e-2) and w.eval()._loss_reg() == {}       # training mode only
    sem = M.create_semantic_transformer(dim=64, depth=1, heads=1, clap_codebook_size=16, semantic_codebook_size=16, num_clap_quantizers=3)
    for stage in (M.CoarseStage(coarse_transformer=model, label_smoothing=0.2, z_loss=1e-3),
                  M.FineStage(fine_transformer=model, label_smoothing=0.2, z_loss=1e-3),
                  M.SemanticStage(semantic_transformer=sem, label_smoothing=0.2, z_loss=1e-3)):
        assert (stage.transformer_wrapper.label_smoothing, stage.transformer_wrapper.z_loss) == (0.2, 1e-3)
    assert M.CoarseStage(coarse_transformer=model).transformer_wrapper.z_loss == 0.0


def test_trainer_config_round_trips_the_two_fields():
    from dataclasses import asdict
    from open_musiclm_amd.config import SingleStageTrainerConfig
    base = dict(stage="coarse", folder="x", valid_frac=0.05, lr=3e-4, lr_warmup=0, batch_size=2, grad_accum_every=1, wd=0.0, max_grad_norm=0.5,
                cross_entropy_loss_weights=[0., 0., 1.], num_train_steps=3, save_results_every=1, save_model_every=1, save_predicted_tokens=False,
                save_reconstructed_wave=False, use_preprocessed_data=False)
    d = asdict(SingleStageTrainerConfig(**base))
    assert d["label_smoothing"] == 0.0 and d["z_loss"] == 0.0
    cfg = SingleStageTrainerConfig(**base, label_smoothing=0.1, z_loss=1e-4)
    again = SingleStageTrainerConfig(**asdict(cfg))
    assert again == cfg and (again.label_smoothing, again.z_loss) == (0.1, 1e-4)


def test_entry_points_are_declared_and_bound():
    """Fails before the two entries exist."""
    from open_musiclm_amd import hip
    hdr = open(os.path.join(ROOT, "include", "omlm.h")).read()
    src = open(os.path.join(ROOT, "open_musiclm_amd", "csrc", "embed_ce.hip")).read()
    f = re.search(r"int omlm_cross_entropy_fwd_reg\(([^)]*)\);", hdr)
    assert f and re.sub(r"\s+", " ", f.group(1)) == ("const float* logits, const int* labels, float* row_lse, float* sums, int R, int V, int ld, "
                                                      "int* err_flag, void* stream")
    assert len(hip.SIGNATURES["omlm_cross_entropy_fwd_reg"]) == f.group(1).count(",") + 1 == 9
    b = re.search(r"int omlm_cross_entropy_bwd_reg\(([^)]*)\);", hdr)
    assert b and re.sub(r"\s+", " ", b.group(1)).endswith("int ldd, int out_dtype, float label_smoothing, float z_loss, void* stream")
    assert len(hip.SIGNATURES["omlm_cross_entropy_bwd_reg"]) == b.group(1).count(",") + 1 == 14
    assert hip.SIGNATURES["omlm_cross_entropy_bwd_reg"][-3:-1] == [hip.f32, hip.f32]
    # the old pair is what it was
    assert len(hip.SIGNATURES["omlm_cross_entropy_fwd"]) == 9 and len(hip.SIGNATURES["omlm_cross_entropy_bwd"]) == 12
    before = hdr[hdr.index("int omlm_cross_entropy_fwd_reg(") - 2600:hdr.index("int omlm_cross_entropy_fwd_reg(")]
    for word in ("smooth = lse - (1 / V) sum_c l[c]", "z      = lse^2", "(1 - eps) nll + eps smooth + zeta z",
                 "p[c] (1 + 2 zeta lse) - (1 - eps) [c == y] - eps / V", "training mode only", "exact-zero gradients", "ACCUMULATED"):
        assert word in before, word
    for name in ("omlm_cross_entropy_fwd", "omlm_cross_entropy_bwd", "omlm_cross_entropy_fwd_reg", "omlm_cross_entropy_bwd_reg"):
        assert f'extern "C" int {name}(' in src


def test_new_entries_refuse_bad_arguments_without_a_device():
    """The C side: eps outside [0, 1), zeta < 0 and non-finite values are refused by name before anything else is looked at (R = 0 and
    null tensors here: nothing is launched, no GPU needed); good values with R = 0 return at once."""
    import __graft_entry__ as G
    from open_musiclm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        G.build()
    lib = hip.lib()
    tail = (0, 5, 8, 8, 2)                                       # R, V, ld, ldd, out_dtype
    assert lib.omlm_cross_entropy_bwd_reg(None, None, None, None, 1.0, None, *tail, 0.1, 1e-2, None) == 0
    assert lib.omlm_cross_entropy_bwd_reg(None, None, None, None, 1.0, None, *tail, 0.0, 0.0, None) == 0
    for eps in (-0.1, 1.0, NAN, INF, -INF):
        assert lib.omlm_cross_entropy_bwd_reg(None, None, None, None, 1.0, None, *tail, eps, 0.0, None) != 0, eps
        assert b"label_smoothing" in lib.omlm_last_error(), eps
    for zeta in (-1e-4, NAN, INF):
        assert lib.omlm_cross_entropy_bwd_reg(None, None, None, None, 1.0, None, *tail, 0.1, zeta, None) != 0, zeta
        assert b"z_loss" in lib.omlm_last_error(), zeta
    assert lib.omlm_cross_entropy_fwd_reg(None, None, None, None, 0, 5, 8, None, None) == 0
    assert lib.omlm_cross_entropy_fwd_reg(None, None, None, None, 1, 5, 8, None, None) != 0          # null pointers with a row to do
    assert b"cross entropy arguments" in lib.omlm_last_error()
    assert lib.omlm_cross_entropy_bwd_reg(None, None, None, None, 1.0, None, 1, 5, 8, 8, 2, 0.1, 1e-2, None) != 0
    assert b"cross entropy arguments" in lib.omlm_last_error()
