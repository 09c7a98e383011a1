"""CPU: the per-quantizer metrics of the cross entropy -- the fp64 restatement (tests/ce_metrics_ref.py) against torch, the declarations of the
two entry points, their refusals and null-pointer behaviour through ctypes (nothing is launched: no GPU needed), the route choice, the
arithmetic of QuantizerMetrics and the defaults that keep today's runs what they are."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_musiclm_amd", "csrc")
INF = float("inf")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _tie_inputs(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, V, generator=g, dtype=torch.float64) * 1.5).round().clamp(-3, 3)      # integers in [-3, 3]: rows full of exact ties
    labels = torch.randint(0, V, (R,), generator=g)
    labels[0::4] = torch.argmax(x, 1)[0::4]                                       # the first maximum: rank 0
    last = V - 1 - torch.argmax(x.flip(1), 1)
    labels[2::8] = last[2::8]                                                     # the last of the tied maxima: not rank 0 where there is a tie
    labels[1::5] = -1
    return x, labels


@pytest.mark.parametrize("V", [1, 2, 7, 65, 1025])
def test_rank_zero_iff_argmax_on_ties(V):
    x, labels = _tie_inputs(64, V, seed=V)
    _, rank, _ = MR.rows(x.numpy(), labels.numpy())
    am = torch.argmax(x, 1)
    live = labels >= 0
    assert bool(((torch.from_numpy(rank) == 0) == (am == labels))[live].all())
    assert bool((torch.from_numpy(rank)[~live] == -1).all())
    # the rank is the label's position in a stable descending sort
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for r in range(64):
        if live[r]:
            assert int((order[r] == labels[r]).nonzero()) == rank[r]
    if V >= 7:
        assert int((rank[live.numpy()] > 0).sum()) > 0 and int((rank[live.numpy()] == 0).sum()) > 0


@pytest.mark.parametrize("V", [1, 2, 41, 1025])
def test_nll_and_entropy_against_torch(V):
    g = torch.Generator().manual_seed(V + 3)
    x = torch.randn(23, V, generator=g, dtype=torch.float64) * 3
    x[1] *= 10
    x[2] += 1e4
    labels = torch.randint(0, V, (23,), generator=g)
    labels[5::7] = -1
    nll, rank, ent = MR.rows(x.numpy(), labels.numpy())
    live = (labels >= 0).numpy()
    want = F.cross_entropy(x, labels, ignore_index=-1, reduction="none").numpy()
    assert np.abs(nll - want)[live].max() <= 1e-12 * max(1.0, np.abs(x.numpy()).max())
    lp = torch.log_softmax(x, 1)
    h = -(lp.exp() * lp).sum(1).numpy()
    assert np.abs(ent - h)[live].max() <= 1e-12 * max(1.0, math.log(V + 1))
    assert (nll[~live] == 0).all() and (ent[~live] == 0).all() and (rank[~live] == -1).all()


def test_minus_inf_columns_add_exactly_zero():
    x = np.array([[0.5, -INF, 1.5, -INF, 0.5], [-INF, 2.0, -INF, -INF, -INF], [1.0, 2.0, 3.0, -INF, 0.0]])
    labels = np.array([2, 1, 3])
    nll, rank, ent = MR.rows(x, labels)
    fin = np.array([0.5, 1.5, 0.5])
    p = np.exp(fin - fin.max()); p /= p.sum()
    assert abs(ent[0] - float(-(p * np.log(p)).sum())) <= 1e-15 and np.isfinite(ent).all()
    assert ent[1] == 0.0 and nll[1] == 0.0 and rank[1] == 0                       # one live column: a point mass
    assert nll[2] == INF and rank[2] == 4                                         # the label on a -inf column: the rank stays exact
    # labels past the vocabulary: treated like ignored rows
    assert MR.rows(x, np.array([5, 9, -1]))[1].tolist() == [-1, -1, -1]


def test_bin_rule():
    # B = 2, n = 7 = 2 * 3 + 1, Q = 3, V = 5 (eos = 4)
    labels = np.array([0, 1, 4, 2, -1, 3, 4,   4, 0, 1, 2, 3, 9, 0])
    nll = np.arange(14, dtype=float) + 1
    ent = nll * 0.5
    rank = np.array([0, 1, 0, 2, -1, 0, 3,   0, 0, 4, 1, 0, -1, 2])
    b = MR.bins(nll, rank, ent, labels, 7, 3, 5, 2)
    assert b[:, 0].tolist() == [4, 3, 2, 3]                                       # t mod 3 of the live non-eos rows; 3 eos rows wherever they stand
    assert b[3].tolist() == [3, 3 + 7 + 8, 0.5 * (3 + 7 + 8), 2, 2]
    assert b[0].tolist() == [4, 1 + 4 + 11 + 14, 0.5 * (1 + 4 + 11 + 14), 1, 2]
    assert b[:, 0].sum() == 12                                                    # row 4 (ignored) and row 12 (label >= V) enter no bin


# ---- declarations ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_after_the_cross_entropy_pair_and_bound():
    from open_musiclm_amd import hip
    hdr = open(os.path.join(ROOT, "include", "omlm.h")).read()
    m = re.search(r"int omlm_ce_metrics\(([^)]*)\);", hdr)
    b = re.search(r"int omlm_ce_metrics_bins\(([^)]*)\);", hdr)
    assert m and b
    assert re.sub(r"\s+", " ", m.group(1)) == ("const float* logits, const int* labels, float* row_nll, int* row_rank, float* row_entropy, "
                                                "int R, int V, int ld, int* err_flag, void* stream")
    assert re.sub(r"\s+", " ", b.group(1)) == ("const float* row_nll, const int* row_rank, const float* row_entropy, const int* labels, "
                                                "int R, int n, int Q, int V, int k_top, double* bins, void* stream")
    assert len(hip.SIGNATURES["omlm_ce_metrics"]) == m.group(1).count(",") + 1 == 10
    assert len(hip.SIGNATURES["omlm_ce_metrics_bins"]) == b.group(1).count(",") + 1 == 11
    assert hdr.index("int omlm_ce_metrics(") > hdr.index("int omlm_cross_entropy_bwd_reg(")
    rule = hdr[hdr.index("int omlm_cross_entropy_bwd_reg("):hdr.index("int omlm_ce_metrics(")]
    for word in ("#{c : l[c] > l[y]} + #{c < y : l[c] == l[y]}", "log s - (sum_c e_c d_c) / s", "adds exactly 0", "err_flag |= 4", "ACCUMULATED",
                 "t mod Q", "y == V - 1", "fixed order", "translation unit of"):
        assert word in rule, word
    src = open(os.path.join(CSRC, "ce_metrics.hip")).read()
    for name in ("omlm_ce_metrics", "omlm_ce_metrics_bins"):
        assert f'extern "C" int {name}(' in src
    assert "ce_metrics" not in open(os.path.join(CSRC, "embed_ce.hip")).read()              # the four cross-entropy kernels: untouched


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    from open_musiclm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        G.build()
    return hip.lib()


def test_nothing_to_do_and_null_pointers(lib):
    assert lib.omlm_ce_metrics(None, None, None, None, None, 0, 5, 8, None, None) == 0
    assert lib.omlm_ce_metrics_bins(None, None, None, None, 0, 7, 3, 5, 2, None, None) == 0
    assert lib.omlm_ce_metrics(None, None, None, None, None, 1, 5, 8, None, None) != 0
    assert b"null pointer" in lib.omlm_last_error() and b"ce_metrics" in lib.omlm_last_error()
    assert lib.omlm_ce_metrics_bins(None, None, None, None, 7, 7, 3, 5, 2, None, None) != 0
    assert b"null pointer" in lib.omlm_last_error() and b"ce_metrics_bins" in lib.omlm_last_error()


@pytest.mark.parametrize("args,word", [((-1, 5, 8), b"R must be >= 0"), ((0, 0, 8), b"V must be >= 1"), ((0, 5, 4), b"ld must be >= V"),
                                        ((3, -2, 8), b"V must be >= 1")])
def test_ce_metrics_refusals_by_name(lib, args, word):
    assert lib.omlm_ce_metrics(None, None, None, None, None, *args, None, None) == -1
    assert word in lib.omlm_last_error(), lib.omlm_last_error()


@pytest.mark.parametrize("args,word", [((-7, 7, 3, 5, 2), b"R must be >= 0"), ((0, 7, 3, 0, 1), b"V must be >= 1"), ((0, 0, 3, 5, 2), b"n must be >= 1"),
                                        ((8, 7, 3, 5, 2), b"R must be a multiple of n"), ((0, 7, 0, 5, 2), b"Q must be >= 1"),
                                        ((0, 7, 3, 5, 0), b"k_top must lie in [1, V]"), ((0, 7, 3, 5, 6), b"k_top must lie in [1, V]")])
def test_ce_metrics_bins_refusals_by_name(lib, args, word):
    assert lib.omlm_ce_metrics_bins(None, None, None, None, *args, None, None) == -1
    assert word in lib.omlm_last_error(), lib.omlm_last_error()


def test_route_is_a_function_of_the_row_width(tmp_path):
    """csrc/ce_metrics_plan.h built with the host c++: one wave per row up to 64 lanes x 17 registers, one workgroup per row above."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path / "libce_metrics_plan.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DOMLM_PLAN_TEST_ABI", "-I", CSRC, "-x", "c++", "-", "-o", so],
                   input=b'#include "ce_metrics_plan.h"\n', check=True)
    plan = C.CDLL(so)
    WAVE, BLOCK = 0, 1
    assert [plan.omlm_plan_ce_metrics_route(V) for V in (1, 2, 64, 65, 1025, 1088)] == [WAVE] * 6
    assert [plan.omlm_plan_ce_metrics_route(V) for V in (1089, 2049, 8193, 1 << 20)] == [BLOCK] * 4
    # four rows per workgroup on the wave route, one on the other; both capped (further rows in trips)
    assert [plan.omlm_plan_ce_metrics_grid(R, 1088) for R in (1, 4, 5, 257, 1 << 20)] == [1, 1, 2, 65, 1024]
    assert [plan.omlm_plan_ce_metrics_grid(R, 1089) for R in (1, 5, 257, 1 << 20)] == [1, 5, 257, 4096]
    # the same threshold as the loss's own forward (CE_NV of csrc/embed_ce.hip)
    ce_nv = int(re.search(r"#define CE_NV (\d+)", open(os.path.join(CSRC, "embed_ce.hip")).read()).group(1))
    nv = int(re.search(r"#define CE_METRICS_NV (\d+)", open(os.path.join(CSRC, "ce_metrics_plan.h")).read()).group(1))
    assert ce_nv == nv == 17


# ---- QuantizerMetrics --------------------------------------------------------------------------------------------------------------
def test_top_k_default_and_refusals():
    from open_musiclm_amd import ops
    assert ops.default_metrics_top_k(1025) == 102 == ops.check_metrics_top_k(None, 1025)
    assert ops.default_metrics_top_k(1025) == max(int((1 - 0.9) * 1025), 1)                  # utils.top_k's expression at filter_thres = 0.9
    assert ops.default_metrics_top_k(5) == 1 and ops.default_metrics_top_k(2049) == 204
    assert ops.check_metrics_top_k(1, 1025) == 1 and ops.check_metrics_top_k(1025, 1025) == 1025
    for bad in (0, -1, 1026, 1.5, "3", True):
        with pytest.raises(ValueError, match="metrics_top_k"):
            ops.check_metrics_top_k(bad, 1025)
    with pytest.raises(ValueError, match="k_top"):
        ops.check_metrics_top_k(0, 5, "k_top")


def test_quantizer_metrics_arithmetic_on_the_host():
    from open_musiclm_amd.metrics import QuantizerMetrics
    m = QuantizerMetrics([12, 1, 3], [33, 49, 41], [0., 0., 1.], top_k=5)
    assert m.bins.dtype == torch.float64 and tuple(m.bins.shape) == (3, 13, 5) and m.k_top == [3, 4, 5] and m.weighted == [2]
    assert m.loss() is None
    m.bins[2, 0] = torch.tensor([4., 6., 2., 1., 3.])
    m.bins[2, 1] = torch.tensor([4., 10., 4., 2., 4.])
    m.bins[2, 3] = torch.tensor([2., 1., 0.5, 2., 2.])                            # eos bin; quantizer 2 stays empty
    m.bins[0, 0] = 7.0                                                            # an unweighted sequence is not reported
    d = m.to_dict("train_")
    assert d["train_loss_q0"] == 1.5 and d["train_accuracy_q0"] == 0.25 and d["train_top5_accuracy_q0"] == 0.75 and d["train_entropy_q0"] == 0.5
    assert d["train_count_q0"] == 4.0 and d["train_loss_q1"] == 2.5 and d["train_accuracy_q1"] == 0.5
    assert d["train_loss_q2"] is None and d["train_accuracy_q2"] is None and d["train_top5_accuracy_q2"] is None and d["train_entropy_q2"] is None
    assert d["train_count_q2"] == 0.0
    assert d["train_loss_eos"] == 0.5 and d["train_accuracy_eos"] == 1.0 and d["train_count_eos"] == 2.0
    assert d["train_loss_total"] == 1.7 and d["train_accuracy_total"] == 0.5 and d["train_count_total"] == 10.0 and d["train_top5_accuracy_total"] == 0.9
    assert all(isinstance(v, float) or v is None for v in d.values()) and not any("seq" in k for k in d)
    assert len(d) == 5 * 5
    assert m.loss() == 1.7
    other = m.like()
    assert float(other.bins.abs().sum()) == 0 and other.same_layout(m)
    other.bins[2, 2] = torch.tensor([1., 3., 1., 0., 0.])
    m.add_(other)
    assert m.to_dict()["loss_q2"] == 3.0 and m.loss() == 20.0 / 11.0
    assert m.zero_() is m and float(m.bins.abs().sum()) == 0 and m.loss() is None
    with pytest.raises(ValueError, match="add_"):
        m.add_(QuantizerMetrics([12, 1, 3], [33, 49, 41], [0., 0., 1.], top_k=6))
    with pytest.raises(ValueError, match="metrics_top_k"):
        QuantizerMetrics([3], [41], [1.], top_k=42)
    # several weighted sequences: the names carry the sequence index, the loss the weights
    m2 = QuantizerMetrics([2, 1], [9, 17], [0.5, 1.0])
    m2.bins[0, 0] = torch.tensor([2., 4., 1., 1., 1.])
    m2.bins[1, 0] = torch.tensor([2., 6., 1., 0., 1.])
    d2 = m2.to_dict("valid_")
    assert d2["valid_seq0_loss_q0"] == 2.0 and d2["valid_seq1_loss_q0"] == 3.0 and d2["valid_seq0_loss_q1"] is None
    assert f"valid_seq1_top{m2.k_top[1]}_accuracy_q0" in d2 and m2.k_top == [1, 1]
    assert m2.loss() == (0.5 * 4 + 6) / 4


def _tiny():
    from open_musiclm_amd import open_musiclm as M
    torch.manual_seed(0)
    return M.create_coarse_transformer(dim=64, depth=1, heads=1, num_coarse_quantizers=2, clap_codebook_size=16, semantic_codebook_size=16,
                                       acoustic_codebook_size=16, num_clap_quantizers=3, ff_dropout=0.0)


def test_wrapper_surface_and_refusals():
    from open_musiclm_amd import open_musiclm as M
    from open_musiclm_amd.metrics import QuantizerMetrics
    prm = inspect.signature(M.TokenConditionedTransformerWrapper.forward).parameters
    assert prm["return_metrics"].default is False
    assert inspect.signature(M.TokenConditionedTransformer.loss_and_logits).parameters["metrics"].default is None
    w = M.TokenConditionedTransformerWrapper(transformer=_tiny(), cross_entropy_loss_weights=[0., 0., 1.])
    m = w.new_metrics()
    assert isinstance(m, QuantizerMetrics) and m.quantizers == [3, 1, 2] and m.vocab == [17, 17, 17] and m.k_top == [1, 1, 1]
    assert w.new_metrics(top_k=4).k_top == [1, 1, 4]
    ids = [torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, 2, dtype=torch.long)]
    with pytest.raises(ValueError, match="return_metrics"):
        w(all_token_ids=ids, return_loss=False, return_metrics=True)              # before any device work
    with pytest.raises(ValueError, match="return_metrics"):
        w(all_token_ids=ids, return_loss=True, return_metrics="yes")
    with pytest.raises(ValueError, match="return_metrics"):
        w(all_token_ids=ids, return_loss=True, return_metrics=QuantizerMetrics([3, 1, 2], [17, 17, 17], [1., 0., 1.]))


BASE = dict(stage="coarse", folder="x", valid_frac=0.05, lr=3e-4, lr_warmup=0, batch_size=2, grad_accum_every=1, wd=0.0, max_grad_norm=0.5,
            cross_entropy_loss_weights=[0., 0., 1.], num_train_steps=3, save_results_every=1, save_model_every=1, save_predicted_tokens=False,
            save_reconstructed_wave=False, use_preprocessed_data=False)


def test_trainer_and_config_defaults_and_round_trip():
    from dataclasses import asdict
    from open_musiclm_amd.config import SingleStageTrainerConfig
    from open_musiclm_amd.trainer import SingleStageTrainer
    prm = inspect.signature(SingleStageTrainer.__init__).parameters
    assert prm["quantizer_metrics"].default is False and prm["metrics_top_k"].default is None and prm["valid_batches"].default == 1
    fields = SingleStageTrainerConfig.__dataclass_fields__
    assert fields["quantizer_metrics"].default is False and fields["metrics_top_k"].default is None and fields["valid_batches"].default == 1
    d = asdict(SingleStageTrainerConfig(**BASE))
    assert (d["quantizer_metrics"], d["metrics_top_k"], d["valid_batches"]) == (False, None, 1)
    assert set(d) - {"stage"} <= set(prm)                                         # create_single_stage_trainer_from_config hands every field on
    cfg = SingleStageTrainerConfig(**BASE, quantizer_metrics=True, metrics_top_k=10, valid_batches=4)
    again = SingleStageTrainerConfig(**asdict(cfg))
    assert again == cfg and (again.quantizer_metrics, again.metrics_top_k, again.valid_batches) == (True, 10, 4)


class _Tokens(torch.utils.data.Dataset):
    def __len__(self):
        return 8

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(i)
        return tuple(torch.randint(0, 16, s, generator=g) for s in ((3,), (2,), (2, 2)))


@pytest.mark.parametrize("kw,word", [(dict(valid_batches=0), "valid_batches"), (dict(valid_batches=-2, quantizer_metrics=True), "valid_batches"),
                                     (dict(valid_batches=1.5, quantizer_metrics=True), "valid_batches"),
                                     (dict(valid_batches=2), "quantizer_metrics"), (dict(quantizer_metrics=True, metrics_top_k=18), "metrics_top_k"),
                                     (dict(quantizer_metrics=True, metrics_top_k=0), "metrics_top_k")])
def test_trainer_refuses_by_name(tmp_path, kw, word):
    from open_musiclm_amd.trainer import SingleStageTrainer
    with pytest.raises(ValueError, match=word):
        SingleStageTrainer(_tiny(), "coarse", num_train_steps=1, batch_size=2, dataset=_Tokens(), results_folder=str(tmp_path / "r"),
                           save_predicted_tokens=False, save_reconstructed_wave=False, **kw)
