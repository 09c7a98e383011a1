"""CPU: the host side of the weight EMA (open_musiclm_amd/ema.py, optimizer.py, config.py) -- the decay schedule against its closed
form, every refusal by its text, the settings as FusedAdam / get_optimizer report them (no flatten on the CPU), and the trainer
config's defaults."""
import json
import math

import numpy as np
import pytest
import torch

import optim_ema_ref as R


def _closed_form(t, decay, after, warmup):
    n = t - after
    if n <= 0:
        return 0.0
    d = float(np.float32(decay))
    return float(np.float32(min(d, (1.0 + n) / (10.0 + n)) if warmup else d))


def test_ema_decay_at_matches_the_closed_form():
    from open_musiclm_amd.ema import ema_decay_at
    decay, after = 0.999, 7
    d32 = float(np.float32(decay))
    # t <= update_after_step: the EMA follows the weights
    for t in (1, 6, 7):
        assert ema_decay_at(t, decay, after, True) == 0.0 and ema_decay_at(t, decay, after, False) == 0.0
    # the first warm-up steps: (1 + n) / (10 + n) = 2/11, 3/12, 4/13
    for n, q in ((1, 2.0 / 11.0), (2, 3.0 / 12.0), (3, 4.0 / 13.0)):
        assert ema_decay_at(after + n, decay, after, True) == float(np.float32(q))
    # the step where (1 + n) / (10 + n) crosses decay: the smallest such n from the inequality 9 / (10 + n) <= 1 - decay
    n_x = math.ceil(9.0 / (1.0 - d32) - 10.0)
    assert (1.0 + n_x) / (10.0 + n_x) >= d32 > n_x / (9.0 + n_x) and 8900 < n_x < 9100
    assert ema_decay_at(after + n_x - 1, decay, after, True) == float(np.float32(n_x / (9.0 + n_x))) <= d32
    assert ema_decay_at(after + n_x, decay, after, True) == d32
    # far beyond, and without the warm-up
    assert ema_decay_at(after + 10 ** 7, decay, after, True) == d32
    assert ema_decay_at(after + 1, decay, after, False) == d32
    # a sweep against the closed form, the numpy restatement of the tests included
    for warmup in (True, False):
        for t in list(range(1, 40)) + [100, 5000, after + n_x - 1, after + n_x, after + n_x + 1, 10 ** 6]:
            for dec, aft in ((decay, after), (0.9, 0), (0.5, 2), (0.0, 0)):
                want = _closed_form(t, dec, aft, warmup)
                assert ema_decay_at(t, dec, aft, warmup) == want == R.decay_at(t, dec, aft, warmup), (t, dec, aft, warmup)


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-12, "x"])
def test_ema_decay_outside_the_unit_interval_is_refused_by_name(decay):
    from open_musiclm_amd.ema import check_ema_settings, ema_decay_at
    from open_musiclm_amd.optimizer import FusedAdam, get_optimizer
    p = [torch.nn.Parameter(torch.zeros(3, 3))]
    for call in (lambda: check_ema_settings(decay), lambda: ema_decay_at(3, decay), lambda: get_optimizer(p, ema_decay=decay),
                 lambda: FusedAdam([{"params": p}], ema_decay=decay)):
        with pytest.raises(ValueError, match=r"ema_decay must be a number in \[0, 1\)"):
            call()


@pytest.mark.parametrize("after", [-1, -100, 2.5])
def test_negative_ema_update_after_step_is_refused_by_name(after):
    from open_musiclm_amd.ema import check_ema_settings
    from open_musiclm_amd.optimizer import get_optimizer
    p = [torch.nn.Parameter(torch.zeros(3, 3))]
    for call in (lambda: check_ema_settings(0.9, after), lambda: get_optimizer(p, ema_decay=0.9, ema_update_after_step=after)):
        with pytest.raises(ValueError, match=r"ema_update_after_step must be an integer >= 0"):
            call()


def test_get_optimizer_reports_the_ema_settings_without_flattening():
    from open_musiclm_amd.optimizer import FusedAdam, get_optimizer
    params = [torch.nn.Parameter(torch.randn(4, 5)), torch.nn.Parameter(torch.randn(7))]
    opt = get_optimizer(params, ema_decay=0.999)
    assert isinstance(opt, FusedAdam) and opt.ema_enabled
    assert opt.ema_settings == dict(decay=0.999, update_after_step=0, warmup=True)
    assert opt._flat is None                                     # CPU parameters: nothing was flattened
    opt = get_optimizer(params, wd=0, ema_decay=0.5, ema_update_after_step=10, ema_warmup=False, some_other_keyword=1)
    assert opt.ema_settings == dict(decay=0.5, update_after_step=10, warmup=False)
    # without the keyword: off, whatever else **kwargs carries (ignored as before)
    for off in (get_optimizer(params), get_optimizer(params, wd=0, some_other_keyword=1), get_optimizer(params, ema_decay=None)):
        assert not off.ema_enabled and off.ema_settings is None and off._flat is None
        with pytest.raises(ValueError, match="keeps no EMA"):
            off.ema_flat


def test_trainer_config_takes_a_dict_without_the_ema_fields(tmp_path):
    from open_musiclm_amd.config import SingleStageTrainerConfig, load_training_config
    base = dict(folder="x", valid_frac=0.05, lr=3e-4, lr_warmup=0, batch_size=2, grad_accum_every=1, wd=0.0,
                max_grad_norm=0.5, cross_entropy_loss_weights=[0.0, 0.0, 1.0], num_train_steps=10, save_results_every=5,
                save_model_every=5, save_predicted_tokens=False, save_reconstructed_wave=False, use_preprocessed_data=True)
    c = SingleStageTrainerConfig(stage="coarse", **base)
    assert (c.ema_decay, c.ema_update_after_step, c.ema_warmup) == (None, 0, True)
    c = SingleStageTrainerConfig(stage="coarse", **base, ema_decay=0.9999, ema_update_after_step=100, ema_warmup=False)
    assert (c.ema_decay, c.ema_update_after_step, c.ema_warmup) == (0.9999, 100, False)
    # a training config file in the reference's layout (none of the new fields) still parses; one stage may switch the EMA on
    train_json = dict(
        clap_rvq_trainer_cfg=dict(folder="x", num_train_steps=1, batch_size=2, accumulate_batches=1, save_model_every=1, save_results_every=1),
        hubert_kmeans_trainer_cfg=dict(folder="x", feature_extraction_num_steps=1, feature_extraction_batch_size=1),
        semantic_trainer_cfg=dict(stage="semantic", **{**base, "cross_entropy_loss_weights": [0.0, 1.0]}),
        coarse_trainer_cfg=dict(stage="coarse", **base), fine_trainer_cfg=dict(stage="fine", **base, ema_decay=0.999),
        data_preprocessor_cfg={})
    (tmp_path / "t.json").write_text(json.dumps(train_json))
    tc = load_training_config(str(tmp_path / "t.json"))
    assert tc.semantic_trainer_cfg.ema_decay is None and tc.coarse_trainer_cfg.ema_decay is None
    assert (tc.fine_trainer_cfg.ema_decay, tc.fine_trainer_cfg.ema_update_after_step, tc.fine_trainer_cfg.ema_warmup) == (0.999, 0, True)
