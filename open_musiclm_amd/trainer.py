"""SingleStageTrainer with the reference's constructor / method surface (reference open_musiclm/trainer.py:111-560),
re-hosted on the MI355X engine:

  * no HF accelerate / DDP: one process per GPU (parallel.DataParallel over RCCL); gradients of all
    grad_accum_every micro-batches accumulate in the optimizer's flat buffer and are exchanged with ONE
    SUM all-reduce per optimizer step (the reference all-reduces on every micro-batch backward, :439);
  * clip_grad_norm_ + Adam(W) + zero_grad + LinearLR warm-up are the fused optimizer step (:444-449);
  * the per-micro-batch `loss.item()` host sync of the reference (:441) is replaced by one device-side
    accumulation that is read back once per optimizer step.

Checkpoint files keep the reference's names and formats ({stage}.transformer|optimizer|scheduler.{step}.pt, :536-549)
so scripts/train_utils.py resumes from them unchanged.
"""
from __future__ import annotations

import itertools
import json
import os
import sys
import time
from dataclasses import asdict, is_dataclass
from pathlib import Path
from shutil import rmtree
from typing import List, Optional

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset, random_split

from .data import PreprocessedDataset, SoundDataset, get_dataloader, get_preprocessed_dataloader
from .open_musiclm import (CoarseStage, FineStage, SemanticStage, TokenConditionedTransformer)
from .optimizer import get_linear_scheduler, get_optimizer
from .parallel import DataParallel
from .utils import copy_file_to_folder, default, exists


def cycle(dl, sampler=None):
    epoch = 0
    while True:
        if sampler is not None:                    # DistributedSampler: a new shuffle every pass (else every epoch repeats)
            sampler.set_epoch(epoch)
        for data in dl:
            yield data
        epoch += 1


def _rank_sampler(dp, ds):
    """DistributedSampler over `ds` for this rank, or None in a single process."""
    if not dp.is_distributed:
        return None
    from torch.utils.data.distributed import DistributedSampler
    return DistributedSampler(ds, num_replicas=dp.world_size, rank=dp.rank, shuffle=True)


def _gather_rows(dp, t: torch.Tensor) -> torch.Tensor:
    """all-gather of [rows, d] along dim 0; a gloo group (CPU collectives) gets the tensor on the host and returns it to its device."""
    if not dp.is_distributed:
        return t
    import torch.distributed as dist
    dev = t.device
    if dist.get_backend() == "gloo" and dev.type != "cpu":
        return dp.all_gather_cat(t.cpu().contiguous()).to(dev)
    return dp.all_gather_cat(t.contiguous())


def yes_or_no(question):
    if not sys.stdin or not sys.stdin.isatty():       # non-interactive launch (torchrun, CI): keep existing results
        return False
    answer = input(f'{question} (y/n) ')
    return answer.lower() in ('yes', 'y')


def accum_log(log, new_logs):
    for key, new_value in new_logs.items():
        log[key] = log.get(key, 0.) + new_value
    return log


def noop(*args, **kwargs):
    pass


class _JsonlTracker:
    """Stand-in for accelerate's trackers (tensorboard / wandb are not hot-path): metrics go to a JSONL file."""

    def __init__(self, logging_dir, run_name, config, enabled):
        self.f = None
        if enabled and logging_dir:
            os.makedirs(logging_dir, exist_ok=True)
            self.f = open(os.path.join(logging_dir, f"{run_name}.jsonl"), "a")
            self.f.write(json.dumps({"config": config}, default=str) + "\n")

    def log(self, values, step):
        if self.f:
            self.f.write(json.dumps({"step": step, **values}) + "\n")
            self.f.flush()


class SingleStageTrainer(nn.Module):
    """trainer.py:111-560.  semantic: needs audio_conditioner + wav2vec (or preprocessed / token datasets);
    coarse: + neural_codec; fine: audio_conditioner + neural_codec."""

    def __init__(self, transformer: TokenConditionedTransformer, stage, *, num_train_steps, batch_size,
                 model_config=None, training_config=None, dataset: Optional[Dataset] = None, wav2vec=None,
                 neural_codec=None, audio_conditioner=None, data_max_length_seconds=1,
                 ignore_files: Optional[List[str]] = None, cross_entropy_loss_weights: Optional[List[float]] = None,
                 ignore_load_errors=True, folder=None, use_preprocessed_data=False, lr=3e-4, lr_warmup=0,
                 grad_accum_every=1, wd=0., max_grad_norm=0.5, valid_frac=0.05, random_split_seed=42,
                 save_results_every=100, save_predicted_tokens=True, save_reconstructed_wave=True,
                 save_model_every=1000, results_folder='./results', accelerate_kwargs: dict = {},
                 config_paths: Optional[List[str]] = None, dataset_yields_tokens: Optional[bool] = None,
                 use_hip_graph: Optional[bool] = None, ema_decay: Optional[float] = None, ema_update_after_step: int = 0,
                 ema_warmup: bool = True, null_cond_prob: float = 0., label_smoothing: float = 0., z_loss: float = 0.,
                 quantizer_metrics: bool = False, metrics_top_k: Optional[int] = None, valid_batches: int = 1):
        """quantizer_metrics (False: off, every step and ``validate`` run exactly what they run without it; no reference counterpart): per
        quantizer of every weighted sequence the mean nll, top-1 and top-k accuracy, mean entropy and count (metrics.QuantizerMetrics), formed
        on the device from the rows the loss walks.  Training: the micro-batches of an optimizer step accumulate onto one trainer-owned buffer
        (eager and HIP-graph route alike), ``train_step`` reads it beside its loss read, puts ``train_``-prefixed entries into its logs and the
        tracker record and zeroes it; the numbers are rank-local like logs['loss'] and describe the plain nll of the training-mode logits
        (label smoothing / z-loss excluded).  Validation: accumulated over ``valid_batches`` batches, summed over ranks, logged with the
        ``valid_`` prefix and kept as ``last_valid_metrics``.  metrics_top_k: the k of the top-k accuracy (None: what the sampler keeps at the
        default filter_thres = 0.9).  valid_batches > 1 (needs quantizer_metrics): valid_loss is the mean of the batch losses and
        valid_accuracy top1 / count of the last sequence; token dump and reconstructed waves still come from the first batch.
        label_smoothing / z_loss (0: off; no reference counterpart): the train wrapper's loss becomes (1 - eps) nll + eps smooth +
        zeta lse^2 per row (TokenConditionedTransformerWrapper, include/omlm.h), in the cross-entropy kernels.  Training mode only:
        ``validate`` (on the model or the EMA twin) reports the plain cross entropy, so valid_loss stays comparable across runs and is
        the plain-CE monitor of a regularised run, while the logged train loss carries both terms.
        null_cond_prob (0: off; no reference counterpart): the share of training samples whose CLAP condition is replaced by the null
        condition (TokenConditionedTransformerWrapper), the training side of ``generate(cond_scale=...)``.  validate, generate and the
        EMA twin's wrapper never drop.
        ema_decay (None: off; no reference counterpart): the fused optimizer step keeps an exponential moving average of the weights
        (ema.py); ``ema_transformer`` is a read-only twin on it, ``generate(use_ema=True)`` / ``validate(steps, use_ema=True)`` run on
        it, and checkpoints carry it ({stage}.transformer_ema.{steps}.pt beside the model; the optimizer file alone resumes it)."""
        super().__init__()
        # accelerate_kwargs is accepted for script compatibility: log_with / logging_dir select the JSONL tracker
        self.dp = DataParallel(device=transformer.device)
        if self.dp.is_distributed and transformer.device.type == 'cuda':
            # One process drives ONE GPU: cuda:LOCAL_RANK.  The reference's scripts build the model with device='cuda' (= cuda:0
            # on every rank) and rely on accelerator.prepare to place it (trainer.py:286-304); here the trainer moves the
            # transformer and the frozen front-ends before the optimizer adopts the parameters.
            target = torch.device('cuda', self.dp.local_rank % max(torch.cuda.device_count(), 1))
            torch.cuda.set_device(target)
            if transformer.device != target:
                transformer.to(target)
                for m in (wav2vec, neural_codec, audio_conditioner):
                    if isinstance(m, nn.Module):
                        m.to(target)
        self.log_with = accelerate_kwargs.get('log_with')
        self.logging_dir = accelerate_kwargs.get('logging_dir') or accelerate_kwargs.get('project_dir')

        self.use_preprocessed_data = use_preprocessed_data
        tokens_in = use_preprocessed_data or bool(default(dataset_yields_tokens, exists(dataset) and not exists(audio_conditioner)))
        self.model_config, self.training_config = model_config, training_config
        self.transformer = transformer
        self.wav2vec, self.audio_conditioner, self.neural_codec = wav2vec, audio_conditioner, neural_codec
        self.stage = stage

        if stage == 'semantic':
            assert tokens_in or (exists(audio_conditioner) and exists(wav2vec))
            token_fields, wave_fields = ('clap_token_ids', 'semantic_token_ids'), ('raw_wave_for_clap', 'raw_wave_for_semantic')
        elif stage == 'coarse':
            assert tokens_in or (exists(wav2vec) and exists(audio_conditioner) and exists(neural_codec))
            token_fields = ('clap_token_ids', 'semantic_token_ids', 'coarse_token_ids')
            wave_fields = ('raw_wave_for_clap', 'raw_wave_for_semantic', 'raw_wave_for_acoustic')
        elif stage == 'fine':
            assert tokens_in or (exists(audio_conditioner) and exists(neural_codec))
            token_fields = ('clap_token_ids', 'coarse_token_ids', 'fine_token_ids')
            wave_fields = ('raw_wave_for_clap', 'raw_wave_for_acoustic')
        else:
            raise ValueError(f'invalid stage: {stage}')
        self.cross_entropy_loss_weights = cross_entropy_loss_weights
        self.null_cond_prob = null_cond_prob
        self.label_smoothing, self.z_loss = label_smoothing, z_loss            # checked by the wrapper, by name
        self.train_wrapper = self._make_stage(transformer, null_cond_prob)
        # refusals by name, before any device work
        if isinstance(valid_batches, bool) or not isinstance(valid_batches, int) or valid_batches < 1:
            raise ValueError(f"valid_batches must be an integer >= 1, not {valid_batches!r}")
        if valid_batches > 1 and not quantizer_metrics:
            raise ValueError("valid_batches > 1 needs quantizer_metrics=True: the validation accuracy over several batches comes from the metrics' bins")
        self.quantizer_metrics, self.metrics_top_k, self.valid_batches = bool(quantizer_metrics), metrics_top_k, valid_batches
        if self.quantizer_metrics:
            from . import ops
            for seq, w in zip(transformer.token_sequences, self.train_wrapper.transformer_wrapper.cross_entropy_loss_weights):
                if w > 0:
                    ops.check_metrics_top_k(metrics_top_k, seq.codebook_size + 1)
        # the buffer the training micro-steps accumulate onto: made on first use, once the model is on its device, and before any capture
        self.__dict__['_train_metrics_buf'] = None
        self.last_valid_metrics = None
        self.ds_fields = token_fields if tokens_in else wave_fields

        self.register_buffer('steps', torch.Tensor([0]))
        self.num_train_steps, self.batch_size, self.grad_accum_every = num_train_steps, batch_size, grad_accum_every

        ema_kw = {} if ema_decay is None else dict(ema_decay=ema_decay, ema_update_after_step=ema_update_after_step, ema_warmup=ema_warmup)
        self.optim = get_optimizer(transformer.parameters(), lr=lr, wd=wd, **ema_kw)
        # the twin and its stage wrapper live in __dict__, NOT among the registered submodules: parameters(), .to() and state_dict() of
        # the trainer must not reach them (the twin's parameters are views of the optimizer's EMA buffer)
        self.__dict__['_ema_twin'] = self.__dict__['_ema_wrapper'] = None
        self.scheduler = get_linear_scheduler(self.optim, total_iters=lr_warmup) if lr_warmup > 0 else None
        self.max_grad_norm = max_grad_norm

        # ---- data ----
        if self.use_preprocessed_data:
            g = self.model_config.global_cfg
            self.ds = PreprocessedDataset(folder, stage=self.stage,
                                          semantic_window_seconds=int(g.semantic_audio_length_seconds),
                                          coarse_window_seconds=int(g.coarse_audio_length_seconds),
                                          fine_window_seconds=int(g.fine_audio_length_seconds),
                                          semantic_steps_per_second=self.model_config.hubert_kmeans_cfg.output_hz,
                                          acoustic_steps_per_second=self.model_config.encodec_cfg.output_hz)
        else:
            self.ds = dataset
            if not exists(self.ds):
                assert exists(folder), 'folder must be passed in, if not passing in a custom dataset for text conditioned audio synthesis training'
                self.ds = SoundDataset(folder, max_length_seconds=data_max_length_seconds, ignore_files=default(ignore_files, []),
                                       ignore_load_errors=ignore_load_errors)
        if valid_frac > 0:
            train_size = int((1 - valid_frac) * len(self.ds))
            valid_size = len(self.ds) - train_size
            self.ds, self.valid_ds = random_split(self.ds, [train_size, valid_size],
                                                  generator=torch.Generator().manual_seed(random_split_seed))
            self.print(f'training with dataset of {len(self.ds)} samples and validating with randomly splitted {len(self.valid_ds)} samples')
        else:
            self.valid_ds = self.ds
            self.print(f'training with shared training and valid dataset of {len(self.ds)} samples')

        make_dl = get_preprocessed_dataloader if (self.use_preprocessed_data or tokens_in) else get_dataloader
        sampler = vsampler = None
        if self.dp.is_distributed:        # per-rank shard of the data (accelerate.prepare(dl) equivalent; batch_size is per process)
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(self.ds, num_replicas=self.dp.world_size, rank=self.dp.rank, shuffle=True)
            vsampler = DistributedSampler(self.valid_ds, num_replicas=self.dp.world_size, rank=self.dp.rank, shuffle=True)
        self.dl = make_dl(self.ds, batch_size=batch_size, shuffle=sampler is None, sampler=sampler)
        self.valid_dl = make_dl(self.valid_ds, batch_size=batch_size, shuffle=vsampler is None, sampler=vsampler)
        self.dl_iter, self.valid_dl_iter = cycle(self.dl, sampler), cycle(self.valid_dl, vsampler)
        if self.dp.is_distributed and transformer.device.type == 'cuda':
            # replicas start identical (rank 0's weights / moments), but draw different forgetful masks and dropout masks
            self.optim.sync_replicas(self.dp)
            torch.cuda.manual_seed(int(torch.initial_seed() + 7919 * (self.dp.rank + 1)) & 0x7FFFFFFFFFFF)

        self.save_model_every, self.save_results_every = save_model_every, save_results_every
        self.save_predicted_tokens, self.save_reconstructed_wave = save_predicted_tokens, save_reconstructed_wave
        self.results_folder = Path(results_folder)
        if self.is_main and len([*self.results_folder.glob('**/*')]) > 0 and yes_or_no('do you want to clear previous experiment checkpoints and results?'):
            rmtree(str(self.results_folder))
        self.results_folder.mkdir(parents=True, exist_ok=True)
        self.dp.barrier()
        if exists(save_reconstructed_wave):
            self.waves_folder = self.results_folder / 'reconstructed_waves'
            self.waves_folder.mkdir(parents=True, exist_ok=True)
        if exists(save_predicted_tokens):
            self.tokens_folder = self.results_folder / 'tokens'
            self.tokens_folder.mkdir(parents=True, exist_ok=True)

        hps = {}
        if exists(model_config) and is_dataclass(model_config):
            hps.update(asdict(model_config.global_cfg))
            hps.update(asdict(getattr(model_config, f'{stage}_cfg')))
        if exists(training_config) and is_dataclass(training_config):
            hps.update(asdict(getattr(training_config, f'{stage}_trainer_cfg')))
        self.tracker = _JsonlTracker(self.logging_dir, f"{stage}_stage_{int(time.time() * 1000)}", hps,
                                     enabled=self.is_main and exists(self.log_with))
        if self.is_main and exists(config_paths):
            configs_folder = self.results_folder / "configs"
            configs_folder.mkdir(parents=True, exist_ok=True)
            for config_path in config_paths:
                copy_file_to_folder(config_path, configs_folder)
        # static-shape token training -> capture the micro-step into a HIP graph (graph.py); raw-audio front-ends stay eager
        self.use_hip_graph = tokens_in if use_hip_graph is None else use_hip_graph
        self._graphed = None

    def _make_stage(self, transformer, null_cond_prob=0.):
        """The stage wrapper of this trainer around `transformer`: the model (train_wrapper, with the trainer's condition drop) or its EMA
        twin (none).  Both carry label_smoothing / z_loss, which act in training mode only (the twin's wrapper lives in eval())."""
        w = self.cross_entropy_loss_weights
        reg = dict(label_smoothing=self.label_smoothing, z_loss=self.z_loss)
        if self.stage == 'semantic':
            return SemanticStage(semantic_transformer=transformer, wav2vec=self.wav2vec, clap=self.audio_conditioner,
                                 cross_entropy_loss_weights=default(w, [0., 1.]), null_cond_prob=null_cond_prob, **reg)
        if self.stage == 'coarse':
            return CoarseStage(coarse_transformer=transformer, neural_codec=self.neural_codec, wav2vec=self.wav2vec,
                               clap=self.audio_conditioner, cross_entropy_loss_weights=default(w, [0., 0., 1.]),
                               null_cond_prob=null_cond_prob, **reg)
        return FineStage(fine_transformer=transformer, clap=self.audio_conditioner, neural_codec=self.neural_codec,
                         cross_entropy_loss_weights=default(w, [0., 0., 1.]), null_cond_prob=null_cond_prob, **reg)

    # ---- checkpointing (trainer.py:359-391) ----------------------------------------------------------
    def save(self, model_path, optim_path, scheduler_path=None, ema_path=None):
        """ema_path: the EMA twin's plain state_dict (the model's keys), for inference scripts; the optimizer file alone resumes the EMA."""
        torch.save({k: v.detach().cpu() for k, v in self.transformer.state_dict().items()}, model_path)
        torch.save(self.optim.state_dict(), optim_path)
        if exists(self.scheduler):
            assert exists(scheduler_path)
            torch.save(self.scheduler.state_dict(), scheduler_path)
        if exists(ema_path):
            torch.save({k: v.detach().cpu() for k, v in self._require_ema().state_dict().items()}, ema_path)

    def load(self, model_path, optim_path, scheduler_path=None, steps=0, ema_path=None):
        """ema_path: overwrite the EMA the optimizer file restored with a twin state_dict.  Nothing of the EMA clock is reset: it is the
        Adam clock, which the optimizer file restores."""
        model_path, optim_path = Path(model_path), Path(optim_path)
        assert model_path.exists() and optim_path.exists()
        self.transformer.load_state_dict(torch.load(model_path, map_location=self.device))
        self.optim.load_state_dict(torch.load(optim_path, map_location=self.device, weights_only=False))
        if exists(ema_path):
            assert Path(ema_path).exists()
            self._require_ema().load_state_dict(torch.load(ema_path, map_location=self.device))      # in place: into the views of E
            self.optim._bump_twins()
        if exists(self.scheduler):
            assert exists(scheduler_path), 'the config specifies lr warmup is used, but no scheduler checkpoint is given. try setting lr_warmup to 0.'
            scheduler_path = Path(scheduler_path)
            assert scheduler_path.exists()
            self.scheduler.load_state_dict(torch.load(scheduler_path, map_location=self.device, weights_only=False))
        self._graphed = None        # weights changed under the captured graph: re-capture on the next micro-step
        # the restored loss-scale block carries the CUMULATIVE skipped-step count, and the restored scheduler was already rewound for those
        # skips: without this the first train_step after a resume reported them again and rewound the warm-up a second time
        rep = self.optim.loss_scale_report() if hasattr(self.optim, 'loss_scale_report') else {}
        self._skipped_seen = rep.get('skipped_steps', 0)
        if self.dp.is_distributed and self.device.type == 'cuda':
            self.optim.sync_replicas(self.dp)
        if steps > 0:
            assert int(self.steps.item()) == 0, 'steps should be 0 when loading a checkpoint for the first time'
            self.steps += steps

    def print(self, msg):
        self.dp.print(msg)

    @property
    def ema_transformer(self) -> Optional[TokenConditionedTransformer]:
        """The read-only twin on the optimizer's weight EMA (ema.EmaTwin), or None with the EMA off.  Built on first use, once the model
        is on the device (the optimizer's flat buffers exist only there)."""
        if self._ema_twin is None and self.optim.ema_enabled and self.device.type == 'cuda':
            from .ema import EmaTwin
            self.__dict__['_ema_twin'] = EmaTwin(self.transformer, self.optim)
            self.__dict__['_ema_wrapper'] = self._make_stage(self._ema_twin).eval()
        return self._ema_twin

    def _require_ema(self):
        if self.ema_transformer is None:
            raise ValueError("this trainer keeps no weight EMA: construct it with ema_decay")
        return self.ema_transformer

    def generate(self, *args, use_ema=False, **kwargs):
        """The wrapper's generate, every keyword passed on: with ``return_logprobs=True`` it returns (ids, LogProbs), with ``cond_scale`` it
        decodes under classifier-free guidance; ``temperature``, ``filter_thres``, ``top_p``, ``cond_scale`` and ``sampler_seed`` take a
        number or one value per row.
        use_ema: sample from the weight EMA (the twin) instead of the training weights."""
        if use_ema:
            self._require_ema()
            return self._ema_wrapper.generate(*args, **kwargs)
        return self.train_wrapper.generate(*args, **kwargs)

    @property
    def device(self):
        return self.transformer.device

    @property
    def is_distributed(self):
        return self.dp.is_distributed

    @property
    def is_main(self):
        return self.dp.is_main

    @property
    def is_local_main(self):
        return self.dp.is_local_main

    def _next_batch(self, it):
        batch = next(it)
        if isinstance(batch, torch.Tensor):
            batch = (batch,)
        return {k: v.to(self.device, non_blocking=True) for k, v in zip(self.ds_fields, batch)}

    # ---- one optimizer step (trainer.py:415-552) -------------------------------------------------------
    def train_metrics(self):
        """The trainer-owned metrics.QuantizerMetrics of the training micro-steps (None with quantizer_metrics off): one device buffer that
        exists before the micro-step is captured, so every replay adds to it."""
        if not self.quantizer_metrics:
            return None
        buf = self._train_metrics_buf
        if buf is None or buf.bins.device != self.device:
            buf = self.__dict__['_train_metrics_buf'] = self.train_wrapper.transformer_wrapper.new_metrics(self.metrics_top_k)
        return buf

    def micro_step(self, data_kwargs):
        """forward + backward of ONE micro-batch; gradients accumulate in the optimizer's flat buffer, and with quantizer_metrics the rows'
        metrics onto ``train_metrics()``."""
        # part of what the captured callable closes over: the flag decides the launches, the buffer is the one every replay adds to
        mkw = dict(return_metrics=self.train_metrics()) if self.quantizer_metrics else {}
        if self.use_hip_graph and self.device.type == 'cuda':
            if self._graphed is None:
                from .graph import GraphedForwardBackward
                self._graphed = GraphedForwardBackward(lambda **kw: self.train_wrapper(**kw, return_loss=True, return_logits=False, **mkw)[0],
                                                       loss_scale=1.0 / self.grad_accum_every)

                def discard():                          # warm-up steps really ran: throw their gradients (and metrics) away
                    self.optim.mark_grads_dirty()
                    self.optim.zero_grad()
                    if mkw:
                        mkw['return_metrics'].zero_()
                    rc = self._relpos_cache()
                    if rc is not None:
                        rc.reset_accum()
                self._graphed.prepare(data_kwargs, after_warmup=discard)
                if self._graphed.capture_error:
                    self.print(f'HIP graph capture unavailable ({self._graphed.capture_error}); launching eagerly')
            loss = self._graphed(**data_kwargs)
            self.optim.mark_grads_dirty()
            return loss.clone()
        loss = self.train_wrapper(**data_kwargs, return_loss=True, return_logits=False, **mkw)[0]
        (loss / self.grad_accum_every).backward()
        self.optim.mark_grads_dirty()
        return loss.detach()

    def _relpos_cache(self):
        """engine.RelposStepCache of the transformer's trunk when gradient accumulation makes it pay (grad_accum_every > 1, learned MLP bias,
        HIP path); OMLM_RELPOS_CACHE=0 keeps the per-micro-batch form."""
        if self.grad_accum_every <= 1 or self.device.type != 'cuda' or os.environ.get("OMLM_RELPOS_CACHE", "1") == "0":
            return None
        tr = getattr(self.transformer, "transformer", None)
        if tr is None or getattr(tr, "rel_pos_bias", None) is None or getattr(tr, "relative_position_bias_type", "") == "t5":
            return None
        from . import engine
        rc = engine.relpos_step_cache(tr)
        rc.enabled = True
        return rc

    def optimizer_step(self):
        """ONE gradient exchange + fused clip/Adam(W)/zero_grad + scheduler tick.  Precision "fp16": a step whose gradients overflowed is
        skipped ON THE DEVICE (no host read here), so the tick happens regardless; train_step, which reads the skip counter next to its loss
        read-back anyway, takes the tick back (_rewind_scheduler) -- warm-up and decay then advance with the Adam clock, on applied steps only."""
        self.dp.allreduce_sum_(self.optim.flat_grad)
        self.optim.step(max_grad_norm=self.max_grad_norm, grad_scale=self.dp.grad_scale())
        if exists(self.scheduler):
            self.scheduler.step()

    def _rewind_scheduler(self, n: int):
        """Take back the scheduler ticks of n optimizer steps the device skipped (fp16 overflow): LinearLR is a closed form of last_epoch."""
        sch = self.scheduler
        if not exists(sch) or n <= 0 or not hasattr(sch, "_get_closed_form_lr"):
            return
        sch.last_epoch = max(sch.last_epoch - n, 0)
        lrs = sch._get_closed_form_lr()
        for g, lr in zip(sch.optimizer.param_groups, lrs):
            g['lr'] = lr
        sch._last_lr = list(lrs)

    def train_step(self):
        steps = int(self.steps.item())
        self.transformer.train()
        self.train_wrapper.train()
        self.optim.zero_grad()
        loss_acc = torch.zeros((), device=self.device)
        rc = self._relpos_cache()
        if rc is not None:
            rc.refresh()                                # the rel-pos table of this step's weights, once for all its micro-batches
        for _ in range(self.grad_accum_every):
            loss_acc += self.micro_step(self._next_batch(self.dl_iter))
        if rc is not None:
            rc.flush()                                  # the MLP's backward on the micro-batches' summed d(table), before the exchange
        self.optimizer_step()
        logs = {'loss': float(loss_acc.item()) / self.grad_accum_every}       # single host sync per optimizer step
        train_metrics = {}
        if self.quantizer_metrics:                   # the host has just waited for the device: this read waits for nothing new
            train_metrics = self.train_metrics().to_dict("train_")
            self.train_metrics().zero_()
            logs.update(train_metrics)
        if self.device.type == 'cuda':
            # the host has just waited for the device: a token id / label past its table (wrong codebook size, damaged token store)
            # was skipped by the kernels and flagged -- surface it like torch's device assert would
            from . import ops
            ops.raise_on_index_error(self.device)
            rep = self.optim.loss_scale_report() if hasattr(self.optim, "loss_scale_report") else {}
            if rep:                                  # precision "fp16": overflowed steps are skipped on the device -- say so
                logs.update(loss_scale=rep["scale"], skipped_steps=rep["skipped_steps"])
                if rep["skipped_steps"] > getattr(self, "_skipped_seen", 0):
                    self.print(f"{steps}: fp16 gradient overflow -- optimizer step skipped ({rep['skipped_steps']} so far), "
                               f"loss scale now {rep['scale']:g}")
                    self._rewind_scheduler(rep["skipped_steps"] - getattr(self, "_skipped_seen", 0))
                    self._skipped_seen = rep["skipped_steps"]
        self.print(f"{steps}: loss: {logs['loss']}")

        valid_loss = valid_accuracy = None
        valid_metrics = {}
        if not (steps % self.save_results_every):
            valid_loss, valid_accuracy = self.validate(steps)
            if self.quantizer_metrics:
                valid_metrics = self.last_valid_metrics
        self.tracker.log({"train_loss": logs['loss'], "valid_loss": valid_loss, "valid_accuracy": valid_accuracy,
                          **train_metrics, **valid_metrics}, step=steps)

        if self.is_main and not (steps % self.save_model_every):
            self.print(f'{steps}: saving model to {str(self.results_folder)}')
            self.save(str(self.results_folder / f'{self.stage}.transformer.{steps}.pt'),
                      str(self.results_folder / f'{self.stage}.optimizer.{steps}.pt'),
                      str(self.results_folder / f'{self.stage}.scheduler.{steps}.pt'),
                      **({} if self.ema_transformer is None else
                         dict(ema_path=str(self.results_folder / f'{self.stage}.transformer_ema.{steps}.pt'))))
            if exists(self.audio_conditioner) and getattr(self.audio_conditioner, 'learn_rvq', False):
                torch.save(self.audio_conditioner.rq.state_dict(), str(self.results_folder / f'{self.stage}.conditioner_rvq.{steps}.pt'))
        self.steps += 1
        return logs

    @torch.no_grad()
    def validate(self, steps, use_ema=False):
        """trainer.py:457-526: teacher-forced validation loss / token accuracy, token dumps, optional wave reconstruction.
        use_ema: on the weight EMA (the twin) instead of the training weights.
        With quantizer_metrics: additionally the per-quantizer metrics of ``valid_batches`` batches (the batches after the first run with
        return_logits=False: no logits leave the device), summed over ranks, in ``last_valid_metrics`` (``valid_`` prefix); every host read
        comes after the last batch's launches.  The return value stays (valid_loss, valid_accuracy); with valid_batches > 1 they are the mean
        of the batch losses and top1 / count of the last sequence from the bins."""
        if use_ema:
            self._require_ema()
        wrapper = self._ema_wrapper if use_ema else self.train_wrapper
        wrapper.eval()
        data_kwargs = self._next_batch(self.valid_dl_iter)
        if not self.quantizer_metrics:
            valid_loss, all_logits, all_labels = wrapper(**data_kwargs, return_loss=True)
            valid_loss = float(self.dp.reduce_mean(valid_loss.detach().reshape(1)).item())
        else:
            vm = wrapper.transformer_wrapper.new_metrics(self.metrics_top_k)
            loss_sum, all_logits, all_labels, _ = wrapper(**data_kwargs, return_loss=True, return_metrics=vm)
            loss_sum = loss_sum.detach().reshape(1)
            for _ in range(self.valid_batches - 1):
                more = wrapper(**self._next_batch(self.valid_dl_iter), return_loss=True, return_logits=False, return_metrics=vm)
                loss_sum = loss_sum + more[0].detach().reshape(1)
            self.dp.sum_across_ranks_(vm.bins)                  # fp64 counters, in their own dtype
            valid_loss = float(self.dp.reduce_mean(loss_sum / self.valid_batches).item())
            host = vm._host()
            self.last_valid_metrics = vm.to_dict("valid_", host=host)
        pred = self.dp.all_gather_cat(all_logits[-1].argmax(1).contiguous()).cpu().long()
        gt = self.dp.all_gather_cat(all_labels[-1].contiguous()).cpu().long()
        valid_accuracy = (pred == gt).float().mean().item()
        if self.valid_batches > 1:
            last = host[-1, :vm.quantizers[-1] + 1]
            valid_accuracy = float(last[:, 3].sum()) / max(float(last[:, 0].sum()), 1.0)
        self.print(f'{steps}: valid loss {valid_loss}, valid acc {valid_accuracy}')
        if self.is_main and self.save_predicted_tokens:
            inter = torch.empty((pred.shape[0] + gt.shape[0], pred.shape[1]), dtype=pred.dtype)
            inter[0::2], inter[1::2] = pred, gt
            np.savetxt(str(self.tokens_folder / f'{self.stage}.tokens.{steps}.txt'), inter, fmt='%-6s',
                       header='predicted and ground truth tokens from the validation set. row 0%2 is predicted, 1%2 is ground truth\n ')
        if self.is_main and self.save_reconstructed_wave and self.stage in ('coarse', 'fine') and exists(self.neural_codec):
            toks = all_logits[-1].argmax(1)[:, :-1]
            toks[toks == self.transformer.eos_ids[-1]] = 0
            q = self.transformer.token_sequences[-1].num_quantizers
            toks = toks.reshape(toks.shape[0], -1, q)
            if self.stage == 'fine':
                cq = self.transformer.token_sequences[-2].num_quantizers
                coarse = all_labels[-2][:, :-1].reshape(toks.shape[0], -1, cq)
                toks = torch.cat((coarse, toks), dim=-1)
            waves = self.neural_codec.decode_from_codebook_indices(toks).cpu()
            try:
                import torchaudio
                for i, wave in enumerate(waves[:4]):
                    torchaudio.save(str(self.waves_folder / f'{self.stage}.reconstructed_wave_{i}.{steps}.wav'), wave, self.neural_codec.sample_rate)
            except ImportError:
                pass
        return valid_loss, valid_accuracy

    def train(self, log_fn=noop):
        while self.steps < self.num_train_steps:
            logs = self.train_step()
            log_fn(logs)
        self.print('training complete')


class ClapRVQTrainer(nn.Module):
    """Learn the residual vector quantizer that turns CLAP embeddings into discrete tokens (trainer.py:564-741).

    Same constructor and step contract as the reference: every step accumulates ``accumulate_batches`` batches of embeddings,
    concatenates them over ranks, and rank 0 runs ONE training-mode pass of the residual VQ over them
    (``audio_conditioner.quantize(embeds, return_rvq_loss=True)`` with ``learn_rvq``: k-means init on the first pass, then EMA
    codebook updates -- csrc/vq_fit.hip); ``clap.rvq.{steps}.pt`` checkpoints carry the library's key layout.
    The CLAP towers are third-party pretrained networks that are not part of this build: when ``audio_conditioner.clap`` is None
    the dataset must yield the embeddings themselves ([D] or [n, D] float tensors, e.g. precomputed CLAP embeddings)."""

    def __init__(self, *, num_train_steps, batch_size, accumulate_batches: Optional[int] = None, audio_conditioner=None,
                 dataset: Optional[Dataset] = None, ignore_files: Optional[List[str]] = None, ignore_load_errors: bool = True,
                 folder=None, wd=0., max_grad_norm=0.5, data_max_length_seconds=10, valid_frac=0.05, random_split_seed=42,
                 save_results_every=100, save_model_every=1000, results_folder='./results', accelerate_kwargs: dict = {},
                 config_paths: Optional[List[str]] = None):
        super().__init__()
        assert exists(audio_conditioner), 'audio_conditioner (ClapQuantized) must be passed in'
        dev = audio_conditioner.rq.codebooks.device
        self.dp = DataParallel(device=dev)
        self.log_with = accelerate_kwargs.get('log_with')
        self.logging_dir = accelerate_kwargs.get('logging_dir') or accelerate_kwargs.get('project_dir')
        self.audio_conditioner = audio_conditioner
        self.embeds_in = not exists(getattr(audio_conditioner, 'clap', None))
        self.ds = dataset
        self.num_train_steps = num_train_steps
        self.accumulate_batches = accumulate_batches
        self.register_buffer('steps', torch.Tensor([0]))
        if not exists(self.ds):
            assert exists(folder), 'folder must be passed in, if not passing in a custom dataset for text conditioned audio synthesis training'
            self.ds = SoundDataset(folder, max_length_seconds=data_max_length_seconds, target_sample_hz=audio_conditioner.sample_rate,
                                   seq_len_multiple_of=None, ignore_files=default(ignore_files, []), ignore_load_errors=ignore_load_errors)
        if valid_frac > 0:
            train_size = int((1 - valid_frac) * len(self.ds))
            valid_size = len(self.ds) - train_size
            self.ds, self.valid_ds = random_split(self.ds, [train_size, valid_size],
                                                  generator=torch.Generator().manual_seed(random_split_seed))
            self.print(f'training with dataset of {len(self.ds)} samples and validating with randomly splitted {len(self.valid_ds)} samples')
        else:
            self.valid_ds = self.ds
            self.print(f'training with shared training and valid dataset of {len(self.ds)} samples')
        # every rank draws ITS shard of the data (what accelerator.prepare(dl) gives the reference, trainer.py:664-669): with plain
        # shuffle=True loaders identically seeded ranks would all contribute the same batches to the gather below
        sampler = _rank_sampler(self.dp, self.ds)
        self.dl = get_dataloader(self.ds, batch_size=batch_size, shuffle=sampler is None, sampler=sampler)
        self.valid_dl = get_dataloader(self.valid_ds, batch_size=batch_size, shuffle=True)
        self.dl_iter, self.valid_dl_iter = cycle(self.dl, sampler), cycle(self.valid_dl)
        self.save_model_every, self.save_results_every = save_model_every, save_results_every
        self.results_folder = Path(results_folder)
        if self.is_main and len([*self.results_folder.glob('**/*')]) > 0 and \
                yes_or_no('do you want to clear previous experiment checkpoints and results?'):
            rmtree(str(self.results_folder))
        self.results_folder.mkdir(parents=True, exist_ok=True)
        hps = {"num_train_steps": num_train_steps, "batch_size": batch_size, "accumulate_batches": accumulate_batches}
        self.tracker = _JsonlTracker(self.logging_dir, "clap_rvq", hps, self.is_main and exists(self.log_with))
        if self.is_main and exists(config_paths):
            configs_folder = self.results_folder / "configs"
            configs_folder.mkdir(parents=True, exist_ok=True)
            for config_path in config_paths:
                copy_file_to_folder(config_path, configs_folder)

    def print(self, msg):
        if self.is_main:
            print(msg)

    @property
    def device(self):
        return self.audio_conditioner.rq.codebooks.device

    @property
    def is_distributed(self):
        return self.dp.is_distributed

    @property
    def is_main(self):
        return self.dp.rank == 0

    @property
    def is_local_main(self):
        return self.dp.local_rank == 0

    def _embed(self, batch) -> torch.Tensor:
        item = batch[0] if isinstance(batch, (list, tuple)) else batch
        if self.embeds_in:
            emb = item.to(self.device).float()
            return emb.reshape(-1, emb.shape[-1])
        return self.audio_conditioner.forward(audio_input=item.to(self.device), return_embedding=True)

    def train_step(self):
        steps = int(self.steps.item())
        self.audio_conditioner.learn_rvq = True
        iters = default(self.accumulate_batches, 1)
        iters = -(-iters // self.dp.world_size)
        embeds = torch.cat([self._embed(next(self.dl_iter)) for _ in range(iters)], dim=0)
        embeds = _gather_rows(self.dp, embeds)
        logs = {}
        if self.is_main:
            loss = self.audio_conditioner.quantize(embeds, return_rvq_loss=True)
            self.print(f'loss: {loss}')
            valid_loss = None
            if not (steps % self.save_results_every):
                with torch.no_grad():
                    self.audio_conditioner.learn_rvq = False
                    valid_loss = self.audio_conditioner.quantize(self._embed(next(self.valid_dl_iter)), return_rvq_loss=True)
                self.print(f'{steps}: valid loss {valid_loss}')
            logs = {"train_loss": loss, "valid_loss": valid_loss}
            self.tracker.log(logs, step=steps)
            if not (steps % self.save_model_every):
                torch.save(self.audio_conditioner.rq.state_dict(), str(self.results_folder / f'clap.rvq.{steps}.pt'))
                self.print(f'{steps}: saving model to {str(self.results_folder)}')
        self.steps += 1
        return logs

    def train(self, log_fn=noop):
        while self.steps < self.num_train_steps:
            logs = self.train_step()
            log_fn(logs)
        self.print('training complete')


class HfHubertKmeansTrainer(nn.Module):
    """Trainer for the k-means part of HfHubertWithKmeans (trainer.py:748-905): 1) collect `feature_extraction_num_steps` batches
    of features, 2) fit sklearn's MiniBatchKMeans on them (`learn_kmeans`, the reference's own call) and dump `kmeans.joblib`;
    `train(device='cuda')` fits on the device instead (kmeans_fit.py) and keeps the features there.
    The MERT / HuBERT extractor is a third-party pretrained network that is not part of this build: when `hubert_kmeans.hubert`
    is None the dataset must yield the features themselves ([t, f] or [b, t, f] float tensors, e.g. precomputed MERT layer-7
    embeddings); with an extractor present the reference's `forward(wav_input=..., return_embed=True)` path is used."""

    def __init__(self, *, feature_extraction_num_steps: int, feature_extraction_batch_size: int, hubert_kmeans,
                 dataset: Optional[Dataset] = None, ignore_files: Optional[List[str]] = None, ignore_load_errors: bool = True,
                 folder=None, data_max_length_seconds=1, results_folder='./results', accelerate_kwargs: dict = {},
                 config_paths: Optional[List[str]] = None):
        super().__init__()
        self.dp = DataParallel(device=torch.device('cpu'), backend='gloo')
        self.ds = dataset
        self.feature_extraction_num_steps = feature_extraction_num_steps
        self.feature_extraction_batch_size = feature_extraction_batch_size
        self.hubert_kmeans = hubert_kmeans
        self.features_in = not exists(getattr(hubert_kmeans, 'hubert', None))
        self.register_buffer('steps', torch.Tensor([0]))
        if not exists(self.ds):
            assert exists(folder), 'folder must be passed in, if not passing in a custom dataset for text conditioned audio synthesis training'
            self.ds = SoundDataset(folder, max_length_seconds=data_max_length_seconds, normalize=True,
                                   target_sample_hz=hubert_kmeans.target_sample_hz, seq_len_multiple_of=hubert_kmeans.seq_len_multiple_of,
                                   ignore_files=default(ignore_files, []), ignore_load_errors=ignore_load_errors)
        self.print(f'training on {feature_extraction_num_steps * feature_extraction_batch_size} out of {len(self.ds)} samples')
        sampler = _rank_sampler(self.dp, self.ds)                            # per-rank shard (trainer.py:812-815 in the reference)
        self.dl = get_dataloader(self.ds, batch_size=feature_extraction_batch_size, shuffle=sampler is None, sampler=sampler)
        self.dl_iter = cycle(self.dl, sampler)
        self.results_folder = Path(results_folder)
        if self.is_main and len([*self.results_folder.glob('**/*')]) > 0 and \
                yes_or_no('do you want to clear previous experiment checkpoints and results?'):
            rmtree(str(self.results_folder))
        self.results_folder.mkdir(parents=True, exist_ok=True)
        if self.is_main and exists(config_paths):
            configs_folder = self.results_folder / "configs"
            configs_folder.mkdir(parents=True, exist_ok=True)
            for config_path in config_paths:
                copy_file_to_folder(config_path, configs_folder)

    def print(self, msg):
        if self.is_main:
            print(msg)

    @property
    def device(self):
        return torch.device('cpu')

    @property
    def is_distributed(self):
        return self.dp.is_distributed

    @property
    def is_main(self):
        return self.dp.rank == 0

    @property
    def is_local_main(self):
        return self.dp.local_rank == 0

    def extract_hubert_features(self):
        return self._extract_hubert_features().cpu().numpy()

    def _extract_hubert_features(self) -> torch.Tensor:
        batch = next(self.dl_iter)
        item = batch[0] if isinstance(batch, (list, tuple)) else batch
        if self.features_in:
            embed = item.float()
            embed = embed.reshape(-1, embed.shape[-1])                       # 'b t f -> (b t) f'
        else:
            dev = next(self.hubert_kmeans.parameters(), item).device       # the waveform goes to the extractor's device
            embed = self.hubert_kmeans.forward(wav_input=item.to(dev), return_embed=True)
            embed = embed.reshape(-1, embed.shape[-1])
        return _gather_rows(self.dp, embed.detach())

    def train(self, log_fn=noop, seed=0, **kmeans_kwargs):
        """`train(device='cuda')` (forwarded to learn_kmeans with the other keywords) fits on the device; the gathered features then
        stay device tensors, NaN-row filter included, instead of the numpy round trip."""
        from .hf_hubert_kmeans import learn_kmeans
        fit_device = kmeans_kwargs.get('device')
        if fit_device is not None:
            from .kmeans_fit import require_cuda_device
            fit_device = require_cuda_device(fit_device)
        self.print('step 1: extracting features. must wait for this to complete before training kmeans.')
        features = []
        num_steps = -(-self.feature_extraction_num_steps // self.dp.world_size)
        while self.steps < num_steps:
            self.print(f'{int(self.steps.item())} / {num_steps} steps')
            if fit_device is not None:
                features.append(self._extract_hubert_features().to(fit_device))
            else:
                features.append(self.extract_hubert_features())
            self.steps += 1
        if fit_device is not None:
            features = torch.cat(features, dim=0).float()
            features = features[~torch.isnan(features).any(dim=-1)].contiguous()
        else:
            features = np.concatenate(features, axis=0)
            features = features[~np.any(np.isnan(features), axis=-1)]
        self.print('step 2: training kmeans')
        if self.is_main:
            self.kmeans_model = learn_kmeans(features, seed, str(self.results_folder / 'kmeans.joblib'),
                                             n_clusters=self.hubert_kmeans.codebook_size, **kmeans_kwargs)
        self.print('training complete')
