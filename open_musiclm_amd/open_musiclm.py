"""TokenConditionedTransformer, its training / sampling wrapper, the three stages and MusicLM, with the
reference's public API (reference open_musiclm/open_musiclm.py) on top of the MI355X engine.

Host responsibilities kept here (all on tiny integer tensors): eos append, label construction, key-mask
construction incl. the forgetful mask, loss weighting bookkeeping, the AR sampling loop and the
sliding-window hierarchical decode.  Everything floating point goes through ``engine`` -> libomlm_hip.so.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass
from typing import List, Mapping, Optional

import torch
import torch.nn.functional as F
from torch import nn
from tqdm import tqdm

from . import decode, engine, hip, ops
from .transformer import Transformer
from .utils import (append_eos_id, batch_unique_consecutive, beartype_jit, default, eval_decorator, exists,
                    float32_to_int16, generate_mask_with_prob, int16_to_float32, mask_out_after_eos_id)


@dataclass
class TokenSequenceInfo():
    """open_musiclm.py:23-30"""
    codebook_size: int
    num_quantizers: int
    unique_consecutive: bool


# Test hook: callable (n_draws, batch, V + 1) -> [n_draws, batch, V + 1] uniforms consumed by `generate` in place of the device
# RNG when no `uniforms` argument is given (the golden test of MusicLM.forward replays the reference's draws through it).
UNIFORM_SOURCE = None
_DEVICE_RNG = object()            # generate(): the uniforms of a call that are drawn from torch's generator on the device


def _flat(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(t.shape[0], -1)


class TokenConditionedTransformer(nn.Module):
    """open_musiclm.py:33-215.  Parameters and state_dict keys are identical to the reference:
    start_tokens.{i}, logit_weights.{i}, embeddings.{i}.weight, [absolute_position_embeddings.{i}.weight],
    transformer.*"""

    def __init__(self, *, token_sequences: List[TokenSequenceInfo], dim, depth, heads=8, attn_dropout=0.,
                 ff_dropout=0.1, has_condition=False, cond_as_self_attn_prefix=False, cond_drop_prob=0.5,
                 grad_shrink_alpha=0.1, use_absolute_position_embeddings=False,
                 max_absolute_position_embeddings=262, precision: Optional[str] = None, **kwargs):
        super().__init__()
        if len(token_sequences) > 4:
            raise ValueError("at most 4 token sequences are supported by the fused gather kernel")
        self.token_sequences = token_sequences
        self.dim = dim
        self.has_condition = has_condition
        self.cond_drop_prob = cond_drop_prob
        self.use_absolute_position_embeddings = use_absolute_position_embeddings
        self.precision = precision            # None -> engine.default_precision() ($OMLM_PRECISION, default bf16)

        self.start_tokens = torch.nn.ParameterList()
        self.logit_weights = torch.nn.ParameterList()
        self.embeddings = torch.nn.ModuleList()
        self.absolute_position_embeddings = torch.nn.ModuleList() if use_absolute_position_embeddings else None
        self.eos_ids = []
        for sequence in token_sequences:
            self.start_tokens.append(nn.Parameter(torch.randn(dim)))
            self.eos_ids.append(sequence.codebook_size)
            rows = sequence.codebook_size + 1
            self.embeddings.append(nn.Embedding(rows * sequence.num_quantizers, dim))
            self.logit_weights.append(nn.Parameter(torch.randn(sequence.num_quantizers, rows, dim)))
            if use_absolute_position_embeddings:
                self.absolute_position_embeddings.append(nn.Embedding(max_absolute_position_embeddings, dim))

        self.transformer = Transformer(dim=dim, depth=depth, heads=heads, attn_dropout=attn_dropout,
                                       ff_dropout=ff_dropout,
                                       cross_attend=has_condition and not cond_as_self_attn_prefix,
                                       cond_as_self_attn_prefix=cond_as_self_attn_prefix,
                                       grad_shrink_alpha=grad_shrink_alpha, **kwargs)
        self.transformer.__dict__["_omlm_owner"] = self
        engine.tag_parameters(self, precision)      # the fused optimizer reads the precision mode off the parameters (16-bit shadow type, loss scale)

    def __setstate__(self, state):
        """pickle / torch.load(model) / copy.deepcopy (EMA copies) / spawn: the parameter -> model registry of engine.tag_parameters is keyed by
        object identity, so a reconstructed model registers its own parameters again (the precision tag itself travels in the Parameter's
        __dict__); without this FusedAdam found 'fp16 parameters without their model' on such a copy."""
        super().__setstate__(state)
        self.transformer.__dict__["_omlm_owner"] = self
        self.__dict__.pop("_omlm_prepared", None)             # operand images of the ORIGINAL's parameters
        engine.tag_parameters(self, self.precision)

    @property
    def device(self):
        return next(self.parameters()).device

    def _precision(self) -> str:
        return self.precision or engine.default_precision()

    def forward(self, *, all_token_ids: List[torch.Tensor], self_attn_mask=None, cond_drop_prob=None,
                return_only_final_seq_logits=False):
        """Returns one [B, n_i, codebook_size+1] fp32 logits tensor per sequence (None for skipped ones).
        cond_drop_prob is accepted and ignored exactly like the reference (no text conditioning)."""
        assert len(all_token_ids) == len(self.token_sequences) == len(self.embeddings)
        ids = [_flat(t).to(self.device) for t in all_token_ids]
        prec = self._precision()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            outs = engine.LogitsFunction.apply(self, ids, self_attn_mask, bool(return_only_final_seq_logits), prec,
                                               *self.parameters())
            it = iter(outs)
            n = len(self.token_sequences)
            return [next(it) if (not return_only_final_seq_logits or s == n - 1) else None for s in range(n)]
        bufs, lay, _ = engine.run_forward(self, ids, self_attn_mask, bool(return_only_final_seq_logits), False, prec)
        return engine.logits_views(self, lay, bufs)

    def forward_with_cond_scale(self, *args, cond_scale=3, **kwargs):
        """open_musiclm.py:192-215: a no-op around forward() without text conditioning."""
        logits = self.forward(*args, cond_drop_prob=0., **kwargs)
        if cond_scale == 1 or not self.has_condition:
            return logits
        null_logits = self.forward(*args, cond_drop_prob=1., **kwargs)
        return [None if a is None else b + (a - b) * cond_scale for a, b in zip(logits, null_logits)]

    # ---- fast paths used by the wrapper ---------------------------------------------------------------
    def last_logits(self, ids: List[torch.Tensor], self_attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, ldV] logits of the final position of the final sequence only (AR decode step, no autograd).  self_attn_mask: the key
        mask [B, rows] of forward(), True = attend; None: every key is attended."""
        bufs, _, _ = engine.run_forward(self, ids, self_attn_mask, True, False, self._precision(), final_rows_only=True)
        return bufs[-1]

    def loss_and_logits(self, ids, labels, self_attn_mask, loss_weights, ignore_negative=None, all_logits=True,
                        label_smoothing=0., z_loss=0., metrics=None):
        """metrics (extension): a metrics.QuantizerMetrics that every weighted sequence's rows are accumulated onto by the two launches of
        csrc/ce_metrics.hip, behind the loss's own forward launch and on the same logits; the loss, the logits and the backward are bit for
        bit what they are without it.  None (the default): the launches it always made.
        ignore_negative[s]: labels < 0 of sequence s are ignore_index rows AND leave the loss normaliser (the padded labels of
        a unique_consecutive sequence, open_musiclm.py:396-404).  all_logits=False: the heads of zero-weight sequences are not
        evaluated (their logits come back as None).
        label_smoothing / z_loss (extensions; include/omlm.h): the loss is sum_s w_s ((1 - eps) NLL_s + eps S_s + zeta Z_s) / total, formed
        and differentiated in the cross-entropy kernels.  Both 0 (the default): the plain cross entropy, the calls it always made.  This
        method applies what it is given; the wrapper passes them in training mode only."""
        ign = tuple(bool(v) for v in ignore_negative) if ignore_negative is not None else (False,) * len(labels)
        reg = (ops.check_label_smoothing(label_smoothing), ops.check_z_loss(z_loss))
        return engine.LossFunction.apply(self, ids, labels, self_attn_mask, tuple(loss_weights), ign, self._precision(),
                                         bool(all_logits), reg, metrics, *self.parameters())


_GENERATE_MASK_ORIG = generate_mask_with_prob


def null_condition_ids(info: TokenSequenceInfo, n: int, device=None) -> torch.Tensor:
    """The null condition of classifier-free guidance (include/omlm.h) as raw ids of `n` positions of a sequence described by `info`:
    -1 - codebook_size * (p mod Q) at position p -- -1 after the per-quantizer offset, which every embedding path (get_embeds, the gather
    kernel, the oracle) gives the zero row of the pad embedding."""
    p = torch.arange(n, device=device, dtype=torch.long)
    return -1 - info.codebook_size * (p % info.num_quantizers) if info.num_quantizers > 1 else torch.full_like(p, -1)


def null_twin(cond_ids: torch.Tensor, info: TokenSequenceInfo, n_ids: int) -> torch.Tensor:
    """cond_ids [B, L] (the flattened condition, an eos possibly appended behind its n_ids id positions) with every id position replaced by
    the null condition; what lies behind them (the eos) is kept."""
    out = cond_ids.clone()
    out[:, :n_ids] = null_condition_ids(info, n_ids, cond_ids.device)
    return out


def check_mask_conditioning(value, name: str = "mask_conditioning") -> bool:
    """generate() / score(): ``mask_conditioning`` must be a bool; anything else is a ValueError that names it."""
    if not isinstance(value, bool):
        raise ValueError(f"{name} must be a bool (True: decode under the training key mask), not {value!r}")
    return value


def _require_conditioning(token_sequences):
    """mask_conditioning=True on a model without a conditioning sequence: there is no position the rule could take out of the keys."""
    if len(token_sequences) < 2:
        raise ValueError("mask_conditioning: the key mask covers the conditioning sequences in front of the predicted one; this model has a "
                         "single token sequence and nothing to mask")


def stage_mask_conditioning(mask_conditioning):
    """MusicLM.forward's ``mask_conditioning`` per stage (_per_stage; None and a stage that is not named: off), every other value checked
    by check_mask_conditioning."""
    return _per_stage(mask_conditioning, lambda v, name: None if v is None else check_mask_conditioning(v, name), "mask_conditioning")


def live_conditioning(cond_ids: List[torch.Tensor], eos_ids, pad_id: int, batch: int, device):
    """THE rule of which conditioning positions are fed and attended (open_musiclm.py:358-371), stated once for the training forward
    (_prepare), generate() and score().  cond_ids: the flattened conditioning sequences [B, n_i] as they are fed -- after unique_consecutive
    and after the optional eos append.  live = (id != pad_id) & (id != eos_id of its sequence).  -> (the ids with every non-live position
    set to 0, the key mask [B, sum(n_i + 1)] bool, True = attend, with every sequence's start token in front of it as True).  The rows of
    the predicted sequence -- its start token, given ids (pads included), generated ids -- are always attended: the caller pads the
    mask with True for them."""
    out, pieces = [], []
    for t, eos in zip(cond_ids, eos_ids):
        live = (t != pad_id) & (t != eos)
        out.append(t.masked_fill(~live, 0))
        pieces.append(F.pad(live, (1, 0), value=True))            # the sequence's start token is always attended
    mask = torch.cat(pieces, dim=-1) if pieces else torch.empty((batch, 0), device=device, dtype=torch.bool)
    return out, mask


def twin_live_conditioning(cond_live: List[torch.Tensor], mask: torch.Tensor, info: TokenSequenceInfo, n_ids: int):
    """The null twin of a prompt under the key mask (the training rule of a dropped sample, ``mask[:, 1:1 + n0] |= dropped``): cond_live /
    mask as live_conditioning returned them for the prompt -> (the twin's ids: the null ids at the condition's n_ids id positions,
    everything else the prompt's zeroed ids; its mask: the prompt's with those n_ids positions attended)."""
    twin_mask = mask.clone()
    twin_mask[:, 1:1 + n_ids] = True
    return [null_twin(cond_live[0], info, n_ids)] + list(cond_live[1:]), twin_mask


def _require_condition(token_sequences, what: str):
    if len(token_sequences) < 2:
        raise ValueError(f"{what}: the condition is token sequence 0 in front of a predicted sequence; this model has a single token "
                         "sequence and nothing to drop or guide on")

# generate(return_logprobs=True): the two log-probabilities (include/omlm.h) of every id the call sampled, fp32 [B, time steps, Q] each
LogProbs = namedtuple("LogProbs", ["model", "sampled"])


def zero_logprobs_after_eos(values: torch.Tensor, ids: torch.Tensor, eos_id: int, keep_eos: bool) -> torch.Tensor:
    """values [B, n] beside the LAST n columns of ids [B, m >= n]: 0.0 wherever mask_out_after_eos_id replaces the id (everything after
    the first eos, and the eos itself unless it is kept), so that a sum over time is the log-probability of the kept part."""
    replaced = mask_out_after_eos_id(ids, eos_id, keep_eos=keep_eos) != ids
    n = values.shape[-1]
    return values.masked_fill(replaced[:, ids.shape[-1] - n:], 0.0)


@beartype_jit
class TokenConditionedTransformerWrapper(nn.Module):
    """open_musiclm.py:219-410."""

    def __init__(self, *, transformer: TokenConditionedTransformer, pad_id=-1, unique_consecutive=True,
                 cross_entropy_loss_weights: Optional[List[float]] = None, mask_prob=0.15, null_cond_prob=0.,
                 label_smoothing=0., z_loss=0.):
        """label_smoothing = eps in [0, 1) and z_loss = zeta >= 0 (extensions; default 0: off, the plain cross entropy and the launches it
        always made): the training loss of a live row becomes (1 - eps) nll + eps smooth + zeta lse^2 (include/omlm.h; eps is
        F.cross_entropy's label_smoothing over the codebook_size + 1 entries, zeta the z-loss of PaLM / T5X, which keeps log Z near 0 --
        what the 16-bit head logits of "fp16" / "fp16ff" want).  Both terms live in the cross-entropy kernels, forward and backward.
        Training mode only, like mask_prob, dropout and null_cond_prob: eval(), trainer.validate() and score() report the plain cross
        entropy, bit for bit what they report without the keywords, so valid_loss stays comparable across runs and is the plain-CE
        monitor of a regularised run.
        null_cond_prob (extension; default 0: off, nothing is drawn): the training side of classifier-free guidance.  In training mode
        sample b of a batch trains on the null condition (null_condition_ids at every id position of token sequence 0, ATTENDED; its
        appended eos, every other sequence and all labels untouched) iff u_b < null_cond_prob, u one torch.rand(B) drawn after the forgetful
        mask's randn.  A number in [0, 1) (1: every sample; tests).  eval() never drops.  ``generate(cond_scale=...)`` is meaningful only
        on weights trained with it."""
        super().__init__()
        self.null_cond_prob = ops.check_null_cond_prob(null_cond_prob)          # refused by name
        self.label_smoothing = ops.check_label_smoothing(label_smoothing)
        self.z_loss = ops.check_z_loss(z_loss)
        if self.null_cond_prob > 0:
            _require_condition(transformer.token_sequences, "null_cond_prob")
        self.transformer = transformer
        self.token_sequences = transformer.token_sequences
        self.unique_consecutive = unique_consecutive
        self.pad_id = pad_id
        self.cross_entropy_loss_weights = default(cross_entropy_loss_weights, [1 for _ in self.token_sequences])
        self.eos_ids = transformer.eos_ids
        self.mask_prob = mask_prob
        assert len(self.token_sequences) == len(self.eos_ids) == len(self.cross_entropy_loss_weights)

    @property
    def device(self):
        return next(self.parameters()).device

    def _loss_reg(self) -> dict:
        """label_smoothing / z_loss as loss_and_logits takes them: the constructor's values in training mode, nothing in eval()."""
        return dict(label_smoothing=self.label_smoothing, z_loss=self.z_loss) if self.training else {}

    def new_metrics(self, top_k=None):
        """A zeroed metrics.QuantizerMetrics for this wrapper's token sequences and loss weights, on the model's device (no host sync).
        top_k: the k of its top-k counter (None: what the sampler keeps at the default filter_thres = 0.9)."""
        from .metrics import QuantizerMetrics
        return QuantizerMetrics.for_model(self.transformer, [float(w) for w in self.cross_entropy_loss_weights], top_k, self.device)

    def _metrics_arg(self, return_metrics, return_loss):
        """forward's ``return_metrics`` -> the QuantizerMetrics to accumulate onto, or None; refusals by name, before any device work."""
        from .metrics import QuantizerMetrics
        if return_metrics is None or return_metrics is False:
            return None
        if not return_loss:
            raise ValueError("return_metrics needs return_loss=True: the metrics are formed from the rows the loss walks")
        if isinstance(return_metrics, QuantizerMetrics):
            if (return_metrics.quantizers, return_metrics.vocab, return_metrics.weights) != \
                    ([s.num_quantizers for s in self.token_sequences], [s.codebook_size + 1 for s in self.token_sequences],
                     [float(w) for w in self.cross_entropy_loss_weights]):
                raise ValueError("return_metrics: the QuantizerMetrics given describes other token sequences or loss weights than this wrapper's")
            return return_metrics
        if return_metrics is True:
            return self.new_metrics()
        raise ValueError(f"return_metrics must be False, True or a QuantizerMetrics, not {return_metrics!r}")

    @eval_decorator
    @torch.no_grad()
    def generate(self, *, conditioning_token_ids: List[torch.Tensor], pred_token_ids: Optional[torch.Tensor] = None,
                 max_time_steps=512, filter_thres=0.9, temperature=1., include_eos_in_output=False,
                 append_eos_to_conditioning_tokens=True, allow_eos_in_output=False, uniforms=None, sampler_rng=None,
                 sampler_seed=None, top_p=None, kv_cache=None, return_logprobs=False, cond_scale=None, mask_conditioning=False, **kwargs):
        """AR sampling (open_musiclm.py:253-326).  Every step re-runs the full causal forward over the grown
        sequence like the reference (results are identical to a KV-cached decode because the stack is strictly
        causal); only the last position's logits are formed, and eos suppression + top-k + Gumbel-argmax run in
        one sampler kernel.  ``uniforms`` ([steps, B, V+1]) injects the uniform draws (tests).
        ``sampler_rng``: "buffer" draws every uniform of the call up front (torch.rand, [ids, B, V+1] floats); "counter" forms them in the
        sampler kernel from the stream of include/omlm.h, seeded by ``sampler_seed`` (None: drawn from torch's generator on the model's
        device, so torch.manual_seed governs the call either way) -- no buffer, and ids that do not depend on how the batch is cut into
        decode calls.  None: "buffer" unless the buffer would exceed decode.UNIFORM_BUFFER_MAX_BYTES (decode.sampler_rng_choice).
        ``top_p``: nucleus sampling inside the top-k set (include/omlm.h) -- of the k kept logits, ranked by value, only those are sampled
        whose preceding softmax mass (at ``temperature``) is below top_p of the kept mass.  A number in (0, 1]; None or 1: off, the call
        is the one it is without the argument.  Works on every route and with every source of uniforms.
        ``kv_cache``: element type of the cached decode's K/V cache -- None or "fp32", or "operand": the precision's 16-bit operand type
        (decode.kv_cache_choice; fp32 for "bf16x3").  The cached values are 16-bit numbers either way, so the ids are the same and the
        cache takes half the bytes (decode.cache_bytes).  On the re-forward route there is no cache and the value has no effect.
        ``return_logprobs``: returns ``(ids, LogProbs(model, sampled))`` -- fp32 [B, max_time_steps - first_step, Q] each, on the model's
        device, for the ids THIS call sampled (not a supplied ``pred_token_ids``): ``model`` is the log-probability of the id under the
        model's own distribution (T = 1, all entries), ``sampled`` under the distribution it was drawn from (top-k, nucleus,
        temperature, eos rule) -- include/omlm.h.  The sampler kernels write them in the launch that picks the id, on every route and with
        every source of uniforms; the flag changes no id.  Where the returned id is the after-eos mask value both numbers are 0.0.
        ``cond_scale`` = s: classifier-free guidance on the condition, token sequence 0 (include/omlm.h).  Every prompt is decoded beside
        its null twin (null_twin: the pad embedding's zero row at every id position of the condition, everything else the same) and the
        ids are sampled from g = null + s (cond - null), formed in fp32 by omlm_guide_logits; top-k, nucleus, temperature, the eos rule
        and both log-probabilities apply to g (``LogProbs.model`` is then the log-softmax of g).  A finite number >= 0; None or 1: off,
        the call launches exactly what it launches without the argument.  A guided call of P prompts is a decode call of 2P rows, so a
        decode call holds decode.max_call_batch // 2 prompts; uniforms (``uniforms``: [steps, P, V+1]), ids and log-probabilities cover
        the P prompts only.  Meaningful only on weights trained with ``null_cond_prob``: any other checkpoint has never seen the null
        condition.
        Per-row settings: ``temperature``, ``filter_thres``, ``top_p``, ``cond_scale`` and ``sampler_seed`` each take a number, as above,
        or a list / tuple / 1-D tensor of length B with one value per row (ranges as for the numbers; a wrong length or a bad entry raises a
        ValueError that names the argument, before any device work).  The rows of one call are then sampled each in its own way by the same
        launches (omlm_sample_rows, omlm_guide_logits_rows; include/omlm.h) on every route, with every source of uniforms and with
        ``return_logprobs``; row r gets what a call with row r's numbers gives it.  A per-row ``cond_scale`` decodes every row beside its
        null twin, the rows of scale 1 included: such a row's g is formed by the rule above and is not promised to equal the unguided call.
        A per-row ``sampler_seed`` needs the counter stream (``sampler_rng`` None chooses it; "buffer" or injected ``uniforms`` are
        refused): every row then draws u(t, 0, c) of its own seed, what a one-sample call with that seed draws, so a row's uniforms depend on
        its seed alone, not on its place in the batch or on its neighbours.  Its ids equal that one-sample call's wherever the step kernels
        give a row the same logits at both batch sizes -- not promised between B = 1 and B >= 2 at dim 1024, where different kernels run.
        With a number the stream index stays the global sample index.
        ``mask_conditioning`` (a bool; False, the default: the reference's sampler, which passes no key mask, and exactly the launches of
        a call without the argument): True decodes under the key mask of the training forward (live_conditioning) -- every conditioning
        position that holds a pad or an eos id, the appended eos included, is fed as id 0 and is no key; start tokens, given
        ``pred_token_ids`` (their pads too) and every generated row are attended.  The ids are then sampled from the distribution that
        training, validate() and the per-quantizer metrics describe.  On the cached route the prefill runs under the mask and every step
        goes through omlm_decode_step_masked (captured cycles included); the re-forward route grows the mask by one attended column per id.
        Works with every source of uniforms, ``top_p``, ``return_logprobs``, per-row settings, ``kv_cache`` and ``cond_scale`` -- a null
        twin takes its prompt's mask with the condition's id positions attended (twin_live_conditioning), as a dropped training sample does.
        With ``append_eos_to_conditioning_tokens=False`` the rule applies to the ids as given, like forward(input_has_eos=True)."""
        if check_mask_conditioning(mask_conditioning):                        # refused by name before any device work
            _require_conditioning(self.token_sequences)
        # rows of the call, as the checks below need them (no conditioning sequence: a model the checks further down refuse or serve as before)
        batch = conditioning_token_ids[0].shape[0] if len(conditioning_token_ids) else (pred_token_ids.shape[0] if exists(pred_token_ids) else 0)
        pred_info, pred_eos_id = self.token_sequences[-1], self.eos_ids[-1]
        V1, Q = pred_info.codebook_size + 1, pred_info.num_quantizers

        def model_checks(guidance):
            if guidance is not None:
                _require_condition(self.token_sequences, "cond_scale")
            assert len(conditioning_token_ids) == len(self.token_sequences) - 1
            ops.check_sampler_width(V1)
        # every sampling argument, checked before any device work
        s = ops.SamplerSettings.checked(batch, V1, temperature=temperature, filter_thres=filter_thres, top_p=top_p, cond_scale=cond_scale,
                                        sampler_seed=sampler_seed, logprobs=return_logprobs, after_guidance=model_checks)
        if isinstance(s.seed, list):
            decode.sampler_rng_choice(sampler_rng, 0, batch, 1, False)          # an unknown sampler_rng is refused as in every call
            if sampler_rng == "buffer" or exists(uniforms):
                raise ValueError("a per-row sampler_seed seeds the counter stream: it cannot be combined with sampler_rng='buffer' or "
                                 "injected uniforms (sampler_rng=None or 'counter', uniforms=None)")
            sampler_rng = "counter"
        decode.kv_cache_choice(kv_cache, self.transformer._precision())         # likewise: a ValueError names the accepted values
        batch, device = conditioning_token_ids[0].shape[0], self.device
        if exists(pred_token_ids):
            assert pred_token_ids.shape[0] == batch
            first_step = pred_token_ids.shape[1]
            sampled = _flat(pred_token_ids).to(device).long()
        else:
            first_step = 0
            sampled = torch.empty((batch, 0), device=device, dtype=torch.long)
        cond, twin = self._condition_rows(conditioning_token_ids, append_eos_to_conditioning_tokens, s.guidance is not None)
        masks = None
        if mask_conditioning:
            cond, twin, masks = self._masked_condition_rows(cond, twin, append_eos_to_conditioning_tokens)
        if pred_info.unique_consecutive:
            sampled = batch_unique_consecutive(sampled, pad_value=self.pad_id)

        n_new = max(max_time_steps - first_step, 0) * Q
        prompt_rows = sum(t.shape[-1] + 1 for t in cond) + 1 + sampled.shape[-1]
        counter = decode.sampler_rng_choice(sampler_rng, n_new, batch, V1, exists(uniforms) or UNIFORM_SOURCE is not None) == "counter"
        if counter and s.seed is None and n_new > 0:
            s = s._replace(seed=int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), device=device, dtype=torch.long)) & 0xFFFFFFFFFFFFFFFF)
        # where the uniforms come from, for either route: None -- the counter stream, formed in the sampler kernel; a tensor
        # [n_new, B, V1] -- injected, or UNIFORM_SOURCE's; _DEVICE_RNG -- the route draws them from torch's generator on the device
        if counter:
            U = None
        elif exists(uniforms):
            U = uniforms
        elif UNIFORM_SOURCE is not None and n_new > 0:
            U = UNIFORM_SOURCE(n_new, batch, V1)
        else:
            U = _DEVICE_RNG
        use_cache = kwargs.pop('use_cache', True) and decode.supports(self.transformer, 1, prompt_rows=prompt_rows) and n_new > 0
        if use_cache and s.guidance is not None:       # a pair is two rows of a decode call; where no call holds two, the re-forward route
            use_cache = decode.supports(self.transformer, 2, self.transformer._precision(), prompt_rows=prompt_rows, wide=True)
        if use_cache:
            new, lps = self._generate_cached(cond, twin, sampled, s, U, n_new, prompt_rows + n_new, allow_eos_in_output,
                                             kwargs.pop('use_graph', False), {} if kv_cache is None else dict(kv_cache=kv_cache), masks)
        else:
            new, lps = self._generate_reforward(cond, twin, sampled, s, U, n_new, allow_eos_in_output, masks)
        sampled = torch.cat((sampled, new), dim=-1)
        if return_logprobs:
            lps = LogProbs(*(zero_logprobs_after_eos(v, sampled, pred_eos_id, include_eos_in_output).reshape(batch, -1, Q) for v in lps))
        sampled = mask_out_after_eos_id(sampled, pred_eos_id, keep_eos=include_eos_in_output)
        if return_logprobs:
            return sampled.reshape(batch, -1, Q), lps
        return sampled.reshape(batch, -1, Q)

    def _condition_rows(self, conditioning_token_ids, append_eos: bool, guided: bool):
        """The conditioning sequences as generate() and score() feed them -> (cond, twin): on the device, unique_consecutive where the
        sequence asks for it, the eos appended (``append_eos``).  ``guided``: flattened, and ``twin`` is the same list with the null twin
        (null_twin) in place of the condition -- only the condition differs between a prompt and its twin; otherwise ``twin`` is None."""
        cond = [t.to(self.device) for t in conditioning_token_ids]
        for i, info in enumerate(self.token_sequences[:-1]):
            if info.unique_consecutive:
                cond[i] = batch_unique_consecutive(cond[i], pad_value=self.pad_id)
        n_cond_ids = _flat(cond[0]).shape[-1] if guided else 0      # id positions of the condition (before its eos)
        if append_eos:
            cond = [append_eos_id(_flat(t).long(), e) for t, e in zip(cond, self.eos_ids)]
        if not guided:
            return cond, None
        cond = [_flat(t).long() for t in cond]
        return cond, [null_twin(cond[0], self.token_sequences[0], n_cond_ids)] + cond[1:]

    def _masked_condition_rows(self, cond, twin, append_eos: bool):
        """mask_conditioning=True: (cond, twin) of _condition_rows -> (cond, twin, (mask, twin_mask)) under the training key mask -- the ids
        with every non-live position zeroed and the [B, conditioning rows] bool masks of live_conditioning / twin_live_conditioning
        (twin and twin_mask None where the call is not guided).  The predicted sequence's rows are not in the masks: _rows_mask adds them."""
        cond = [_flat(t).long() for t in cond]              # (at least one sequence: generate() and score() refuse the flag otherwise)
        cond, mask = live_conditioning(cond, self.eos_ids, self.pad_id, cond[0].shape[0], self.device)
        if twin is None:
            return cond, None, (mask, None)
        n_cond_ids = cond[0].shape[-1] - (1 if append_eos else 0)
        twin, twin_mask = twin_live_conditioning(cond, mask, self.token_sequences[0], n_cond_ids)
        return cond, twin, (mask, twin_mask)

    @staticmethod
    def _rows_mask(mask: torch.Tensor, n_pred: int) -> torch.Tensor:
        """A conditioning mask grown by the predicted sequence's start token and its n_pred ids, all attended: the key mask of the rows."""
        return F.pad(mask, (0, 1 + n_pred), value=True)

    def _generate_cached(self, cond, twin, sampled, s, U, n_new, rows, allow_eos, use_graph, kv_kw, masks=None):
        """generate()'s KV-cached route (decode.py): one new row per sampled id instead of the reference's full re-forward; the ids are
        sampled straight into a [steps, B] buffer that the next decode step reads.  -> (the new ids [B, n_new], the two log-probability
        planes [B, n_new] or None).  A decode call holds up to decode.max_call_batch samples (64 on the matrix-core step kernels, which
        carry four groups of 16 through every launch) -- guided: half as many pairs, rows [0, P) the prompts and rows [P, 2P) their null
        twins -- and larger batches run as consecutive calls: samples are independent, and every call streams the weights once per id.
        Arguments as generate() prepared them: ``cond`` / ``twin`` (_condition_rows), ``sampled`` (the given ids, [B, n0]), ``s`` (the
        call's ops.SamplerSettings), ``U`` (the source of uniforms), ``rows`` (prompt rows + n_new: what a decoder must hold), ``masks``
        (None, or _masked_condition_rows' pair: the decoders are then built with key_mask=True and prefilled under the rows' mask)."""
        batch, device, precision = sampled.shape[0], self.device, self.transformer._precision()
        Q, n0, guided = self.token_sequences[-1].num_quantizers, sampled.shape[-1], twin is not None
        if U is _DEVICE_RNG:
            U = torch.rand(n_new, batch, self.token_sequences[-1].codebook_size + 1, device=device)
        elif U is not None:
            U = U[:n_new].to(device).float().contiguous()
        forbid = [(not allow_eos) or (ind != Q - 1) for ind in range(Q)]
        group = decode.max_call_batch(self.transformer, precision) // (2 if guided else 1)
        pieces, lp_pieces = [], []
        for b0 in range(0, batch, group):
            b1 = min(batch, b0 + group)
            c = s.cut(b0, b1)
            prompt = [t[b0:b1] for t in cond] + [sampled[b0:b1]]
            if guided:
                prompt = [torch.cat((t, n[b0:b1]), dim=0) for t, n in zip(prompt, twin + [sampled])]
            if masks is None:
                dec = decode.CachedDecoder(self.transformer, (2 if guided else 1) * (b1 - b0), rows, precision, wide=True, **kv_kw)
                last = dec.prefill(prompt)
            else:
                km = torch.cat((masks[0][b0:b1], masks[1][b0:b1]), dim=0) if guided else masks[0][b0:b1]
                dec = decode.CachedDecoder(self.transformer, (2 if guided else 1) * (b1 - b0), rows, precision, wide=True, key_mask=True, **kv_kw)
                last = dec.prefill(prompt, key_mask=self._rows_mask(km, n0))
            # a keyword at its default is not passed.  Counter stream: sample b draws u(step, b, c) whichever piece it rides in
            loop_kw = dict(rng=(c.seed, b0)) if U is None else {}
            if s.logprobs:
                loop_kw.update(logprobs=True)
            if guided:
                loop_kw.update(guidance=c.guidance)
            loop = decode.SamplingLoop(dec, last, None if U is None else U[:, b0:b1].contiguous(), n0, n_new, c.k, c.temperature, forbid,
                                       use_graph=use_graph, top_p=c.top_p, **loop_kw)
            pieces.append(loop.run().t())                      # [b, n_new]
            if s.logprobs:
                lp_pieces.append((loop.lp_model.t(), loop.lp_sampled.t()))
        return torch.cat(pieces, dim=0), tuple(torch.cat(ps, dim=0) for ps in zip(*lp_pieces)) if s.logprobs else None

    def _generate_reforward(self, cond, twin, sampled, s, U, n_new, allow_eos, masks=None):
        """generate()'s re-forward route: every id re-runs the full causal forward over the grown sequence like the reference, one sampler
        call per id.  -> (the new ids [B, n_new], the two log-probability planes [B, n_new] or None).  Guided: one forward over 2B rows
        (the prompts, then their null twins), then the combine in place over the conditional half.  Arguments as for _generate_cached;
        per-row settings are uploaded once, here.  ``masks``: every forward runs under the rows' key mask, one attended column more per id."""
        batch, n0, device = sampled.shape[0], sampled.shape[-1], self.device
        Q, V1 = self.token_sequences[-1].num_quantizers, self.token_sequences[-1].codebook_size + 1
        nxt = torch.empty(batch, device=device, dtype=torch.long)
        # [ids, B]: row `step` is written by the launch that samples id `step`
        lps = tuple(torch.zeros(n_new, batch, device=device) for _ in range(2)) if s.logprobs else None
        if twin is not None:
            cond2 = [torch.cat((c, t), dim=0) for c, t in zip(cond, twin)]
        cmask = None if masks is None else torch.cat(masks, dim=0) if twin is not None else masks[0]
        up = s.upload(device)
        rows_kw = {f"row_{m}": t for m, t in up.tensors.items() if t is not None}

        def mask_arg(ids):          # () without a mask: the call it has always been
            return () if cmask is None else (self._rows_mask(cmask, ids.shape[-1]),)
        for step in (t * Q + ind for t in tqdm(range(n_new // Q), desc='generating predicted tokens') for ind in range(Q)):
            if twin is not None:
                both = self.transformer.last_logits(cond2 + [torch.cat((sampled, sampled), dim=0)], *mask_arg(sampled))
                last = both[:batch]
                ops.guide_logits(last, both[batch:], last, V1, up.guidance)
            else:
                last = self.transformer.last_logits(cond + [sampled], *mask_arg(sampled))
            if U is None:
                src = dict(seed=up.seed, step=step)
            elif U is _DEVICE_RNG:
                src = dict(uniform=torch.empty(batch, V1, device=device).uniform_(0, 1))
            else:
                src = dict(uniform=U[step].to(device).float().contiguous())
            lp = dict(lp_model=lps[0][step], lp_sampled=lps[1][step]) if s.logprobs else {}
            ops.sample(last, nxt, V1, up.k, up.temperature, (not allow_eos) or (step % Q != Q - 1), top_p=up.top_p, **src, **lp, **rows_kw)
            sampled = torch.cat((sampled, nxt[:, None]), dim=-1)
        return sampled[:, n0:], tuple(v.t() for v in lps) if s.logprobs else None

    @eval_decorator
    @torch.no_grad()
    def score(self, *, conditioning_token_ids: List[torch.Tensor], pred_token_ids: torch.Tensor,
              append_eos_to_conditioning_tokens=True, cond_scale=None, mask_conditioning=False) -> torch.Tensor:
        """The teacher-forced twin of ``generate(return_logprobs=True).model``: fp32 [B, T, Q], entry (b, t, q) the log-probability
        (lp_model of include/omlm.h: the model's own distribution, T = 1, all entries) of id ``pred_token_ids[b, t, q]`` given the
        conditioning and the ids before it -- under the logits ``transformer.last_logits(cond + [pred_flat[:, :t Q + q]])`` gives.
        One forward over the whole sequence with generate's semantics (no key mask, the conditioning eos appended and embedded);
        omlm_cross_entropy_fwd writes every row's log-sum-exp, the rest is a gather and a subtract.
        ``cond_scale`` = s (None or 1: off): the twin of ``generate(return_logprobs=True, cond_scale=s).model`` -- one forward over the 2B
        rows of prompts and null twins, omlm_guide_logits over every row, then the same; the log-softmax of g.
        ``mask_conditioning`` (a bool; False: off): the twin of ``generate(return_logprobs=True, mask_conditioning=True).model`` -- the one
        forward runs under generate's key mask (live_conditioning; every row of the predicted sequence attended)."""
        if check_mask_conditioning(mask_conditioning):                          # refused by name before any device work
            _require_conditioning(self.token_sequences)
        cond_scale = ops.check_cond_scale(cond_scale)                           # before any device work; None = off
        if cond_scale is not None:
            _require_condition(self.token_sequences, "cond_scale")
        assert len(conditioning_token_ids) == len(self.token_sequences) - 1
        pred_info = self.token_sequences[-1]
        assert not (self.unique_consecutive and pred_info.unique_consecutive), "score: a unique_consecutive predicted sequence has no [B, T, Q] form"
        hip.require_gpu(self.transformer.start_tokens[0], "model parameters")
        device, Q, V1 = self.device, pred_info.num_quantizers, pred_info.codebook_size + 1
        batch = pred_token_ids.shape[0]
        pred = _flat(pred_token_ids).to(device).long()                        # [B, T Q]
        L = pred.shape[-1]
        assert L % Q == 0 and all(t.shape[0] == batch for t in conditioning_token_ids)
        if L > 0 and bool(((pred < 0) | (pred >= V1)).any()):
            raise ValueError(f"score: pred_token_ids must lie in [0, {V1 - 1}] (the codebook and its eos); got "
                             f"[{int(pred.min())}, {int(pred.max())}]")
        if L == 0:
            return torch.zeros(batch, 0, Q, device=device)
        cond, twin = self._condition_rows(conditioning_token_ids, append_eos_to_conditioning_tokens, cond_scale is not None)
        kmask = None
        if mask_conditioning:
            cond, twin, masks = self._masked_condition_rows(cond, twin, append_eos_to_conditioning_tokens)
            kmask = self._rows_mask(torch.cat(masks, dim=0) if cond_scale is not None else masks[0], L)
        rows_pred = pred
        if cond_scale is not None:          # rows [0, B) the prompts, rows [B, 2B) their null twins
            cond = [torch.cat((c, t), dim=0) for c, t in zip(cond, twin)]
            rows_pred = torch.cat((pred, pred), dim=0)
        # row j of the predicted sequence (its start token, then the ids) holds the logits after pred[:, :j]: rows 0 .. L - 1 score the L ids,
        # the last row (what would follow them) carries the ignore label
        bufs, _, _ = engine.run_forward(self.transformer, cond + [rows_pred], kmask, True, False, self.transformer._precision())
        buf = bufs[-1]
        if cond_scale is not None:
            assert buf.shape[0] == 2 * batch * (L + 1), (buf.shape, batch, L)
            buf, null = buf[:batch * (L + 1)], buf[batch * (L + 1):]
            ops.guide_logits(buf, null, buf, V1, cond_scale)
        assert buf.shape[0] == batch * (L + 1), (buf.shape, batch, L)
        labels = F.pad(pred, (0, 1), value=-1).to(torch.int32).reshape(-1).contiguous()
        lse = torch.empty(buf.shape[0], device=device)
        ops.ce_fwd(buf, labels, lse, torch.zeros(1, device=device), V1)
        own = buf.view(batch, L + 1, -1)[:, :L].gather(2, pred[:, :, None]).squeeze(-1)
        return (own - lse.view(batch, L + 1)[:, :L]).reshape(batch, L // Q, Q)

    # ---- the trainers' optimizer-step path: id / label / mask construction as ONE kernel launch -------------------------------------
    def _fused_prepare_ok(self, all_token_ids, input_has_eos) -> bool:
        """return_loss=True, return_logits=False on GPU tensors without unique_consecutive sequences (shipped configs: False) and with the
        module's own generate_mask_with_prob (tests inject masks by replacing it: they take the torch path).  OMLM_FUSED_PREP=0: off."""
        if input_has_eos or os.environ.get("OMLM_FUSED_PREP", "1") == "0" or generate_mask_with_prob is not _GENERATE_MASK_ORIG:
            return False
        if self.unique_consecutive and any(info.unique_consecutive for info in self.token_sequences):
            return False
        n_tot = sum(int(t.numel() // t.shape[0]) + 1 for t in all_token_ids) + len(all_token_ids) - 1
        return all(t.is_cuda for t in all_token_ids) and n_tot <= 4096

    def _forward_loss_fused(self, all_token_ids, metrics=None):
        """Same arithmetic as _prepare + TokenConditionedTransformer.forward's id flattening + generate_mask_with_prob, in one launch
        (ops.prepare_train_batch); consumes the RNG exactly like the torch path (one randn of the mask's shape).  Labels come back as
        int32 tensors [B, len + 1]."""
        device = self.device
        ids = [_flat(t).to(device).long().contiguous() for t in all_token_ids]
        B = ids[0].shape[0]
        N = sum(t.shape[1] + 1 for t in ids) + len(ids) - 1
        scores, n_drop = None, 0
        if self.mask_prob > 0 and self.training:
            n_drop = min(int(N * self.mask_prob), N - 1)
            scores = torch.randn((B, N), device=device)
        null_kw = {}
        if self.null_cond_prob > 0 and self.training:      # the condition drop of _prepare: the same draw, in the same place
            null_kw = dict(null_u=torch.rand(B, device=device), null_p=self.null_cond_prob)
        weights = [float(w) for w in self.cross_entropy_loss_weights]
        seqs = self.token_sequences
        ids32, keymask, labels, lens = ops.prepare_train_batch(ids, [int(e) for e in self.eos_ids], [s.num_quantizers for s in seqs],
                                                               [s.codebook_size for s in seqs], self.pad_id, scores, n_drop,
                                                               [True] * len(ids), **null_kw)
        prepared = engine.PreparedIds(ids32, lens)
        ignore = [False] * len(ids)
        kw = self._loss_reg() if metrics is None else dict(self._loss_reg(), metrics=metrics)
        if torch.is_grad_enabled():
            loss, *logits = self.transformer.loss_and_logits(prepared, labels, keymask, weights, ignore, False, **kw)
        else:
            with torch.enable_grad():
                loss, *logits = self.transformer.loss_and_logits(prepared, labels, keymask, weights, ignore, False, **kw)
            loss = loss.detach()
        out = (loss, [l.transpose(1, 2) if l is not None else None for l in logits], labels)
        return out if metrics is None else (*out, metrics)

    def _prepare(self, all_token_ids, return_loss, input_has_eos):
        """eos append, labels, last-token drop, key mask (open_musiclm.py:340-376); in training mode with null_cond_prob > 0 the
        condition drop behind them (the constructor's docstring)."""
        batch, device = all_token_ids[0].shape[0], self.device
        ids = [_flat(t).to(device).long() for t in all_token_ids]
        if self.training:
            assert not input_has_eos, "train sequences (from clap, wav2vec, etc.) shouldn't come with an eos token"
        if not input_has_eos:
            ids = [append_eos_id(t, e) for t, e in zip(ids, self.eos_ids)]
        if self.unique_consecutive:
            for i, info in enumerate(self.token_sequences):
                if info.unique_consecutive:
                    ids[i] = batch_unique_consecutive(ids[i], pad_value=self.pad_id)
        labels = None
        if return_loss:
            labels = [t.clone() for t in ids]
            ids[-1] = ids[-1][:, :-1]
        ids[:-1], mask = live_conditioning(ids[:-1], self.eos_ids, self.pad_id, batch, device)
        mask = F.pad(mask, (0, ids[-1].shape[-1] + 1), value=True)   # predicted tokens + their start token
        forget = generate_mask_with_prob(mask.shape, self.mask_prob, device=mask.device) if self.mask_prob > 0 and self.training else None
        if self.null_cond_prob > 0 and self.training:
            # u is drawn after the forgetful mask's randn; a dropped sample's condition ids become the null ids and are attended
            n0 = ids[0].shape[-1] - (0 if input_has_eos else 1)               # id positions of the condition: not its appended eos
            dropped = torch.rand(batch, device=device) < self.null_cond_prob
            ids[0] = torch.where(dropped[:, None] & (torch.arange(ids[0].shape[-1], device=device) < n0)[None],
                                 null_twin(ids[0], self.token_sequences[0], n0), ids[0])
            mask[:, 1:1 + n0] |= dropped[:, None]
        if forget is not None:
            mask = mask & forget
        return ids, labels, mask

    def forward(self, *, all_token_ids: List[torch.Tensor], return_loss: bool = False, input_has_eos: bool = False,
                return_logits: bool = True, return_metrics=False, **kwargs):
        """return_logits=False (extension, return_loss=True only): the logits of sequences whose loss weight is 0 are not computed
        and come back as None -- the trainers' optimizer steps read only the loss (trainer.py:428-447).
        return_metrics (extension, return_loss=True only; False: off, the call launches exactly what it launches without the argument):
        True -- the result gains a fourth element, a metrics.QuantizerMetrics of this call: per weighted sequence and per quantizer the
        count, nll, entropy, top-1 and top-k hits of its rows, formed on the device by two launches behind the loss's own
        (csrc/ce_metrics.hip; include/omlm.h) -- no host sync; ``.to_dict()`` reads it.  A QuantizerMetrics (``new_metrics()``) -- accumulated onto
        and returned: what the trainer uses under HIP-graph capture, where the buffer exists before the capture and every replay adds to
        it.  Works on both preparation routes; loss, logits and gradients are bit for bit those of the call without it.  The metrics
        describe the PLAIN nll of the logits this call formed: in training mode those are the training-mode logits (dropout, the forgetful
        mask and the condition drop are on), and label smoothing and z-loss are not part of the numbers.  The padded labels of a
        unique_consecutive sequence are ignored rows, as in the loss."""
        assert len(all_token_ids) == len(self.token_sequences)
        metrics = self._metrics_arg(return_metrics, return_loss)
        if return_loss and not return_logits and self._fused_prepare_ok(all_token_ids, input_has_eos):
            return self._forward_loss_fused(all_token_ids, metrics)
        ids, labels, mask = self._prepare(all_token_ids, return_loss, input_has_eos)
        if not return_loss:
            return self.transformer(all_token_ids=ids, self_attn_mask=mask, **kwargs)
        weights = [float(w) for w in self.cross_entropy_loss_weights]
        # unique_consecutive sequences carry pad_id labels: F.cross_entropy(ignore_index=pad_id) and num_logits = (labels != pad_id)
        # .sum() in the reference (:396-404); the fused loss ignores negative labels and counts the rest on the device
        ignore = [bool(info.unique_consecutive and self.unique_consecutive) for info in self.token_sequences]
        loss_labels = [lb.masked_fill(lb == self.pad_id, -1) if ig else lb for lb, ig in zip(labels, ignore)]
        kw = self._loss_reg() if metrics is None else dict(self._loss_reg(), metrics=metrics)
        if torch.is_grad_enabled():
            loss, *logits = self.transformer.loss_and_logits(ids, loss_labels, mask, weights, ignore, return_logits, **kw)
        else:
            with torch.enable_grad():
                loss, *logits = self.transformer.loss_and_logits(ids, loss_labels, mask, weights, ignore, return_logits, **kw)
            loss = loss.detach()
        all_logits = [l.transpose(1, 2) if l is not None else None for l in logits]               # 'b n c -> b c n' (:389)
        return (loss, all_logits, labels) if metrics is None else (loss, all_logits, labels, metrics)


def create_semantic_transformer(dim=1024, depth=6, clap_codebook_size=1024, semantic_codebook_size=1024,
                                num_clap_quantizers=12, **kwargs):
    """open_musiclm.py:414-428"""
    seqs = [TokenSequenceInfo(clap_codebook_size, num_clap_quantizers, False),
            TokenSequenceInfo(semantic_codebook_size, 1, False)]
    return TokenConditionedTransformer(token_sequences=seqs, dim=dim, depth=depth, **kwargs)


def create_coarse_transformer(dim=512, depth=6, clap_codebook_size=1024, semantic_codebook_size=1024,
                              acoustic_codebook_size=1024, num_clap_quantizers=12, num_coarse_quantizers=4, **kwargs):
    """open_musiclm.py:432-450"""
    seqs = [TokenSequenceInfo(clap_codebook_size, num_clap_quantizers, False),
            TokenSequenceInfo(semantic_codebook_size, 1, False),
            TokenSequenceInfo(acoustic_codebook_size, num_coarse_quantizers, False)]
    return TokenConditionedTransformer(token_sequences=seqs, dim=dim, depth=depth, **kwargs)


def create_fine_transformer(dim=512, depth=6, clap_codebook_size=1024, acoustic_codebook_size=1024,
                            num_clap_quantizers=12, num_coarse_quantizers=4, num_fine_quantizers=8, **kwargs):
    """open_musiclm.py:454-472"""
    seqs = [TokenSequenceInfo(clap_codebook_size, num_clap_quantizers, False),
            TokenSequenceInfo(acoustic_codebook_size, num_coarse_quantizers, False),
            TokenSequenceInfo(acoustic_codebook_size, num_fine_quantizers, False)]
    return TokenConditionedTransformer(token_sequences=seqs, dim=dim, depth=depth, **kwargs)


def get_or_compute_clap_token_ids(clap_token_ids, clap, conditioning_audio, conditioning_text):
    """open_musiclm.py:476-485"""
    if not exists(clap_token_ids):
        assert exists(conditioning_audio) ^ exists(conditioning_text), "either condition on text or audio"
        assert exists(clap)
        clap_token_ids = clap(text_input=conditioning_text) if exists(conditioning_text) else clap(audio_input=conditioning_audio)
    return clap_token_ids


def get_or_compute_semantic_token_ids(semantic_token_ids, raw_audio, wav2vec):
    """open_musiclm.py:489-495"""
    if not exists(semantic_token_ids):
        assert exists(raw_audio)
        assert exists(wav2vec)
        semantic_token_ids = wav2vec(raw_audio, flatten=False)
    return semantic_token_ids


def get_or_compute_acoustic_token_ids(coarse_token_ids, fine_token_ids, raw_audio, neural_codec, num_coarse_quantizers: int):
    """open_musiclm.py:499-510"""
    if exists(raw_audio):
        assert not exists(coarse_token_ids) and not exists(fine_token_ids), "either provide coarse + fine ids or raw audio"
        assert exists(neural_codec), 'A neural audio codec must be provided if given raw wave for training'
        with torch.no_grad():
            neural_codec.eval()
            _, indices, _ = neural_codec(raw_audio, return_encoded=True)
            coarse_token_ids, fine_token_ids = indices[..., :num_coarse_quantizers], indices[..., num_coarse_quantizers:]
    return coarse_token_ids, fine_token_ids


class _Stage(nn.Module):
    """Shared plumbing of SemanticStage / CoarseStage / FineStage (open_musiclm.py:514-814)."""

    def _make_wrapper(self, transformer, pad_id, unique_consecutive, cross_entropy_loss_weights, mask_prob, null_cond_prob=0.,
                      label_smoothing=0., z_loss=0.):
        """label_smoothing / z_loss: the wrapper's training-mode loss terms (its constructor's docstring); eval() is the plain cross entropy."""
        self.transformer_wrapper = TokenConditionedTransformerWrapper(
            transformer=transformer, pad_id=pad_id, unique_consecutive=unique_consecutive,
            cross_entropy_loss_weights=cross_entropy_loss_weights, mask_prob=mask_prob, null_cond_prob=null_cond_prob,
            label_smoothing=label_smoothing, z_loss=z_loss)

    @property
    def device(self):
        return next(self.parameters()).device

    def _sample(self, conditioning, pred, max_time_steps, filter_thres, temperature, include_eos_in_output,
                append_eos_to_conditioning_tokens, **kwargs):
        return self.transformer_wrapper.generate(
            conditioning_token_ids=conditioning, pred_token_ids=pred, max_time_steps=max_time_steps,
            filter_thres=filter_thres, temperature=temperature, include_eos_in_output=include_eos_in_output,
            append_eos_to_conditioning_tokens=append_eos_to_conditioning_tokens, **kwargs)


def _split_logprobs(result, kwargs):
    """What wrapper.generate returned -> (ids, f): with return_logprobs among the stage's keyword arguments the wrapper returned
    (ids, LogProbs) and f(out) is (out, LogProbs) -- the stage's own result, ids or wave, beside them; otherwise f is the identity."""
    if kwargs.get("return_logprobs", False):
        ids, lps = result
        return ids, lambda out: (out, lps)
    return result, lambda out: out


class SemanticStage(_Stage):
    def __init__(self, *, semantic_transformer: TokenConditionedTransformer, wav2vec=None, clap=None, pad_id=-1,
                 unique_consecutive=False, cross_entropy_loss_weights: List[float] = None, mask_prob=0.15, null_cond_prob=0.,
                 label_smoothing=0., z_loss=0.):
        super().__init__()
        self.wav2vec, self.clap = wav2vec, clap
        num_semantic_tokens = semantic_transformer.token_sequences[1].codebook_size
        if exists(wav2vec):
            assert wav2vec.codebook_size == num_semantic_tokens, \
                f'num_semantic_tokens on SemanticTransformer must be set to {wav2vec.codebook_size}'
        self._make_wrapper(semantic_transformer, pad_id, unique_consecutive, cross_entropy_loss_weights, mask_prob, null_cond_prob,
                           label_smoothing, z_loss)

    @eval_decorator
    @torch.no_grad()
    def generate(self, *, conditioning_text=None, conditioning_audio=None, input_audio=None, clap_token_ids=None,
                 semantic_token_ids=None, filter_thres=0.9, temperature=1., max_time_steps=30 * 25,
                 include_eos_in_output=False, append_eos_to_conditioning_tokens=True, **kwargs):
        """``return_logprobs=True`` (like every sampling keyword, passed on to the wrapper): returns (ids, LogProbs).  ``cond_scale``
        (classifier-free guidance on the CLAP tokens) is such a keyword in every stage's generate.  ``temperature``, ``filter_thres``,
        ``top_p``, ``cond_scale`` and ``sampler_seed`` are handed on as they are in every stage's generate: a number, or one value per row
        (TokenConditionedTransformerWrapper.generate)."""
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, conditioning_audio, conditioning_text)
        if exists(semantic_token_ids) or exists(input_audio):
            semantic_token_ids = get_or_compute_semantic_token_ids(semantic_token_ids, input_audio, self.wav2vec)
        else:
            semantic_token_ids = None
        return self._sample([clap_token_ids], semantic_token_ids, max_time_steps, filter_thres, temperature,
                            include_eos_in_output, append_eos_to_conditioning_tokens, **kwargs)

    def forward(self, *, raw_wave_for_clap=None, raw_wave_for_semantic=None, clap_token_ids=None,
                semantic_token_ids=None, return_loss=False, **kwargs):
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, raw_wave_for_clap, conditioning_text=None)
        semantic_token_ids = get_or_compute_semantic_token_ids(semantic_token_ids, raw_wave_for_semantic, self.wav2vec)
        return self.transformer_wrapper.forward(all_token_ids=[clap_token_ids, semantic_token_ids],
                                                return_loss=return_loss, **kwargs)


class CoarseStage(_Stage):
    def __init__(self, *, coarse_transformer: TokenConditionedTransformer, wav2vec=None, clap=None, neural_codec=None,
                 pad_id=-1, unique_consecutive=False, cross_entropy_loss_weights: List[float] = None, mask_prob=0.15, null_cond_prob=0.,
                 label_smoothing=0., z_loss=0.):
        super().__init__()
        self.wav2vec, self.clap, self.neural_codec = wav2vec, clap, neural_codec
        num_semantic_tokens = coarse_transformer.token_sequences[1].codebook_size
        if exists(wav2vec):
            assert wav2vec.codebook_size == num_semantic_tokens, \
                f'num_semantic_tokens on CoarseTransformer must be set to {wav2vec.codebook_size}'
        self.num_coarse_quantizers = coarse_transformer.token_sequences[-1].num_quantizers
        self._make_wrapper(coarse_transformer, pad_id, unique_consecutive, cross_entropy_loss_weights, mask_prob, null_cond_prob,
                           label_smoothing, z_loss)

    @eval_decorator
    @torch.no_grad()
    def generate(self, *, semantic_token_ids, coarse_token_ids=None, conditioning_text=None, conditioning_audio=None,
                 clap_token_ids=None, filter_thres=0.9, temperature=1., max_time_steps=10 * 600,
                 include_eos_in_output=False, append_eos_to_conditioning_tokens=True, reconstruct_wave=False, **kwargs):
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, conditioning_audio, conditioning_text)
        sampled = self._sample([clap_token_ids, semantic_token_ids], coarse_token_ids, max_time_steps, filter_thres,
                               temperature, include_eos_in_output, append_eos_to_conditioning_tokens, **kwargs)
        sampled, with_lps = _split_logprobs(sampled, kwargs)
        if reconstruct_wave:
            assert exists(self.neural_codec)
            wave = self.neural_codec.decode_from_codebook_indices(sampled)
            return with_lps(wave.squeeze(1))
        return with_lps(sampled)

    def forward(self, *, raw_wave_for_clap=None, raw_wave_for_semantic=None, raw_wave_for_acoustic=None,
                clap_token_ids=None, semantic_token_ids=None, coarse_token_ids=None, return_loss=False, **kwargs):
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, raw_wave_for_clap, conditioning_text=None)
        semantic_token_ids = get_or_compute_semantic_token_ids(semantic_token_ids, raw_wave_for_semantic, self.wav2vec)
        coarse_token_ids, _ = get_or_compute_acoustic_token_ids(coarse_token_ids, None, raw_wave_for_acoustic,
                                                                self.neural_codec, self.num_coarse_quantizers)
        return self.transformer_wrapper.forward(all_token_ids=[clap_token_ids, semantic_token_ids, coarse_token_ids],
                                                return_loss=return_loss, **kwargs)


class FineStage(_Stage):
    def __init__(self, *, fine_transformer: TokenConditionedTransformer, clap=None, neural_codec=None, pad_id=-1,
                 unique_consecutive=False, cross_entropy_loss_weights: List[float] = None, mask_prob=0.15, null_cond_prob=0.,
                 label_smoothing=0., z_loss=0.):
        super().__init__()
        self.clap, self.neural_codec = clap, neural_codec
        self.num_coarse_quantizers = fine_transformer.token_sequences[1].num_quantizers
        self._make_wrapper(fine_transformer, pad_id, unique_consecutive, cross_entropy_loss_weights, mask_prob, null_cond_prob,
                           label_smoothing, z_loss)

    @eval_decorator
    @torch.no_grad()
    def generate(self, *, coarse_token_ids, fine_token_ids=None, conditioning_text=None, conditioning_audio=None,
                 clap_token_ids=None, filter_thres=0.9, temperature=1., max_time_steps=3 * 600,
                 include_eos_in_output=False, append_eos_to_conditioning_tokens=True, reconstruct_wave=False, **kwargs):
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, conditioning_audio, conditioning_text)
        sampled = self._sample([clap_token_ids, coarse_token_ids], fine_token_ids, max_time_steps, filter_thres,
                               temperature, include_eos_in_output, append_eos_to_conditioning_tokens, **kwargs)
        sampled, with_lps = _split_logprobs(sampled, kwargs)
        if reconstruct_wave:
            assert exists(self.neural_codec)
            wave = self.neural_codec.decode_from_codebook_indices(torch.cat((coarse_token_ids, sampled), dim=-1))
            return with_lps(wave.squeeze(1))
        return with_lps(sampled)

    def forward(self, *, raw_wave_for_clap=None, raw_wave_for_acoustic=None, clap_token_ids=None,
                coarse_token_ids=None, fine_token_ids=None, return_loss=False, **kwargs):
        clap_token_ids = get_or_compute_clap_token_ids(clap_token_ids, self.clap, raw_wave_for_clap, conditioning_text=None)
        coarse_token_ids, fine_token_ids = get_or_compute_acoustic_token_ids(
            coarse_token_ids, fine_token_ids, raw_wave_for_acoustic, self.neural_codec, self.num_coarse_quantizers)
        assert exists(coarse_token_ids) and exists(fine_token_ids)
        return self.transformer_wrapper.forward(all_token_ids=[clap_token_ids, coarse_token_ids, fine_token_ids],
                                                return_loss=return_loss, **kwargs)


def _windows(t: torch.Tensor, size: int, step: int):
    """[B, T, ...] -> list of [B, size, ...] windows at stride `step` (tensor.unfold semantics, :958-959)."""
    n = (t.shape[1] - size) // step + 1
    return [t[:, i * step: i * step + size] for i in range(max(n, 0))]


def _stack_windows(windows: List[torch.Tensor]) -> torch.Tensor:
    """W windows [B, ...] -> [W * B, ...] along the batch axis: window w of sample b is row w * B + b."""
    return torch.cat(list(windows), dim=0)


def _unstack_windows(stacked: torch.Tensor, n_windows: int) -> List[torch.Tensor]:
    """Inverse of _stack_windows: [W * B, ...] -> W tensors [B, ...] in window order."""
    assert n_windows > 0 and stacked.shape[0] % n_windows == 0, (stacked.shape, n_windows)
    return list(stacked.split(stacked.shape[0] // n_windows, dim=0))


def _per_stage(value, check, name):
    """(semantic, coarse, fine) values of a MusicLM.forward argument `name` for the stages' generate(): None, a number for all three, or a
    mapping with any of "semantic" / "coarse" / "fine".  Every value goes through check(value, name); a ValueError names what is wrong."""
    stages = ("semantic", "coarse", "fine")
    if isinstance(value, Mapping):
        unknown = sorted(set(value) - set(stages), key=str)
        if unknown:
            raise ValueError(f"{name}: unknown stage(s) {unknown}; a mapping takes any of {list(stages)}")
        for stage in stages:
            check(value.get(stage), f"{name}[{stage!r}]")
        return tuple(value.get(stage) for stage in stages)
    check(value, name)
    return (value,) * 3


def stage_top_p(top_p):
    """MusicLM.forward's ``top_p`` per stage (_per_stage), every value checked by ops.check_top_p."""
    return _per_stage(top_p, ops.check_top_p, "top_p")


def stage_cond_scale(cond_scale):
    """MusicLM.forward's ``cond_scale`` per stage (_per_stage; a stage that is not named decodes unguided), every value checked by
    ops.check_cond_scale."""
    return _per_stage(cond_scale, ops.check_cond_scale, "cond_scale")


class MusicLM(nn.Module):
    """open_musiclm.py:818-1071: hierarchical semantic -> coarse -> fine sliding-window decode.

    Extensions over the reference signature (all optional, defaults reproduce the reference):
      clap_token_ids  -- bypass the CLAP text tower with pre-quantised conditioning ids (synthetic benchmarks);
      return_tokens   -- return (semantic, coarse, fine) id tensors instead of decoding a waveform;
      fine_windows_together -- a permission, not a demand: where the fine windows do not depend on each other (no overlap, i.e.
                         fine_sliding_window_step_percent == 1, and no primed fine ids) they may be generated in ONE fine.generate call,
                         stacked along the batch axis (window w of prompt b is sample w * B + b; a decode call carries up to
                         decode.max_call_batch samples), instead of one call per window.  Everywhere else the flag changes nothing
                         and the windows run one after the other.  Each sample sees the same conditioning either way, but the default
                         random stream is consumed in a different order (one [steps, W * B, V] draw instead of W draws of
                         [steps, B, V]), so sampled ids differ from the sequential call's unless the uniforms are injected.
                         Default False: the reference's call-by-call structure.
      sampler_rng     -- handed to every stage's generate(): "buffer", "counter" or None (TokenConditionedTransformerWrapper.generate).
                         With "counter" each generate call draws its own seed from torch's generator; inside one call a sample's
                         uniforms depend on its index in that call alone, not on how the call is cut into decode calls.
      top_p           -- nucleus sampling in every stage's generate(): a number in (0, 1] for all three stages, or a mapping with any of
                         "semantic" / "coarse" / "fine" (a stage that is not named samples without a nucleus).  None: off.
      kv_cache        -- handed to every stage's generate(): None / "fp32", or "operand" to keep the cached decode's keys and values in the
                         precision's 16-bit operand type -- the same ids from half the cache bytes (decode.cache_bytes sizes a call).
      cond_scale      -- classifier-free guidance on the CLAP tokens in every stage's generate() (TokenConditionedTransformerWrapper
                         .generate): a finite number >= 0 for all three stages, or a mapping with any of "semantic" / "coarse" / "fine"
                         (a stage that is not named decodes unguided).  None or 1: off.  Each guided decode call carries a prompt and
                         its null twin, so fine_windows_together stacks half as many windows into one decode call.  Meaningful only on
                         stages trained with null_cond_prob.
      mask_conditioning -- decode under the training key mask in every stage's generate() (TokenConditionedTransformerWrapper.generate):
                         a bool for all three stages, or a mapping with any of "semantic" / "coarse" / "fine" (a stage that is not
                         named decodes as the reference does).  None or False: off.
    ``generate`` is an alias of ``forward``."""

    def __init__(self, *, wav2vec=None, clap=None, neural_codec=None, semantic_transformer: TokenConditionedTransformer,
                 coarse_transformer: TokenConditionedTransformer, fine_transformer: TokenConditionedTransformer):
        super().__init__()
        assert semantic_transformer.token_sequences[1].codebook_size == coarse_transformer.token_sequences[1].codebook_size
        assert coarse_transformer.token_sequences[2].codebook_size == fine_transformer.token_sequences[2].codebook_size
        assert coarse_transformer.token_sequences[2].num_quantizers == fine_transformer.token_sequences[1].num_quantizers
        self.semantic = SemanticStage(semantic_transformer=semantic_transformer, wav2vec=wav2vec, clap=clap)
        self.coarse = CoarseStage(coarse_transformer=coarse_transformer, wav2vec=wav2vec, clap=clap, neural_codec=neural_codec)
        self.fine = FineStage(fine_transformer=fine_transformer, clap=clap, neural_codec=neural_codec)
        self.wav2vec, self.clap, self.neural_codec = wav2vec, clap, neural_codec

    @property
    def device(self):
        return next(self.parameters()).device

    @eval_decorator
    @torch.no_grad()
    def forward(self, *, text: Optional[List[str]] = None, prime_wave=None, prime_wave_sample_hz=None, output_seconds=8,
                semantic_window_seconds=10, coarse_window_seconds=4, fine_window_seconds=2,
                semantic_steps_per_second=50, acoustic_steps_per_second=75, return_coarse_generated_wave=False,
                mask_out_generated_fine_tokens=False, semantic_sliding_window_step_percent=0.5,
                coarse_sliding_window_step_percent=0.5, fine_sliding_window_step_percent=1,
                clap_token_ids=None, return_tokens=False, fine_windows_together=False, sampler_rng=None, top_p=None, kv_cache=None,
                cond_scale=None, mask_conditioning=None):
        top_ps, scales = stage_top_p(top_p), stage_cond_scale(cond_scale)          # refused by name before any work
        key_masks = stage_mask_conditioning(mask_conditioning)                     # likewise
        decode.check_kv_cache(kv_cache)                                            # likewise
        # the sampling keywords of each stage's generate(); kv_cache and cond_scale only when given (a keyword at its default is not passed)
        kv_kw = {} if kv_cache is None else dict(kv_cache=kv_cache)
        kw_sem, kw_coarse, kw_fine = (dict(sampler_rng=sampler_rng, top_p=p, **kv_kw, **({} if g is None else dict(cond_scale=g)),
                                           **({} if m is None else dict(mask_conditioning=m)))
                                      for p, g, m in zip(top_ps, scales, key_masks))
        if not exists(clap_token_ids):
            assert exists(text), 'text needs to be passed in if one of the transformer requires conditioning'
            clap_token_ids = get_or_compute_clap_token_ids(None, self.clap, conditioning_audio=None, conditioning_text=text)

        sem_hz, ac_hz = semantic_steps_per_second, acoustic_steps_per_second
        # audio continuation (open_musiclm.py:896-926)
        prime_coarse_all = prime_fine_all = None
        prime_sem = prime_coarse = prime_fine = None
        sem_adjust = coarse_adjust = fine_adjust = 0
        if exists(prime_wave):
            from .utils import prepare_audio
            assert exists(prime_wave_sample_hz)
            wave_w2v = prepare_audio(prime_wave, prime_wave_sample_hz, self.wav2vec.target_sample_hz, normalize=True,
                                     target_length_seconds=semantic_window_seconds)
            wave_codec = prepare_audio(prime_wave, prime_wave_sample_hz, self.neural_codec.sample_rate, normalize=False,
                                       target_length_seconds=semantic_window_seconds)
            c_sem = get_or_compute_semantic_token_ids(None, wave_w2v, self.wav2vec)
            c_coarse, c_fine = get_or_compute_acoustic_token_ids(
                None, None, wave_codec, self.neural_codec, self.coarse.transformer_wrapper.token_sequences[2].num_quantizers)
            n_sem = int(sem_hz * semantic_window_seconds * (1 - semantic_sliding_window_step_percent))
            n_coarse = int(ac_hz * coarse_window_seconds * (1 - coarse_sliding_window_step_percent))
            n_fine = int(ac_hz * fine_window_seconds * (1 - fine_sliding_window_step_percent))
            prime_coarse_all, prime_fine_all = c_coarse, c_fine
            prime_sem = c_sem[:, -n_sem:] if c_sem.shape[1] >= n_sem else c_sem
            prime_coarse = c_coarse[:, -n_coarse:]
            prime_fine = c_fine[:, -n_fine:] if n_fine > 0 else None
            sem_adjust = n_sem - int(sem_hz * coarse_window_seconds * (1 - coarse_sliding_window_step_percent))
            coarse_adjust = n_coarse - int(ac_hz * fine_window_seconds * (1 - fine_sliding_window_step_percent))
            fine_adjust = n_fine

        # ---- semantic stage (:930-952): one window, then 50%-overlap continuation windows ----
        sem = self.semantic.generate(clap_token_ids=clap_token_ids, semantic_token_ids=prime_sem,
                                     max_time_steps=int(min(output_seconds, semantic_window_seconds) * sem_hz),
                                     include_eos_in_output=False, append_eos_to_conditioning_tokens=True, **kw_sem)
        while sem.shape[1] < int(output_seconds * sem_hz):
            keep = int(semantic_window_seconds * sem_hz * (1 - semantic_sliding_window_step_percent))
            nxt = self.semantic.generate(clap_token_ids=clap_token_ids, semantic_token_ids=sem[:, -keep:],
                                         max_time_steps=int(semantic_window_seconds * sem_hz),
                                         include_eos_in_output=False, append_eos_to_conditioning_tokens=True, **kw_sem)
            sem = torch.cat([sem, nxt[:, keep:]], dim=1)
        sem_all = sem
        sem = sem[:, sem_adjust:]

        # ---- coarse stage (:956-984): semantic windows of coarse_window*50-1 ids at 50% stride ----
        win = int(coarse_window_seconds * sem_hz - 1)
        coarse = None
        for sem_win in _windows(sem, win, int(win * coarse_sliding_window_step_percent)):
            if exists(coarse):
                keep = int(coarse_window_seconds * ac_hz * (1 - coarse_sliding_window_step_percent))
                cond_coarse = coarse[:, -keep:]
            else:
                keep, cond_coarse = 0, prime_coarse
            pred = self.coarse.generate(clap_token_ids=clap_token_ids, semantic_token_ids=sem_win,
                                        coarse_token_ids=cond_coarse,
                                        max_time_steps=int(coarse_window_seconds * ac_hz), reconstruct_wave=False,
                                        include_eos_in_output=False, append_eos_to_conditioning_tokens=True,
                                        temperature=0.95, **kw_coarse)
            coarse = pred if not exists(coarse) else torch.cat([coarse, pred[:, keep:]], dim=1)
        if return_coarse_generated_wave:
            return self.neural_codec.decode_from_codebook_indices(coarse).squeeze(1)
        coarse = coarse[:, coarse_adjust:]

        # ---- fine stage (:996-1026): non-overlapping (100% stride) coarse windows ----
        fwin = int(fine_window_seconds * ac_hz)
        fstep = int(fwin * fine_sliding_window_step_percent)
        fine = None
        coarse_wins = _windows(coarse, fwin, fstep)
        if fine_windows_together and fstep == fwin and not exists(prime_fine) and len(coarse_wins) > 1:
            # independent windows (all coarse ids are known, keep == 0, no fine conditioning): one call over W * B samples
            pred = self.fine.generate(clap_token_ids=clap_token_ids.repeat(len(coarse_wins), *([1] * (clap_token_ids.dim() - 1))),
                                      coarse_token_ids=_stack_windows(coarse_wins), fine_token_ids=None,
                                      max_time_steps=fwin, reconstruct_wave=False, include_eos_in_output=False,
                                      append_eos_to_conditioning_tokens=True, temperature=0.4, **kw_fine)
            fine = torch.cat(_unstack_windows(pred, len(coarse_wins)), dim=1)
            coarse_wins = []
        for coarse_win in coarse_wins:
            if exists(fine):
                keep = int(fwin * (1 - fine_sliding_window_step_percent))
                cond_fine = fine[:, -keep:] if keep > 0 else None
            else:
                keep, cond_fine = 0, prime_fine
            pred = self.fine.generate(clap_token_ids=clap_token_ids, coarse_token_ids=coarse_win, fine_token_ids=cond_fine,
                                      max_time_steps=fwin, reconstruct_wave=False, include_eos_in_output=False,
                                      append_eos_to_conditioning_tokens=True, temperature=0.4, **kw_fine)
            fine = pred if not exists(fine) else torch.cat([fine, pred[:, keep:]], dim=1)
        fine = fine[:, fine_adjust:]
        if exists(prime_coarse_all) and exists(prime_fine_all):
            fine = torch.cat([prime_fine_all, fine], dim=1)
            coarse = torch.cat([prime_coarse_all, coarse], dim=1)
        if return_tokens:
            return sem_all, coarse, fine
        acoustic = torch.cat([coarse[:, : fine.shape[1]], fine], dim=-1) if coarse.shape[1] != fine.shape[1] \
            else torch.cat([coarse, fine], dim=-1)
        assert exists(self.neural_codec), "a neural codec is required to decode tokens to a waveform (or pass return_tokens=True)"
        return self.neural_codec.decode_from_codebook_indices(acoustic).squeeze(1)

    generate = forward

    @eval_decorator
    @torch.no_grad()
    def generate_top_match(self, *, text: List[str], num_samples=4, num_top_matches: int = 1, **kwargs):
        """open_musiclm.py:1039-1071: sample num_samples waves per prompt, rank by CLAP text/audio cosine similarity."""
        try:
            from torchaudio.functional import resample
        except ImportError as e:  # pragma: no cover
            raise ImportError("generate_top_match needs torchaudio to resample for CLAP") from e
        all_samples, all_similarities = [], []
        for prompt in text:
            batch_text = [prompt] * num_samples
            samples = self.forward(text=batch_text, **kwargs)
            text_latents = self.clap(text_input=[prompt], return_embedding=True).repeat(num_samples, 1)
            clap_input = int16_to_float32(float32_to_int16(resample(samples, self.neural_codec.sample_rate, self.clap.sample_rate)))
            audio_latents = self.clap(audio_input=clap_input, return_embedding=True)
            sim = F.cosine_similarity(text_latents, audio_latents, dim=-1)
            top = sim.topk(num_top_matches, dim=0, sorted=True).indices
            all_similarities.append(sim[top].detach().cpu())
            all_samples.append(samples[top])
        return all_samples, all_similarities
