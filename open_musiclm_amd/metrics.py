"""Per-quantizer loss, accuracy, label rank and entropy of a residual-codebook stage (extension; no reference counterpart).

The cross entropy of a stage is a mean over quantizers that learn at very different speeds: the first one quickly, the last ones near the
uniform log(codebook) for a long time.  ``QuantizerMetrics`` holds, per weighted token sequence and per quantizer, the sums the kernels of
csrc/ce_metrics.hip form on the device from the logits the loss has just walked (include/omlm.h: omlm_ce_metrics, omlm_ce_metrics_bins):
count, nll, entropy, top-1 hits (rank == 0) and top-k hits (rank < k_top: how often the true id survives the sampler's top-k filter).
Accumulating costs no host read; ``to_dict`` does the one read."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import ops

COUNT, NLL, ENTROPY, TOP1, TOPK = range(5)


def _ratio(a: float, c: float) -> Optional[float]:
    return None if c == 0 else a / c


class QuantizerMetrics:
    """One fp64 device tensor ``bins`` [nseq, Qmax + 1, 5]: for token sequence s, rows [0, Q_s) are its quantizers (position t of the
    sequence belongs to quantizer t mod Q_s), row Q_s is the eos bin (rows whose label is the eos entry, wherever they stand), and the five
    columns are {count, nll, entropy, top1, topk}.  Sequences of loss weight 0 stay zero and are not reported.

    quantizers / vocab / weights: per token sequence, the number of quantizers, the entries of a logits row (codebook_size + 1: the eos
    entry counts) and the cross-entropy loss weight.  top_k: the k of the top-k counter (ops.check_metrics_top_k; None: what the sampler
    keeps at the default filter_thres = 0.9, per sequence).  Constructing, ``accumulate``, ``zero_`` and ``add_`` never sync the host."""

    def __init__(self, quantizers: Sequence[int], vocab: Sequence[int], weights: Sequence[float], top_k=None, device=None):
        assert len(quantizers) == len(vocab) == len(weights) and len(quantizers) >= 1
        self.quantizers = [int(q) for q in quantizers]
        self.vocab = [int(v) for v in vocab]
        self.weights = [float(w) for w in weights]
        assert all(q >= 1 for q in self.quantizers) and all(v >= 1 for v in self.vocab)
        # refused by name before any device work; a sequence without weight is never accumulated: its k is the default
        self.k_top = [ops.check_metrics_top_k(top_k if w > 0 else None, v) for v, w in zip(self.vocab, self.weights)]
        self.bins = torch.zeros(len(self.quantizers), max(self.quantizers) + 1, 5, dtype=torch.float64, device=device)

    @classmethod
    def for_model(cls, model, weights: Sequence[float], top_k=None, device=None) -> "QuantizerMetrics":
        """For a TokenConditionedTransformer's token sequences, on the model's device."""
        seqs = model.token_sequences
        return cls([s.num_quantizers for s in seqs], [s.codebook_size + 1 for s in seqs], weights, top_k,
                   device if device is not None else model.device)

    def like(self) -> "QuantizerMetrics":
        """A zeroed object of the same layout on the same device."""
        out = object.__new__(QuantizerMetrics)
        out.quantizers, out.vocab, out.weights, out.k_top = list(self.quantizers), list(self.vocab), list(self.weights), list(self.k_top)
        out.bins = torch.zeros_like(self.bins)
        return out

    def same_layout(self, other: "QuantizerMetrics") -> bool:
        return (self.quantizers, self.vocab, self.weights, self.k_top) == (other.quantizers, other.vocab, other.weights, other.k_top)

    @property
    def weighted(self) -> List[int]:
        return [s for s, w in enumerate(self.weights) if w > 0]

    # ---- device side -------------------------------------------------------------------------------------------------------------
    def scratch(self, rows: int):
        """The per-row outputs of omlm_ce_metrics for up to `rows` rows: (nll fp32, rank int32, entropy fp32)."""
        dev = self.bins.device
        return (torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, device=dev))

    def accumulate(self, s: int, logits: torch.Tensor, labels: torch.Tensor, n: int, scratch=None):
        """The two launches for token sequence s: fp32 logits [B * n, ld] in [B, n] row order and int32 labels [B * n] (negative: ignored).
        Read-only on both; the bins of s grow.  scratch: what ``scratch`` returned for at least B * n rows (reusable across sequences)."""
        R, Q, V = logits.shape[0], self.quantizers[s], self.vocab[s]
        assert labels.dtype == torch.int32 and labels.numel() == R and logits.dtype == torch.float32
        nll, rank, ent = (t[:R] for t in (scratch if scratch is not None else self.scratch(R)))
        ops.ce_metrics(logits, labels, V, row_nll=nll, row_rank=rank, row_entropy=ent)
        ops.ce_metrics_bins(nll, rank, ent, labels, n, Q, V, self.k_top[s], self.bins[s, :Q + 1])

    def zero_(self) -> "QuantizerMetrics":
        self.bins.zero_()
        return self

    def add_(self, other: "QuantizerMetrics") -> "QuantizerMetrics":
        if not self.same_layout(other):
            raise ValueError("QuantizerMetrics.add_: the two objects describe different sequences, weights or top_k")
        self.bins.add_(other.bins.to(self.bins.device))
        return self

    # ---- host side: each of these is ONE read of the device tensor ---------------------------------------------------------------
    def _host(self) -> torch.Tensor:
        return self.bins.detach().cpu()

    def loss(self, host: Optional[torch.Tensor] = None) -> Optional[float]:
        """sum_s w_s NLL_s / sum_s count_s over the weighted sequences: the plain cross entropy, which the scalar loss reports when
        label_smoothing = z_loss = 0.  None when nothing was counted."""
        h = self._host() if host is None else host
        num = sum(self.weights[s] * float(h[s, :self.quantizers[s] + 1, NLL].sum()) for s in self.weighted)
        return _ratio(num, sum(float(h[s, :self.quantizers[s] + 1, COUNT].sum()) for s in self.weighted))

    def to_dict(self, prefix: str = "", host: Optional[torch.Tensor] = None) -> dict:
        """Plain floats per weighted sequence: for quantizer i ``{prefix}loss_q{i}`` (mean nll), ``accuracy_q{i}`` (top-1), ``top{k}_accuracy_q{i}``,
        ``entropy_q{i}`` (mean, nats) and ``count_q{i}``; the same with ``_eos`` for the eos bin and with ``_total`` over all bins of the
        sequence.  With more than one weighted sequence the names carry the sequence index: ``{prefix}seq{s}_loss_q{i}``.  A mean over an
        empty bin is None, not NaN.  host: a copy ``_host()`` returned, to share one read between several of these methods."""
        h = self._host() if host is None else host
        many = len(self.weighted) > 1
        out = {}
        for s in self.weighted:
            Q, k = self.quantizers[s], self.k_top[s]
            p = f"{prefix}seq{s}_" if many else prefix
            rows = [(f"q{i}", h[s, i]) for i in range(Q)] + [("eos", h[s, Q]), ("total", h[s, :Q + 1].sum(0))]
            for name, r in rows:
                c = float(r[COUNT])
                out[f"{p}loss_{name}"] = _ratio(float(r[NLL]), c)
                out[f"{p}accuracy_{name}"] = _ratio(float(r[TOP1]), c)
                out[f"{p}top{k}_accuracy_{name}"] = _ratio(float(r[TOPK]), c)
                out[f"{p}entropy_{name}"] = _ratio(float(r[ENTROPY]), c)
                out[f"{p}count_{name}"] = c
        return out
