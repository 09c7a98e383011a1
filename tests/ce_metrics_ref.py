"""fp64 / numpy restatement of the row rule and the bin rule of include/omlm.h (omlm_ce_metrics, omlm_ce_metrics_bins).  No project code."""
import numpy as np


def rows(x, labels):
    """x [R, V] (any real dtype, taken as fp64), labels [R] ints -> (nll fp64 [R], rank int64 [R], entropy fp64 [R]).
    Ignored rows (label < 0) and rows whose label is >= V: 0, -1, 0."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    R, V = x.shape
    nll, rank, ent = np.zeros(R), np.full(R, -1, dtype=np.int64), np.zeros(R)
    for r in range(R):
        y = int(labels[r])
        if y < 0 or y >= V:
            continue
        l = x[r]
        mx = l.max()
        with np.errstate(invalid="ignore", over="ignore"):
            d = l - mx
            e = np.exp(d)
            s = e.sum()
            ed = np.where(e > 0, e * np.where(e > 0, d, 0.0), 0.0).sum()          # a column with e == 0 adds exactly 0
            nll[r] = (mx + np.log(s)) - l[y]
        rank[r] = int((l > l[y]).sum()) + int((l[:y] == l[y]).sum())
        ent[r] = np.log(s) - ed / s
    return nll, rank, ent


def bins(nll, rank, ent, labels, n, Q, V, k_top):
    """[Q + 1, 5] fp64 {count, nll, entropy, top1, topk}: rows in [B, n] order, t = r mod n, bin Q for the eos label V - 1, t mod Q otherwise."""
    labels = np.asarray(labels).astype(np.int64)
    out = np.zeros((Q + 1, 5))
    assert len(labels) % n == 0
    for r, y in enumerate(labels):
        if y < 0 or y >= V:
            continue
        b = Q if y == V - 1 else (r % n) % Q
        out[b] += (1.0, float(nll[r]), float(ent[r]), float(rank[r] == 0), float(rank[r] < k_top))
    return out
