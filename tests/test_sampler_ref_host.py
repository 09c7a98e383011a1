"""The sampler restatement of tests/loss_optim_sampler_ref.py without a GPU: on rows without ties it is the reference's own
top-k filter + Gumbel argmax (oracle.top_k_filter / oracle.gumbel_argmax); on tied rows it keeps the lowest indices, which
torch.topk does not promise -- the reason the GPU tests check the kernel against the restatement and not against torch.topk."""
import torch

import loss_optim_sampler_ref as R


def test_restatement_equals_oracle_on_rows_without_ties():
    from oracle import musiclm_oracle as O
    g = torch.Generator().manual_seed(11)
    for V, thres, T in ((1025, 0.9, 0.95), (64, 0.5, 1.0), (2048, 0.99, 2.0), (7, 0.0, 0.5)):
        logits = torch.randn(64, V, generator=g, dtype=torch.float64) * 4
        assert all(len(set(r.tolist())) == V for r in logits)             # no ties: the kept set is the same under any tie rule
        u = torch.rand(64, V, generator=g, dtype=torch.float64)
        k = max(int((1 - thres) * V), 1)
        want = O.gumbel_argmax(O.top_k_filter(logits, thres), u, T)
        assert torch.equal(R.sample(logits, u, k, T, False), want)
        last = logits.clone()
        last[:, -1] = float("-inf")
        assert torch.equal(R.sample(logits, u, k, T, True), O.gumbel_argmax(O.top_k_filter(last, thres), u, T))


def test_restatement_keeps_the_lowest_tied_indices():
    x = torch.tensor([[3., 1, 2, 2, 2, 2, 0, 2, 2, 2]])
    assert R.kept_mask(x, 3, False)[0].nonzero().flatten().tolist() == [0, 2, 3]
    assert R.kept_mask(x, 1, False)[0].nonzero().flatten().tolist() == [0]
    assert R.kept_mask(x, 10, True)[0].tolist() == [True] * 10              # k = V keeps everything, the forbidden -inf included
    # every kept entry -inf: index 0, like torch.argmax of an all -inf row
    assert int(R.sample(torch.tensor([[float("-inf")] * 4]), torch.full((1, 4), 0.5), 2, 1.0, False)) == 0


def test_loss_scale_restatement_clamps():
    s = [4.0, 0.0, 0.0, 0.0, 4.0]
    s = R.loss_scale_update(s, False, 2.0, 0.5, 3, 2.0, 16.0)
    assert s == [2.0, 0.0, 1.0, 0.0, 4.0]
    s = R.loss_scale_update(s, False, 2.0, 0.5, 3, 2.0, 16.0)
    assert s == [2.0, 0.0, 2.0, 0.0, 2.0]                                  # scale_min
    for _ in range(3):
        s = R.loss_scale_update(s, True, 2.0, 0.5, 3, 2.0, 16.0)
    assert s == [4.0, 0.0, 2.0, 3.0, 2.0]
