"""Bounds that the GPU op cases (tests/support_op_cases.py) assert, checked on the CPU against a plain torch restatement of what they bound."""
import torch

from tests.support_op_cases import dropout_mean_bound, dropout_std_bounds


def test_dropout_kept_mass_bound_holds_for_a_bernoulli_restatement():
    """the p = 0.25 case of t_mha: 64 queries x 2 batch elements x 12 heads, 96 keys, v = 1 -- softmax rows of random logits, a Bernoulli keep mask
    scaled by 1 / (1 - p); and the worst case of the bound, one-hot probabilities.  Twenty seeds each: a 6-sigma bound does not fail."""
    rows, Lk, p = 64 * 2 * 12, 96, 0.25
    bound = dropout_mean_bound(rows, p)
    assert 0.08 < bound < 0.09                                    # 6 sqrt(1 / (3 * 1536)) = 0.0884
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for trial in range(20):
        for probs in (torch.softmax(torch.randn(rows, Lk, generator=g, dtype=torch.float64), -1), torch.eye(Lk, dtype=torch.float64)[torch.randint(0, Lk, (rows,), generator=g)]):
            keep = (torch.rand(rows, Lk, generator=g) >= p).double() / (1.0 - p)
            out = (probs * keep).sum(-1)
            worst = max(worst, abs(out.mean().item() - 1.0))
            assert abs(out.mean().item() - 1.0) <= bound
            lo, hi = dropout_std_bounds(p, Lk)
            assert lo <= out.std().item() <= hi
            assert not lo <= probs.sum(-1).std().item() <= hi     # no dropout at all: every output exactly 1, std 0 -- outside the bounds
    assert worst > bound / 60                                     # the bound is not vacuous: one-hot rows come within an order of magnitude of one sigma
    assert dropout_mean_bound(rows, p, 2.0 ** -9) == bound + 2.0 ** -8
