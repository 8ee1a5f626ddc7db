"""CPU tests of train_step.row_weight: the factor a rank's mean loss over its real rows is differentiated with, so that the gradient exchange's
mean over the ranks is the mean over the real rows of all ranks."""
import pytest
import torch


def test_values():
    from facialmmt_amd.train_step import row_weight
    assert row_weight(2, 2, 3) == 2 * 2 / 3
    assert row_weight(1, 2, 3) == 1 * 2 / 3
    assert row_weight(1, 2, None) == 1.0
    assert row_weight(4, 1, 4) == 1.0                                       # one rank: its rows are all rows
    assert row_weight(2, 2, 4, 2) == 1.0 and row_weight(3, 2, 4, 4) == 1.5
    assert row_weight(2, 2, 3) + row_weight(1, 2, 3) == 2.0                 # the weights of a step sum to the world size


def test_every_bound_raises():
    from facialmmt_amd.train_step import row_weight
    for b in (0, -1):
        with pytest.raises(ValueError):
            row_weight(b, 2, 3)
        with pytest.raises(ValueError):
            row_weight(b, 2, None)                                           # a rank without a real row is not covered
    with pytest.raises(ValueError):
        row_weight(2, 2, 2)                                                  # the other rank would hold no row: b + (world - 1) = 3 > 2
    with pytest.raises(ValueError):
        row_weight(2, 3, 3)                                                  # two other ranks, one row left
    assert row_weight(2, 3, 4) == 1.5                                        # ... the smallest possible value passes
    with pytest.raises(ValueError):
        row_weight(2, 2, 5, 2)                                               # more than world * B_captured = 4
    assert row_weight(2, 2, 4, 2) == 1.0                                     # ... the largest possible value passes
    assert row_weight(2, 2, 5) == 0.8                                        # without a bound from the caller no upper limit is known
    with pytest.raises(ValueError):
        row_weight(1, 0, None)


@pytest.mark.parametrize("rows", [(2, 1), (4, 1, 3)])
def test_weighted_mean_of_means_is_the_mean_over_all_real_rows(rows):
    """sum_r (w_r / world) * mean_r == mean over all real rows, in fp64: what the all-reduce (the mean over the ranks) computes of the weighted losses"""
    from facialmmt_amd.train_step import row_weight
    g = torch.Generator().manual_seed(11)
    per_rank = [torch.rand(b, dtype=torch.float64, generator=g) * 3 for b in rows]
    world, total = len(rows), sum(rows)
    got = sum(row_weight(b, world, total, max(rows)) / world * x.mean() for b, x in zip(rows, per_rank))
    want = torch.cat(per_rank).mean()
    assert abs(float(got) - float(want)) <= 1e-15 * max(1.0, abs(float(want)))
    plain = sum(x.mean() for x in per_rank) / world                          # without the weights it is a different number
    assert abs(float(plain) - float(want)) > 1e-3
