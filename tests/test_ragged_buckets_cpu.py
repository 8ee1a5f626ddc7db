"""Host half of the bucketed ragged training step (`frame_capacity` as an ascending tuple on train_step.TargetStep / GraphedTargetStep): the
normalisation of the argument (`train_step.frame_buckets`) and the choice of the capacity a batch runs in (`train_step.frame_bucket`, which is
eval_step.pick_bucket's rule).  No GPU."""
import pytest
import torch


def test_frame_buckets_normalises_none_int_and_tuple():
    from facialmmt_amd.train_step import frame_buckets
    assert frame_buckets(None) is None
    assert frame_buckets(12) == (12,)
    assert frame_buckets((8, 12)) == (8, 12)
    assert frame_buckets([8, 12]) == (8, 12)                       # a list is the same thing
    assert frame_buckets((384, 512, 640)) == (384, 512, 640)
    assert all(type(c) is int for c in frame_buckets((torch.tensor(8), 12)))


@pytest.mark.parametrize("bad", [(12, 8), (8, 8), (0, 8), (), (8, -1), 0, -3])
def test_frame_buckets_refuses_what_is_not_ascending_positive_and_distinct(bad):
    from facialmmt_amd.train_step import frame_buckets
    with pytest.raises(ValueError, match="frame_capacity"):
        frame_buckets(bad)


def test_the_bucket_of_a_batch_is_the_smallest_that_holds_its_clamped_total():
    from facialmmt_amd.eval_step import pick_bucket
    from facialmmt_amd.train_step import frame_bucket
    buckets, Lv = (8, 12), 6
    for counts, want in (([3, 4], 8), ([2, 6], 8), ([6, 5], 12), ([6, 6], 12)):
        assert frame_bucket(counts, Lv, buckets) == want, counts
        assert frame_bucket(torch.tensor(counts), Lv, buckets) == want, counts          # a CPU tensor is read like the list
        assert frame_bucket(counts, Lv, buckets) == pick_bucket(counts, Lv, buckets)     # one rule, stated once
    assert frame_bucket([9, 2], Lv, buckets) == 8                  # 9 clamps to Lv = 6 BEFORE the sum: 8 frames, not 11
    assert frame_bucket([9, -2], Lv, buckets) == 8                 # and a negative count to 0
    assert frame_bucket([9, 9], Lv, buckets) == 12
    assert frame_bucket([3, 4], Lv, (12,)) == 12                   # an int capacity is a tuple of one


def test_a_total_above_the_largest_bucket_raises_naming_it():
    from facialmmt_amd.train_step import check_frame_total, frame_bucket
    with pytest.raises(ValueError, match="frame_capacity=8") as bucketed:
        frame_bucket([6, 6], 6, (4, 8))
    with pytest.raises(ValueError) as single:                      # the text of the single-capacity guard, word for word
        check_frame_total([6, 6], 6, 8)
    assert str(bucketed.value) == str(single.value)
    with pytest.raises(ValueError, match="frame_capacity=12"):
        frame_bucket(torch.tensor([6, 6, 1]), 6, (8, 12))
