"""The pieces the graphed steps share, on CPU tensors: the flat-gradient tail (train_step.FlatGradientTail: hand-over, update) against plain torch,
graph_capture.copy_into_static (check everything, then copy) and the frame-capacity host rules (one function behind three names)."""
import pytest
import torch


def test_flat_gradient_tail_equals_clip_and_step_on_the_summed_gradients():
    """nn.Linear(3, 2), SGD(lr 0.1), clip 0.5; on the CPU neither fused path is eligible, so hand_over() is the multi-tensor copy / add and update()
    is clip_grad_norm_ + opt.step() over the flat buffers.  One micro-step (overwrite) and a window of two (accumulate): the parameters equal, bit
    for bit, those of a twin that clipped and stepped on the summed gradients; no leaf keeps a .grad; under accumulation the buffers end zeroed."""
    from facialmmt_amd.train_step import FlatGradientTail
    for window in (1, 2):
        torch.manual_seed(0)
        model, twin = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
        twin.load_state_dict(model.state_dict())
        w0 = model.weight.detach().clone()
        opt, opt2 = torch.optim.SGD(model.parameters(), lr=0.1), torch.optim.SGD(twin.parameters(), lr=0.1)
        tail = FlatGradientTail(model.parameters(), opt, 0.5, window > 1)
        assert tail.fused is None and tail.handover is None and not tail.exchanging and all(p.grad is None for p in model.parameters())
        grads = [[torch.randn_like(p) * 3 for p in model.parameters()] for _ in range(window)]        # norm well above the clip value
        for gs in grads:
            for p, g in zip(model.parameters(), gs):
                p.grad = g.clone()
            tail.hand_over()
            assert all(p.grad is None for p in model.parameters())
        tail.update()
        for q, *gs in zip(twin.parameters(), *grads):
            q.grad = sum(gs[1:], gs[0].clone())
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5)
        opt2.step()
        for p, q in zip(model.parameters(), twin.parameters()):
            assert torch.equal(p, q) and p.grad is None
        assert not torch.equal(model.weight, w0)                                                         # something moved
        if window > 1:
            assert all(not b[0].any() for b in tail.flat.buckets)


def test_copy_into_static_checks_every_entry_before_it_copies_one():
    from facialmmt_amd.graph_capture import copy_into_static
    static = [torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(4), torch.zeros(2, 5), torch.zeros(1)]
    own = static[2]
    own.fill_(7.0)
    batch = (torch.ones(2, 3), [4, 5], own, torch.full((2, 5), 2.0), torch.tensor([9.0]))
    copy_into_static(static, batch, "step", skip=(4,))
    assert torch.equal(static[0], batch[0]) and static[1].tolist() == [4, 5] and torch.equal(static[3], batch[3])
    assert static[2] is own and torch.equal(own, torch.full((4,), 7.0))                             # dst is src: left alone
    assert float(static[4]) == 0.0                                                                    # skip=
    before = [t.clone() for t in static]
    bad = (torch.full((2, 3), 5.0), [6, 7], torch.ones(4), torch.ones(2, 6), torch.tensor([1.0]))
    with pytest.raises(ValueError) as err:
        copy_into_static(static, bad, "step")
    assert "entry 3" in str(err.value) and "(2, 6)" in str(err.value) and "(2, 5)" in str(err.value)
    assert all(torch.equal(a, b) for a, b in zip(static, before))                                    # entries 0..2 were NOT copied
    with pytest.raises(ValueError, match="4 entries"):
        copy_into_static(static, bad[:4], "step")
    assert all(torch.equal(a, b) for a, b in zip(static, before))


def test_frame_capacity_host_rules_exist_once():
    from facialmmt_amd import eval_step, train_step
    assert train_step.frame_bucket is train_step.pick_bucket is eval_step.pick_bucket
    with pytest.raises(ValueError) as err:
        train_step.check_frame_total([3, 9, 2], 4, 8)
    assert "9 face frames" in str(err.value) and "frame_capacity=8" in str(err.value)
    assert train_step.check_frame_total([3, 9, 2], 4, 9) is None                                     # clamped: 3 + 4 + 2 = 9
