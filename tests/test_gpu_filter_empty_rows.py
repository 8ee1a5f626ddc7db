"""The frame filter's HIP kernel (ops.select_frames: fmmt_select_frames_fwd / _fwd_n / _bwd) on batches that hold utterances WITHOUT frames, against the
reference's literal loop (oracle.train_glue.select_frames_loop): trailing empty rows as pad_target_batch builds them, (3, 2, 0, 0) and (1, 0, 0, 0), and an
empty utterance in the middle, (3, 0, 2), each in the three branches -- some faces pass, none passes (keep everything), all pass.  The kernel moves values
and gathers one gradient per slot: output, kept-frame mask and the gradient of preds are compared for equality.  With a row count (the packed path) preds
carries three more rows behind the real faces, all above the threshold: they must neither be owned nor move a batch out of the keep-everything branch.
Inputs and cases are those of tests/test_pad_rows_cpu.py, which holds the torch formulation to the same loop."""
import pytest
import torch

from tests.test_pad_rows_cpu import _filter_inputs

pytestmark = pytest.mark.gpu

PASSES = {"some_pass": [1, 0, 1, 1, 0], "none_passes": [0] * 5, "all_pass": [1] * 5}


@pytest.mark.parametrize("packed", [False, True], ids=["every_row_a_face", "n_valid"])
@pytest.mark.parametrize("branch", sorted(PASSES))
@pytest.mark.parametrize("num_imgs", [(3, 2, 0, 0), (1, 0, 0, 0), (3, 0, 2)], ids=lambda n: "-".join(map(str, n)))
def test_kernel_equals_the_literal_loop_with_empty_utterances(num_imgs, branch, packed):
    from facialmmt_amd import ops
    from oracle.train_glue import select_frames_loop
    dev = torch.device("cuda:0")
    n, rows, thr = sum(num_imgs), len(num_imgs), 0.5
    preds, vin, vmask = _filter_inputs(list(num_imgs), PASSES[branch][:n])
    dout = torch.randn(rows, 4, 6 + 7, generator=torch.Generator().manual_seed(3))
    pl = preds.clone().requires_grad_(True)
    want, want_mask = select_frames_loop(pl, vin, vmask, list(num_imgs), thr)
    (want * dout).sum().backward()
    extra = torch.eye(7)[[1, 4, 6]] * 0.97 + 0.03 / 7 if packed else preds[:0]          # padding rows of a capacity, above the threshold
    pk = torch.cat((preds, extra)).to(dev).requires_grad_(True)
    assert ops.select_frames_fusable(pk, vin.to(dev), vmask.to(dev))
    n_valid = torch.tensor([n, n], dtype=torch.int32, device=dev) if packed else None
    got, got_mask = ops.select_frames(pk, vin.to(dev), vmask.to(dev), torch.tensor(num_imgs, device=dev), thr, n_valid)
    (got * dout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(got.detach().cpu(), want.detach()) and torch.equal(got_mask.cpu(), want_mask)
    assert torch.equal(pk.grad[:n].cpu(), pl.grad) and (not packed or float(pk.grad[n:].abs().max()) == 0.0)
    empty = [u for u, k in enumerate(num_imgs) if k == 0]
    assert float(got_mask[empty].abs().max()) == 0.0                                   # an utterance without frames keeps nothing, in every branch
    if branch == "none_passes":
        assert torch.equal(got_mask.cpu(), vmask)
    else:
        assert float(got_mask.sum()) > 0
