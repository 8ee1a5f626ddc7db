"""Plumbing every captured step shares (train_step's three graphed training steps, graph_multimodal, eval_step.GraphedEvalStep): streams that are
really distinct, the garbage-collection fence around a capture, the warm-up on the capture stream and its undoing, the copy of a batch into the
captured input buffers, and the replay of the update graph at the end of an accumulation window.  No kernel is launched from here."""
from __future__ import annotations

import contextlib
import os

import torch


def require_packet_capture_off(who):
    """what a capturing constructor calls first: RuntimeError unless the process started with the runtime's packet capture switched off"""
    if os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "") != "0":
        raise RuntimeError(f"{who}: DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 must be in the environment before the HIP runtime initialises (import "
                           "facialmmt_amd before the first CUDA call, or export it; see facialmmt_amd/__init__.py): with ROCm 7.0's packet "
                           "capture, gradients of replayed graphs are wrong from the third replay on")


def _autocast(dtype, **kw):
    """`with _autocast(dtype):` -- torch.autocast on the GPU at `dtype`, nothing at None (`kw`: torch.autocast's, e.g. cache_enabled=False)"""
    return torch.autocast("cuda", dtype=dtype, **kw) if dtype is not None else contextlib.nullcontext()


def pick_concurrent_stream(device, candidates: int = 8, cycles: int = 4_000_000):
    """A HIP stream that really runs concurrently with the current one.  HIP multiplexes streams onto a handful of
    hardware queues (4 by default) and two streams that share a queue serialise; which queue a new stream lands on
    depends on how many streams the process created before (RCCL, for one, creates several at process-group
    initialisation -- measured: the text-encoder overlap vanished in every run that had called init_process_group).
    So measure it: spin kernels on both streams, keep the first candidate whose pair finishes in about the time
    of one.  Returns (stream, ratio) with ratio = t(pair) / t(single); falls back to the best candidate."""
    import time
    main = torch.cuda.current_stream(device)

    def timed(fn):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0
    torch.cuda._sleep(cycles)                              # warm up the spin kernel
    single = min(timed(lambda: torch.cuda._sleep(cycles)) for _ in range(3))
    best, best_ratio, keep = None, float("inf"), []
    for _ in range(candidates):
        s = distinct_stream(device, keep)
        keep.append(s)                                     # keep candidates alive so that the next one is a new stream

        def pair():
            s.wait_stream(main)
            torch.cuda._sleep(cycles)
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
        ratio = min(timed(pair) for _ in range(2)) / single
        if ratio < best_ratio:
            best, best_ratio = s, ratio
        if ratio < 1.3:
            break
    return best, best_ratio


def distinct_stream(device, avoid=()):
    """A side stream that is a different HIP stream from every stream in `avoid` and from the current one.
    torch.cuda.Stream() hands out entries of a per-device pool of 32 round-robin: in a process that has created a few dozen
    streams a "new" stream can BE the capture stream or another branch's stream, and a fork / join between a stream and
    itself inside a graph capture has crashed the HIP runtime (intermittent segmentation fault in the capture of a step when
    the whole GPU test suite ran in one process).  So: compare the raw handles and keep drawing."""
    taken = {s.cuda_stream for s in avoid if s is not None} | {torch.cuda.current_stream(device).cuda_stream}
    keep = []
    for _ in range(64):
        s = torch.cuda.Stream(device=device)
        if s.cuda_stream not in taken:
            return s
        keep.append(s)
    raise RuntimeError("distinct_stream: the stream pool only returns streams that are already in use")


# Captured graphs are never destroyed.  On this ROCm (7.0 runtime under torch 2.10) tearing down HIP graphs that were captured
# with forked streams is what the intermittent crashes of a long-lived process traced back to: destroyed by a garbage
# collection during a later capture -> abort inside the capture; destroyed right before the next capture -> segmentation
# fault in that graph's first replay.  A training process captures a handful of graphs; holding on to them costs nothing.
_KEEP_GRAPHS = []


class capture_window:
    """Garbage collection fenced off a graph capture: collect NOW (cycles left by earlier steps may own HIP graphs, streams
    and pool memory whose destructors call into the HIP runtime), then keep the cyclic collector off until the capture ends.
    torch.cuda.graph stopped collecting on entry (torch >= 2.9 only does with torch.compiler.config.force_cudagraph_gc), and a
    collection that fires in the middle of a capture destroys such objects while the stream is capturing: measured here as an
    intermittent abort / segmentation fault of the process (faulthandler: "Garbage-collecting" inside the capture of a step
    that followed other graph-capturing steps), two runs in five of the whole GPU suite."""

    def __enter__(self):
        import gc
        self._was = gc.isenabled()
        gc.collect()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


def _restore(snap):
    """copy the snapshot back, touching only what changed: an untouched buffer keeps its version counter, so host-side
    caches keyed on it (SwinTransformerBlock._mask_is_standard) stay valid and nothing synchronises inside the capture"""
    with torch.no_grad():
        for t, v in snap:
            if not torch.equal(t, v):
                t.copy_(v)


def _reset_optimizer_state(opt):
    """zero every tensor of the optimizer state in place (moments, step counters): undoes the warm-up steps that precede
    a graph capture without re-allocating the state the captured graph will address"""
    for st in opt.state.values():
        for v in st.values():
            if torch.is_tensor(v):
                v.zero_()
    for g in opt.param_groups:                              # HFAdamW keeps its (device) step counter in the group, not in opt.state
        if torch.is_tensor(g.get("step")):
            g["step"].zero_()


def _bump_versions(params):
    """A graph replay updates parameters in place without autograd noticing: bump their version counters, so that eager code
    that caches by version (ops._lp: the bf16 weight shadows of an eval() pass after training) rebuilds what it cached."""
    inc = getattr(torch._C, "_increment_version", None)
    if inc is None:
        return
    try:
        inc(params)
    except TypeError:
        for p in params:
            inc(p)


@contextlib.contextmanager
def warmup_undone(snap, device, stream, undo=None):
    """`with warmup_undone(...):` -- the block runs on `stream` (the capture stream: lazy initialisations -- kernel attributes, shadow caches,
    optimizer state -- happen where the capture will run) behind what the current stream holds; on exit the streams are joined, the device is
    synchronised, every (tensor, value) of `snap` is put back, `undo()` puts back what else the passes touched (a training step's optimizer state
    and flat gradient buffers; nothing for evaluation) and the generator returns to its state at entry."""
    rng = torch.cuda.get_rng_state(device)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        yield
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize(device)
    _restore(snap)
    if undo is not None:
        undo()
    torch.cuda.set_rng_state(rng, device)


def check_static_shapes(static, batch, who):
    """A batch against the captured input buffers `static`, on the host, before anything is copied or launched: the batch's entries as tensors
    (lists -- the reference's collate hands num_imgs and the utterance index over as lists -- become tensors), or ValueError for another number
    of entries or an entry of another shape."""
    if len(batch) != len(static):
        raise ValueError(f"{who}: batch of {len(batch)} entries, captured with {len(static)}")
    srcs = [s if torch.is_tensor(s) else torch.as_tensor(s) for s in batch]
    for i, (dst, src) in enumerate(zip(static, srcs)):
        if tuple(src.shape) != tuple(dst.shape):
            raise ValueError(f"{who}: batch entry {i} has shape {tuple(src.shape)}, the captured graphs are for {tuple(dst.shape)}")
    return srcs


def copy_into_static(static, batch, who, skip=()):
    """copy a batch into the captured input buffers, without a host synchronisation -- only once EVERY entry has passed check_static_shapes: a
    rejected batch leaves `static` as it was.  An entry that is its buffer, or whose index is in `skip`, is not copied."""
    srcs = check_static_shapes(static, batch, who)
    with torch.no_grad():
        for i, (dst, src) in enumerate(zip(static, srcs)):
            if i not in skip and dst is not src:
                dst.copy_(src, non_blocking=True)


def replay_update(step, accumulation_steps, before_update=None):
    """the end of a micro-step of a graphed training step: count it, and on the last one of an accumulation window run `before_update()` (a
    gradient exchange), replay graph B (clip + optimizer), tell autograd the parameters moved and step the schedule"""
    step.i_batch += 1
    if step.i_batch % accumulation_steps == 0:
        if before_update is not None:
            before_update()
        step.graph_b.replay()
        _bump_versions(step.flat.params)                    # a replay changes the parameters behind autograd's back
        if step.sched is not None:
            step.sched.step()
