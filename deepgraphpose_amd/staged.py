"""Frames (and the flow magnitude computed from them) put on the device ahead of the training step that reads them.

The fit drivers build the batch of iteration it + 1 on a prefetch thread while the GPU trains on iteration it; the thread also uploads the
batch's frames on a stream of its own.  What crosses from that stream to the consumer's is a `Staged` pair: the device tensor and the event
behind the last work that wrote it.  The pair is a value, so the event cannot get lost on the way the way an attribute of the tensor would
(a slice, a view or .to() returns a new tensor object): whoever derives another tensor from `tensor` wraps it with the same `ready`.
Producers: _FrameUploader, _device_flow.  Consumers: _frames_to_device (TrainSession.run) and dgp_loss_prepare (loss.py), both through
_on_current_stream."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import engine


class Staged(NamedTuple):
    tensor: torch.Tensor
    ready: Optional[torch.cuda.Event]        # None: already ordered on the consumer's stream


def _on_current_stream(x):
    """A Staged pair, or a bare device tensor (no event: the caller ordered it), -> the tensor, usable on the current stream of its device:
    the stream waits for the pair's event, and the allocator learns that the tensor is in use there."""
    tensor, ready = x if isinstance(x, Staged) else (x, None)
    cur = torch.cuda.current_stream(tensor.device)
    if ready is not None:
        cur.wait_event(ready)
    tensor.record_stream(cur)
    return tensor


def _as_uint8(images):
    img = np.ascontiguousarray(images)
    if img.dtype != np.uint8:
        img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img


class _FrameUploader:
    """Uploads a batch's frames from the prefetch thread: numpy -> one of a few pinned staging buffers -> device, asynchronously on its
    own HIP stream, so that the frames of iteration it + 1 are already resident when the GPU finishes iteration it (a 10 MB pageable
    copy at the start of every step is 0.4 ms of idle GPU).  -> Staged(device frames, the copy's event)."""

    def __init__(self, device, slots: int = 4):
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        self.stream = torch.cuda.Stream(device=self.device)
        self.slots, self.pinned, self.turn = slots, [None] * slots, 0
        self.copied = [None] * slots              # event behind the last H2D copy issued from each staging buffer

    def __call__(self, images) -> Staged:
        img = _as_uint8(images)
        k = self.turn
        self.turn = (k + 1) % self.slots
        if self.copied[k] is not None:
            self.copied[k].synchronize()          # the copy queued from this buffer `slots` items ago must have read it (any prefetch depth)
        if self.pinned[k] is None or self.pinned[k].numel() < img.size:
            self.pinned[k] = torch.empty(img.size, dtype=torch.uint8).pin_memory()
        stage = self.pinned[k][:img.size].view(img.shape)
        stage.numpy()[...] = img
        with torch.cuda.stream(self.stream):
            dev = stage.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.copied[k] = ev
        return Staged(dev, ev)


def _device_flow(uploader, device, images):
    """fit_dgp's temporal clique on the device: the batch's frames are uploaded (by the uploader, on its stream, when prefetching) and
    learn_wt's flow magnitude [nt-1, H, W] is computed from them on the same stream (engine.optical_flow, the reference's parameters).
    -> (Staged frames, Staged magnitude) sharing ONE event, recorded behind the flow (the frames are ready no later than the flow that
    read them); without an uploader everything runs on the current stream and both events are None."""
    if uploader is None:
        dev = torch.from_numpy(np.ascontiguousarray(np.asarray(images).astype(np.uint8))).to(device)
        return Staged(dev, None), Staged(engine.optical_flow(dev), None)
    dev = uploader(images).tensor                 # (same stream as the flow below: no wait on the copy's own event)
    with torch.cuda.stream(uploader.stream):
        mag = engine.optical_flow(dev)
        ev = torch.cuda.Event()
        ev.record(uploader.stream)
    return Staged(dev, ev), Staged(mag, ev)


def _frames_to_device(trainer, images):
    """Batch images -> uint8 device frames; the net follows the batch's resolution (videos of one project may differ in size:
    the reference's placeholders are [None, None, None, 3]).  A Staged pair from _FrameUploader passes through after its copy, a bare
    device tensor as it is; anything else is a host array and is uploaded here."""
    on_device = isinstance(images, Staged) or (isinstance(images, torch.Tensor) and images.is_cuda)
    frames = _on_current_stream(images) if on_device else _as_uint8(images)
    if (trainer.net.in_h, trainer.net.in_w) != tuple(frames.shape[1:3]):
        trainer.set_input_size(int(frames.shape[1]), int(frames.shape[2]))
    return frames if on_device else torch.from_numpy(frames).to(trainer.device)
