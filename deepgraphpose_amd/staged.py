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


IMAGE_CACHE_BYTES = 1 << 30         # device bytes an _ImageCache may hold (the size of eval.py's CHUNK_BYTES); read when an image is added


class _ImageCache:
    """The labeled images of a PoseDataset as uint8 device tensors [H, W, 3]: each is decoded once, on first use, and uploaded on the
    uploader's stream (the current stream without an uploader) -- the stream every later read of it runs on (_device_sample), so no
    event is kept.  A project has a few dozen labeled images and fit_dlc draws from them up to 200 000 times.  The cache holds at most
    IMAGE_CACHE_BYTES; get() returns None for an image that does not fit, whose samples then take the host path for their pixels
    (announced once)."""

    def __init__(self, dataset, device, uploader=None):
        self.dataset, self.uploader = dataset, uploader
        self.device = torch.device("cuda", device) if isinstance(device, int) else device
        self.images, self.refused, self.bytes, self.announced = {}, set(), 0, False

    def get(self, item):
        import os
        from .dlc_dataset import imread
        key = item.image_id
        if key in self.images:
            return self.images[key]
        if key in self.refused:
            return None
        img = np.array(imread(os.path.join(self.dataset.cfg.project_path, item.im_path)))      # (a writable copy)
        if self.bytes + img.nbytes > IMAGE_CACHE_BYTES:
            self.refused.add(key)
            if not self.announced:
                self.announced = True
                print("image cache: %s (%d bytes) does not fit the %d-byte cache; such samples' pixels are prepared on the host"
                      % (item.im_path, img.nbytes, IMAGE_CACHE_BYTES), flush=True)
            return None
        dev = self.uploader(img).tensor if self.uploader is not None else torch.from_numpy(img).to(self.device)
        self.images[key] = dev
        self.bytes += img.nbytes
        return dev


_RESIZE_REFUSED = [False]


def _device_sample(dataset, plan, cache, uploader, device):
    """One fit_dlc sample built on the device from its plan (PoseDataset.plan_batch): the pixels by engine.window_resize from the cached
    image (BOX below scale 1, BILINEAR above: imresize's filters without OpenCV), the four target maps by engine.target_maps from the
    plan's entries -- on the uploader's stream, or on the current one without an uploader.
    -> (Staged frames uint8 [1, h, w, 3], {part_score_targets, part_score_weights, locref_targets, locref_mask: Staged fp32}), all
    sharing ONE event (None without an uploader).  An image the cache refused, or a shape the resize kernel refuses (said once), has
    its pixels prepared on the host and uploaded; the maps are built on the device all the same."""
    from . import _lib
    from .dlc_dataset import plan_entries
    cfg = dataset.cfg

    def build():
        image = cache.get(plan.item)
        frames = None
        if image is not None:
            try:
                frames = engine.window_resize(image, plan.crop, plan.out_hw, "box" if plan.scale < 1 else "bilinear", plan.mirror)[None]
            except _lib.DgpError as e:
                if not _RESIZE_REFUSED[0]:
                    _RESIZE_REFUSED[0] = True
                    print("window_resize refused a sample (%s); such samples' pixels are prepared on the host" % e, flush=True)
                image = image.cpu().numpy()
        if frames is None:
            host = np.ascontiguousarray(dataset.host_pixels(plan, image))[None]
            frames = uploader(host).tensor if uploader is not None else torch.from_numpy(host).to(device)
        ent = plan_entries(plan)
        sc, wts, lmap, lmask = engine.target_maps(ent, [0, ent.shape[0]], 1, int(plan.sm_size[0]), int(plan.sm_size[1]), int(cfg.num_joints),
                                                  pos_dist_thresh=cfg.pos_dist_thresh, stride=dataset.stride, scale=plan.scale,
                                                  locref_stdev=cfg.locref_stdev,
                                                  weigh_only_present_joints=bool(cfg.weigh_only_present_joints), device=device)
        return frames, dict(part_score_targets=sc, part_score_weights=wts, locref_targets=lmap, locref_mask=lmask)

    if uploader is None:
        frames, maps = build()
        ev = None
    else:
        with torch.cuda.stream(uploader.stream):
            frames, maps = build()
            ev = torch.cuda.Event()
            ev.record(uploader.stream)
    return Staged(frames, ev), {k: Staged(v, ev) for k, v in maps.items()}


def _device_locref(uploader, device, joint_loc, nt, vis_within, nx_out, ny_out, nj, dgp_cfg):
    """The DGP drivers' locref targets on the device: coord2map's entries (dataset.coord2map_entries) spread over the batch's nt frames
    -- labeled frame ii of joint_loc is frame vis_within[ii], every other frame has no entries and comes out zero -- and
    engine.target_maps with coord2map's constants (stride 8, scale 1).  -> (Staged locref_map, Staged locref_mask) [nt, nx_out, ny_out,
    2 nj] sharing one event, on the uploader's stream (current stream and None without one)."""
    from .dataset import coord2map_entries
    joint_loc = np.asarray(joint_loc, dtype=np.float64)
    ent, off = coord2map_entries(joint_loc.reshape(-1, nj, 2), nj)
    counts = np.zeros(nt, dtype=np.int64)
    order = np.argsort(np.asarray(vis_within, dtype=np.int64), kind="stable") if len(vis_within) else np.zeros(0, dtype=np.int64)
    counts[np.asarray(vis_within, dtype=np.int64)] = np.diff(off)
    ent = np.concatenate([ent[off[i]:off[i + 1]] for i in order] + [np.zeros((0, 3))])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    def build():
        _, _, lmap, lmask = engine.target_maps(ent, offsets, nt, nx_out, ny_out, nj, pos_dist_thresh=dgp_cfg.pos_dist_thresh, stride=8.0,
                                               scale=1.0, locref_stdev=dgp_cfg.locref_stdev, scmap=None, weights=None, device=device)
        return lmap, lmask

    if uploader is None:
        lmap, lmask = build()
        return Staged(lmap, None), Staged(lmask, None)
    with torch.cuda.stream(uploader.stream):
        lmap, lmask = build()
        ev = torch.cuda.Event()
        ev.record(uploader.stream)
    return Staged(lmap, ev), Staged(lmask, ev)
