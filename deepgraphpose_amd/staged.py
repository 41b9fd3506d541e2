"""Frames (and the flow magnitude computed from them) put on the device ahead of the training step that reads them.

The fit drivers build the batch of iteration it + 1 on a prefetch thread while the GPU trains on iteration it; the thread also uploads the
batch's frames on a stream of its own.  What crosses from that stream to the consumer's is a `Staged` pair: the device tensor and the event
behind the last work that wrote it.  The pair is a value, so the event cannot get lost on the way the way an attribute of the tensor would
(a slice, a view or .to() returns a new tensor object): whoever derives another tensor from `tensor` wraps it with the same `ready`.
Producers: _FrameUploader, _device_flow, _FrameStore.batch, _device_augment.  Consumers: _frames_to_device (TrainSession.run) and dgp_loss_prepare
(loss.py), both through _on_current_stream."""
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

    def _stage(self, img):
        """img -> (its copy in the next pinned staging buffer, that buffer's index); blocks until the buffer's last copy has read it"""
        k = self.turn
        self.turn = (k + 1) % self.slots
        if self.copied[k] is not None:
            self.copied[k].synchronize()          # the copy queued from this buffer `slots` items ago must have read it (any prefetch depth)
        if self.pinned[k] is None or self.pinned[k].numel() < img.size:
            self.pinned[k] = torch.empty(img.size, dtype=torch.uint8).pin_memory()
        stage = self.pinned[k][:img.size].view(img.shape)
        stage.numpy()[...] = img
        return stage, k

    def __call__(self, images) -> Staged:
        stage, k = self._stage(_as_uint8(images))
        with torch.cuda.stream(self.stream):
            dev = stage.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.copied[k] = ev
        return Staged(dev, ev)

    def into(self, dst: torch.Tensor, images):
        """As __call__, but the copy lands in `dst`, an existing device tensor of the images' shape (a run of a _FrameStore's slots)"""
        stage, k = self._stage(_as_uint8(images))
        with torch.cuda.stream(self.stream):
            dst.copy_(stage, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.copied[k] = ev


def _device_flow(uploader, device, images):
    """fit_dgp's temporal clique on the device: the batch's frames are uploaded (by the uploader, on its stream, when prefetching) and
    learn_wt's flow magnitude [nt-1, H, W] is computed from them on the same stream (engine.optical_flow, the reference's parameters).
    -> (Staged frames, Staged magnitude) sharing ONE event, recorded behind the flow (the frames are ready no later than the flow that
    read them); without an uploader everything runs on the current stream and both events are None."""
    if uploader is None:
        return _flow_of(None, torch.from_numpy(np.ascontiguousarray(np.asarray(images).astype(np.uint8))).to(device))
    return _flow_of(uploader, uploader(images).tensor)      # (same stream as the flow: no wait on the copy's own event)


def _flow_of(uploader, dev):
    """_device_flow's second half, for frames that are on the device already (uploaded or gathered on the uploader's stream, or on the
    current one without an uploader) -> (Staged frames, Staged magnitude)"""
    if uploader is None:
        return Staged(dev, None), Staged(engine.optical_flow(dev), None)
    with torch.cuda.stream(uploader.stream):
        mag = engine.optical_flow(dev)
        ev = torch.cuda.Event()
        ev.record(uploader.stream)
    return Staged(dev, ev), Staged(mag, ev)


def _device_augment(uploader, device, images, plans, positions) -> Staged:
    """aug_backend="hip": the batch -- a host array, uploaded here (by the uploader, on its stream, when prefetching), or a device
    tensor written on that stream (a _FrameStore's gather) -- with the plans of its labeled frames applied on the device
    (engine.augment_frames) on the same stream.  -> Staged(frames, the event behind the last stage); without an uploader everything
    runs on the current stream and the event is None."""
    on_device = isinstance(images, torch.Tensor) and images.is_cuda
    if uploader is None:
        dev = images if on_device else torch.from_numpy(_as_uint8(images)).to(device)
        return Staged(engine.augment_frames(dev, plans, positions), None)
    dev = images if on_device else uploader(images).tensor      # (same stream as the stages: no wait on the copy's own event)
    with torch.cuda.stream(uploader.stream):
        engine.augment_frames(dev, plans, positions)
        ev = torch.cuda.Event()
        ev.record(uploader.stream)
    return Staged(dev, ev)


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


FRAME_STORE_BYTES = 16 << 30        # device bytes the _FrameStores of ONE run may hold together; read when a store is filled.  A choice, not
#                                     a measurement: a 2000-frame selection (n_max_frames) of 1280 x 720 video is 5.5 GB, so this holds
#                                     three such videos, and is 6 % of an MI355X's 288 GB
FRAME_STORE_RUN_BYTES = 32 << 20    # frames uploaded per copy while a store is filled (the size the uploader's pinned buffers grow to)


class _FrameStore:
    """The frames a DGP driver trains on -- the sorted unique union of one Dataset's idxs["chunk"], idxs["pv"] and idxs["ph"] -- decoded
    ONCE, in ascending order (a decoder reads forward), and kept on the device as equal-pitch slots (engine.FrameSlots); the schedule
    then visits each about n_times_all_frames = 100 times without touching the source again.  The fill uploads runs of
    FRAME_STORE_RUN_BYTES through the uploader's pinned buffers on its stream (plain copies on the current stream without one), the
    stream every later gather runs on, so no event is kept.  The labeled frames (pv) are also kept as host arrays: data_aug needs their
    pixels.  `budget`: the device bytes this store may take (what is left of FRAME_STORE_BYTES in its run); models/staging.frame_slots
    decides which frames get a slot, the others are `refused`: their batches read them from the source (a labeled one from its host
    copy) and send them through gather_frames' patch (announced once per run by the caller's `announce`)."""

    def __init__(self, dataset, device, uploader=None, budget=None, announce=None):
        import time
        from .models.staging import frame_slots, slot_stride
        self.dataset, self.uploader = dataset, uploader
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        idxs = dataset.idxs
        selected = np.unique(np.concatenate([np.asarray(idxs[k], dtype=np.int64).reshape(-1) for k in ("chunk", "pv", "ph")]))
        labeled = set(int(i) for i in idxs["pv"])
        H, W = int(dataset.nx_in), int(dataset.ny_in)
        self.shape, self.frame_bytes = (H, W, 3), H * W * 3
        stride = slot_stride(self.frame_bytes)
        self.slots, self.refused = frame_slots(selected, self.frame_bytes, FRAME_STORE_BYTES if budget is None else budget, last=labeled)
        self.bytes = len(self.slots) * stride
        self.host, self.last_patched = {}, 0
        if self.refused and announce is not None:
            announce("frame store: %d of %s's %d selected frames do not fit the %d-byte budget; their batches read them from the source"
                     % (len(self.refused), dataset.video_name, len(selected), FRAME_STORE_BYTES))
        t0 = time.perf_counter()
        with torch.cuda.stream(uploader.stream if uploader is not None else torch.cuda.current_stream(self.device)):
            data = torch.empty((len(self.slots), stride), dtype=torch.uint8, device=self.device)
        self.frames = engine.FrameSlots(data, (H, W))
        per_run = max(1, FRAME_STORE_RUN_BYTES // self.frame_bytes)
        run, first = [], 0

        def flush():
            nonlocal run, first
            if run:
                dst = data[first:first + len(run), :self.frame_bytes]
                block = np.stack(run).reshape(len(run), self.frame_bytes)
                if uploader is not None:
                    uploader.into(dst, block)
                else:
                    dst.copy_(torch.from_numpy(block))
                first += len(run)
                run = []

        for f in selected.tolist():                      # ascending: slots are numbered in this order (frame_slots)
            if f not in self.slots and f not in labeled:
                continue
            img = self._read(f)
            if f in labeled:
                self.host[f] = img
            if f in self.slots:
                run.append(img)
                if len(run) == per_run:
                    flush()
        flush()
        if uploader is not None:
            uploader.stream.synchronize()                # (the fill's seconds are the copies' too; nothing trains before iteration 0)
        self.fill_s = time.perf_counter() - t0
        print("frame store: %s: %d frames, %d bytes on %s, filled in %.2f s" % (dataset.video_name, len(self.slots), self.bytes, self.device,
                                                                              self.fill_s), flush=True)

    def _read(self, f):
        img = np.array(self.dataset.video_clip.frame_at(f), dtype=np.uint8)      # (a copy: an ArraySource hands out views)
        if img.shape != self.shape:
            raise ValueError("frame %d of %s is %s, not %s" % (f, self.dataset.video_name, img.shape, self.shape))
        return img

    def batch(self, batch_frames, replaced=None) -> Staged:
        """The frames numbered batch_frames, in that order, as one device batch uint8 [nt, H, W, 3].  `replaced`: {position: pixels} of
        the positions whose pixels were made for this batch (the augmented labeled frames).  Those and the frames without a slot are
        uploaded as ONE patch; everything else comes from the store; one engine.gather_frames on the uploader's stream (the current
        one without an uploader: event None) writes the batch.  With nothing replaced and every frame stored no pixel is uploaded."""
        from .models.staging import gather_table
        replaced = replaced or {}
        src, order = gather_table(batch_frames, self.slots, replaced)
        pixels = []
        for p in order:
            f = int(batch_frames[p])
            pixels.append(replaced[p] if p in replaced else self.host[f] if f in self.host else self._read(f))
        self.last_patched = len(order)
        host = _as_uint8(np.stack(pixels)) if pixels else None
        if self.uploader is None:
            patch = torch.from_numpy(host).to(self.device) if host is not None else None
            return Staged(engine.gather_frames(self.frames, src, patch), None)
        patch = self.uploader(host).tensor if host is not None else None      # (same stream as the gather: no wait on the copy's event)
        with torch.cuda.stream(self.uploader.stream):
            out = engine.gather_frames(self.frames, src, patch)
            ev = torch.cuda.Event()
            ev.record(self.uploader.stream)
        return Staged(out, ev)


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
