"""The host side of estimate_pose's pipeline that never touches the GPU (models/eval.py drives it): the ring of staging buffers between
the threads that fill batches and the one consumer that uploads them, the two producers, the chunk geometry and a shard's frames.
No torch in here: the buffers are anything numpy can write to (eval.py passes the .numpy() views of its pinned tensors).
Also the torch-free half of the fit drivers' device frame store (staged._FrameStore): which frames get a slot, and a batch's gather table."""
from __future__ import annotations

import itertools
import threading
import time

import numpy as np


class StagingRing:
    """N producer threads fill `bufs` (one batch each), ONE consumer takes the batches in order 0, 1, 2, ... and hands every slot back
    once it is done with it.  All state is guarded by `cv`: staged[k] = (slot, frames) of batch k; free = the slots nobody holds;
    n_got / n_freed = batches the consumer has taken / slots it has handed back; total = the number of batches once known;
    err = the first error of either side, which ends every wait; stage_s = seconds the producers reported with their batches."""

    def __init__(self, bufs):
        self.bufs = bufs
        self.cv = threading.Condition()
        self.staged, self.free = {}, list(range(len(bufs)))
        self.n_got = self.n_freed = 0
        self.total = self.err = None
        self.stage_s = 0.0

    def take(self, k: int) -> int:
        """A free slot for batch k.  Staging window: batch k is staged only while k < n_freed + nslots and a slot is free -- those are the
        batches that can hold a slot at once, so no thread can starve an earlier batch (the one the consumer waits for) of its slot."""
        with self.cv:
            while not (k < self.n_freed + len(self.bufs) and self.free) and self.err is None:
                self.cv.wait()
            if self.err is not None:
                raise RuntimeError("staging stopped")
            return self.free.pop()

    def publish(self, k: int, slot: int, nb: int, seconds: float = 0.0):
        with self.cv:
            self.staged[k] = (slot, nb)
            self.stage_s += seconds
            self.cv.notify_all()

    def set_total(self, n: int):
        with self.cv:
            self.total = n
            self.cv.notify_all()

    def fail(self, e: BaseException):
        """Error handling: the first error of a producer or of the consumer; take() and get() raise from then on, so no thread waits for ever."""
        with self.cv:
            self.err = self.err or e
            self.cv.notify_all()

    def give_back(self, slot: int):
        with self.cv:
            self.free.append(slot)
            self.n_freed += 1
            self.cv.notify_all()

    def get(self, k: int, reclaim):
        """Consumer: (slot, frames) of batch k, or None when there is no batch k; raises a producer's error.  While the consumer holds no
        slot it polls (50 ms waits); while it holds some the producers may be waiting for exactly those, so it calls reclaim(), which has
        to give_back() at least one of them (eval.py: blocks on its oldest upload)."""
        while True:
            with self.cv:
                if self.err is not None:
                    raise self.err
                if k in self.staged:
                    self.n_got += 1
                    return self.staged.pop(k)
                if self.total is not None and k >= self.total:
                    return None
                if self.n_got == self.n_freed:
                    self.cv.wait(0.05)
                    continue
            reclaim()


def stage_stack(ring: StagingRing, frames, lo: int, hi: int, batch_size: int, tid: int, n_threads: int):
    """Producer over an in-memory stack: thread tid stages batches tid, tid + n_threads, ... of frames[lo:hi], ONE GIL-free copy each
    (the caller declares the total, which is known up front).  Any error is recorded in the ring and raised again in the consumer."""
    try:
        for k in range(tid, -(-(hi - lo) // batch_size), n_threads):
            a = lo + k * batch_size
            nb = min(batch_size, hi - a)
            slot = ring.take(k)
            t_ = time.perf_counter()
            np.copyto(ring.bufs[slot][:nb], frames[a:a + nb])
            ring.publish(k, slot, nb, time.perf_counter() - t_)
    except BaseException as e:
        ring.fail(e)


def stage_decoded(ring: StagingRing, frames, n_local: int, batch_size: int):
    """Producer over a decoder (one thread: decoding is sequential): the first n_local frames of the iterator `frames`, frame by frame; a
    short last batch is published, then the total is declared.  Any error is recorded in the ring and raised again in the consumer."""
    try:
        k, fill, count, slot = 0, 0, 0, None
        for fr in frames:
            if count >= n_local:
                break
            if slot is None:
                slot = ring.take(k)
            np.copyto(ring.bufs[slot][fill], fr)
            fill += 1
            count += 1
            if fill == batch_size:
                ring.publish(k, slot, fill)
                k, fill, slot = k + 1, 0, None
        if fill:
            ring.publish(k, slot, fill)
            k += 1
        ring.set_total(k)
    except BaseException as e:
        ring.fail(e)


def stage_jpeg(ring: StagingRing, source, info0, lo: int, hi: int, batch_size: int, tid: int, n_threads: int, name="the video"):
    """Producer over a source of baseline JPEG streams (source.jpeg_bytes(t), thread-safe): stage_stack's dealing scheme -- thread tid
    stages batches tid, tid + n_threads, ... of frames [lo, hi), the caller declares the total -- but a batch is Huffman-decoded, not
    copied: frame i of the batch goes into row i of the slot's (coef int16 [B, total_blocks * 64], qt uint16 [B, ncomp * 64]) pair
    through dgp_jpeg_entropy_decode, which holds no lock and no GIL.  A frame whose size or sampling differs from info0 (the first
    frame's dgp_jpeg_probe) is a ValueError naming the frame; like any error it is recorded in the ring and raised in the consumer."""
    from .. import jpeg
    try:
        for k in range(tid, -(-(hi - lo) // batch_size), n_threads):
            a = lo + k * batch_size
            nb = min(batch_size, hi - a)
            slot = ring.take(k)
            t_ = time.perf_counter()
            coef, qt = ring.bufs[slot]
            for i in range(nb):
                data = source.jpeg_bytes(a + i)
                if data is None:
                    raise ValueError("frame %d of %s is not a JPEG file" % (a + i, name))
                info = jpeg.probe(data)
                if not jpeg.same_geometry(info, info0):
                    raise ValueError("frame %d of %s is %d x %d %s, the first frame %d x %d %s" % (
                        a + i, name, info.width, info.height, jpeg.SAMPLING_NAMES[info.sampling], info0.width, info0.height,
                        jpeg.SAMPLING_NAMES[info0.sampling]))
                jpeg.entropy_decode(data, info, coef[i], qt[i])
            ring.publish(k, slot, nb, time.perf_counter() - t_)
    except BaseException as e:
        ring.fail(e)


def chunk_plan(n_frames: int, world: int, batch_size: int, batch_bytes: int, env_batches: int, chunk_bytes: int):
    """-> (chunk_batches, n_rounds).  A chunk is the run of batches whose frames stay on the device until their range check has come back
    clean: env_batches (DGP_EVAL_CHUNK_BATCHES) of them, but at most chunk_bytes of frames (1 GiB: 36 batches of 32 at 640 x 480, 24 of
    16 at 1280 x 720) and never more than the longest shard holds; at least one.  Chunk rounds: every term is the same on every rank --
    the longest shard's length, never the rank's own, and nothing like free memory -- because each round ends in a collective."""
    per_rank_batches = max(1, -(-(-(-n_frames // world)) // batch_size))
    chunk_cap = int(chunk_bytes // max(batch_bytes, 1)) or 1
    chunk_batches = max(1, min(env_batches, chunk_cap, per_rank_batches))
    return chunk_batches, -(-per_rank_batches // chunk_batches)


def shard_frames(source, lo: int, hi: int, world: int, name="the video"):
    """-> (first, rest): the first frame of the shard [lo, hi) of `source` and an iterator over its other frames.  A sharded run seeks
    (frame_at) when the source can; otherwise the frames before lo are decoded and dropped.  An empty shard of a seekable source gets
    frame 0 as `first` (the frame size is needed everywhere) and no frames; no first frame at all is a ValueError."""
    if world > 1 and hasattr(source, "frame_at"):
        return source.frame_at(lo if hi > lo else 0), (source.frame_at(t) for t in range(lo + 1, hi))
    it = iter(source.iter_frames())
    first = next(itertools.islice(it, lo, None), None)
    if first is None:
        raise ValueError("no frames in %s" % (name,))
    return first, itertools.islice(it, max(hi - lo - 1, 0))


def slot_stride(frame_bytes: int) -> int:
    """The byte pitch of a frame store's slots: frame_bytes rounded up to 16 (every slot starts 16-byte aligned)"""
    return -(-int(frame_bytes) // 16) * 16


def frame_slots(frames, frame_bytes: int, budget_bytes: int, last=()):
    """Which of a video's selected frames get a slot in the device frame store (staged._FrameStore) when the store may hold
    budget_bytes: -> ({frame: slot}, refused frames, sorted).  `frames`: any sequence of frame numbers; its sorted unique values are
    the candidates, and a slot costs slot_stride(frame_bytes).  All of them are stored when they fit.  Otherwise the frames in `last`
    (the labeled ones, of which the drivers keep host copies anyway: leaving them out costs no decode) give way first, and inside
    either group the lower frame numbers are kept.  Slots are numbered in ascending frame order, the order in which the store is
    filled, so a decoder reads forward."""
    cand = sorted(set(int(f) for f in frames))
    n_fit = max(0, int(budget_bytes)) // slot_stride(frame_bytes)
    late = set(int(f) for f in last)
    order = [f for f in cand if f not in late] + [f for f in cand if f in late]
    kept = sorted(order[:n_fit])
    return {f: s for s, f in enumerate(kept)}, sorted(order[n_fit:])


def gather_table(batch_frames, slots, patched=()):
    """The `src` table of engine.gather_frames for one batch: batch_frames[p] is the frame number at position p of the batch, `slots`
    maps the stored frames to their slots, `patched` holds the POSITIONS whose pixels are uploaded for this batch (augmented labeled
    frames).  A position whose frame has no slot is patched as well.  -> (src int32 [nt], patch positions in patch order): position p
    reads slot slots[frame] (src >= 0; a frame that occurs twice reads the same slot twice), or patch frame k (src = -1 - k) when it
    is the k-th patched position."""
    forced = set(int(p) for p in patched)
    src, order = [], []
    for p, f in enumerate(batch_frames):
        if p in forced or int(f) not in slots:
            src.append(-1 - len(order))
            order.append(p)
        else:
            src.append(slots[int(f)])
    return np.asarray(src, dtype=np.int32), order
