"""The host side of estimate_pose that needs no GPU (deepgraphpose_amd/models/staging.py): the staging ring and its two producers, the
chunk geometry and a shard's frames.  Every thread started here is a daemon and is joined with a time limit: a deadlock fails, it does
not hang."""
import threading

import numpy as np
import pytest

from deepgraphpose_amd.dist import shard_range
from deepgraphpose_amd.frames import ArraySource
from deepgraphpose_amd.models import staging as S

JOIN_S = 5.0


def _join(threads):
    for th in threads:
        th.join(JOIN_S)
    assert not [th.name for th in threads if th.is_alive()], "threads still running: deadlock"


def _stack(n=20):
    return np.random.RandomState(3).randint(0, 256, (n, 4, 5, 3)).astype(np.uint8)


class _Consumer(threading.Thread):
    """Takes the batches in order like estimate_pose's upload loop, but keeps every slot until it asks for the next-but-one batch (or until
    the ring calls reclaim), so that producers really wait for slots.  What it saw ends up in .got / .totals / .error."""

    def __init__(self, ring):
        super().__init__(daemon=True, name="consumer")
        self.ring, self.held, self.got, self.totals, self.error = ring, [], [], [], None

    def give_oldest(self):
        k, slot, nb, seen = self.held.pop(0)
        assert np.array_equal(self.ring.bufs[slot][:nb], seen), "slot of batch %d was written while the consumer held it" % k
        self.ring.give_back(slot)

    def run(self):
        try:
            k = 0
            while True:
                while self.held and self.held[0][0] <= k - 2:
                    self.give_oldest()
                item = self.ring.get(k, self.give_oldest)
                if item is None:
                    break
                slot, nb = item
                self.totals.append(self.ring.total)
                self.got.append(self.ring.bufs[slot][:nb].copy())
                self.held.append((k, slot, nb, self.got[-1]))
                k += 1
            while self.held:
                self.give_oldest()
        except BaseException as e:
            self.error = e


class _WindowLog:
    """the stack the producers read: every read of batch k notes (k, n_freed, slots in use) -- the producer holds batch k's slot by then"""

    def __init__(self, frames, ring, lo, batch_size):
        self.frames, self.ring, self.lo, self.batch_size, self.seen = frames, ring, lo, batch_size, []

    def __getitem__(self, sl):
        with self.ring.cv:
            self.seen.append(((sl.start - self.lo) // self.batch_size, self.ring.n_freed, len(self.ring.bufs) - len(self.ring.free)))
        return self.frames[sl]


@pytest.mark.parametrize("n_threads,nslots", [(2, 2), (2, 8), (1, 1)])
def test_ring_stack_producers_keep_order_bytes_and_the_staging_window(n_threads, nslots):
    frames, B = _stack(20), 3
    ring = S.StagingRing([np.zeros((B, 4, 5, 3), np.uint8) for _ in range(nslots)])
    src = _WindowLog(frames, ring, 0, B)
    ring.set_total(7)
    producers = [threading.Thread(target=S.stage_stack, args=(ring, src, 0, 20, B, t, n_threads), daemon=True, name="stage%d" % t)
                 for t in range(n_threads)]
    con = _Consumer(ring)
    for th in producers + [con]:
        th.start()
    _join(producers + [con])
    assert con.error is None, con.error
    assert [len(b) for b in con.got] == [3] * 6 + [2]                       # in order, the last batch short
    assert np.array_equal(np.concatenate(con.got), frames)
    assert sorted(k for k, _, _ in src.seen) == list(range(7))
    # n_freed only grows, so a batch staged outside the window k < n_freed + nslots at the time of take() is still outside it at its read
    # unless the consumer freed a slot in between; the slots in use can never exceed the ring
    assert all(k < n_freed + nslots and 1 <= used <= nslots for k, n_freed, used in src.seen), src.seen
    assert ring.n_got == ring.n_freed == 7 and sorted(ring.free) == list(range(nslots)) and not ring.staged and ring.stage_s > 0


def test_ring_stack_producers_take_a_shard_from_the_middle():
    frames, B = _stack(20), 3
    ring = S.StagingRing([np.zeros((B, 4, 5, 3), np.uint8) for _ in range(2)])
    ring.set_total(3)
    producers = [threading.Thread(target=S.stage_stack, args=(ring, frames, 5, 12, B, t, 2), daemon=True) for t in range(2)]
    con = _Consumer(ring)
    for th in producers + [con]:
        th.start()
    _join(producers + [con])
    assert con.error is None and [len(b) for b in con.got] == [3, 3, 1] and np.array_equal(np.concatenate(con.got), frames[5:12])


def _decoded(frames_iter, n_local, nslots=2, B=3):
    ring = S.StagingRing([np.zeros((B, 4, 5, 3), np.uint8) for _ in range(nslots)])
    producer = threading.Thread(target=S.stage_decoded, args=(ring, frames_iter, n_local, B), daemon=True, name="decode")
    con = _Consumer(ring)
    producer.start(), con.start()
    _join([producer, con])
    return ring, con


def test_ring_decoded_producer_publishes_a_short_last_batch_then_the_total():
    frames = _stack(10)
    ring, con = _decoded(iter(frames[:7]), 7)
    assert con.error is None and [len(b) for b in con.got] == [3, 3, 1] and np.array_equal(np.concatenate(con.got), frames[:7])
    # two slots: while the consumer holds batches 0 and 1 the producer cannot have finished -- the total is not known yet
    assert con.totals[:2] == [None, None] and ring.total == 3
    pulled = []
    ring, con = _decoded((pulled.append(i) or f for i, f in enumerate(frames)), 7)        # a decoder that runs past the shard's end
    assert con.error is None and np.array_equal(np.concatenate(con.got), frames[:7]) and ring.total == 3
    assert len(pulled) <= 8                                                              # (one look ahead at the most)
    ring, con = _decoded(iter(frames), 0)                                                # an empty shard
    assert con.error is None and con.got == [] and ring.total == 0


def test_ring_decoder_error_is_raised_in_the_consumer():
    frames, boom = _stack(10), KeyError("frame 4")

    def decoder():
        for i, f in enumerate(frames):
            if i == 4:
                raise boom
            yield f
    ring, con = _decoded(decoder(), 10)
    assert con.error is boom and len(con.got) <= 1                                       # (batch 1 never completes)


def test_ring_consumer_error_frees_a_producer_blocked_on_a_slot():
    frames, B = _stack(9), 3
    ring = S.StagingRing([np.zeros((B, 4, 5, 3), np.uint8)])
    ring.set_total(3)
    producer = threading.Thread(target=S.stage_stack, args=(ring, frames, 0, 9, B, 0, 1), daemon=True)
    producer.start()
    assert ring.get(0, None) == (0, 3)                     # the one slot is now the consumer's: the producer waits in take(1)
    ring.fail(RuntimeError("upload failed"))               # ... and the consumer leaves without giving it back
    _join([producer])
    assert 1 not in ring.staged and ring.free == []
    with pytest.raises(RuntimeError, match="upload failed"):
        ring.get(1, None)


def test_chunk_plan_geometry():
    small = 64 * 96 * 3 * 4
    assert S.chunk_plan(40, 1, 4, small, 2, 1 << 30) == (2, 5)          # test_estimate_pose_reruns_only_the_chunk_that_overflowed's
    assert S.chunk_plan(40, 1, 4, small, 64, 1 << 30) == (10, 1)
    # two ranks: 20 frames = 5 batches per rank -> 3 rounds; no argument is a rank's own, so a short shard runs the same rounds
    assert S.chunk_plan(40, 2, 4, small, 2, 1 << 30) == (2, 3) == S.chunk_plan(39, 2, 4, small, 2, 1 << 30)
    assert S.chunk_plan(10 ** 6, 1, 32, 32 * 480 * 640 * 3, 64, 1 << 30)[0] == 36        # the byte cap: 1 GiB of frames
    assert S.chunk_plan(10 ** 6, 1, 16, 16 * 720 * 1280 * 3, 64, 1 << 30)[0] == 24
    assert S.chunk_plan(3, 8, 4, small, 64, 1 << 30) == (1, 1)                           # fewer frames than ranks
    assert S.chunk_plan(0, 2, 4, small, 64, 1 << 30) == (1, 1)
    assert S.chunk_plan(40, 1, 4, 1 << 40, 64, 1 << 30) == (1, 10)                       # a batch larger than the cap: one batch per chunk


class _DecodeOnly:
    """a source without random access (a decoder)"""

    def __init__(self, frames):
        self.frames_, self.n_frames = frames, len(frames)

    def iter_frames(self):
        return iter(self.frames_)


def test_shard_frames_seek_skip_and_empty_shards():
    frames = _stack(10)

    def shard(source, lo, hi, world):
        first, rest = S.shard_frames(source, lo, hi, world, "clip")
        return np.stack([first] + list(rest))
    assert np.array_equal(shard(ArraySource(frames), 0, 10, 1), frames)
    for make in (ArraySource, _DecodeOnly):
        for rank in range(4):
            lo, hi = shard_range(10, rank, 4)                              # 3 + 3 + 3 + 1 frames
            assert np.array_equal(shard(make(frames), lo, hi, 4), frames[lo:hi]), (make.__name__, rank)
    assert shard_range(9, 3, 4) == (9, 9)
    first, rest = S.shard_frames(ArraySource(frames[:9]), 9, 9, 4, "clip")                # an empty shard: frame 0 for its size, no frames
    assert np.array_equal(first, frames[0]) and list(rest) == []
    # Kept as found, not fixed: a decoder has no frame left once it has skipped to an EMPTY shard (which always starts at the video's
    # end), so that rank raises where a seekable source goes on with frame 0 -- the other ranks are left alone in their collectives.
    with pytest.raises(ValueError, match="no frames in clip"):
        S.shard_frames(_DecodeOnly(frames[:9]), 9, 9, 4, "clip")
    for make in (ArraySource, _DecodeOnly):
        with pytest.raises(ValueError, match="no frames in clip"):
            S.shard_frames(make(frames[:0]), 0, 0, 1, "clip")
