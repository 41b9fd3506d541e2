"""The DGP fit drivers' host side without a GPU: trainer, session and frame uploader are the recorders of scripts/fit_feed_digest.py, so a
run is set-up, schedule, batches, prints and snapshot names alone.  Plus the Staged pair (deepgraphpose_amd/staged.py) against a stub stream."""
import numpy as np
import pytest
import torch

from scripts import fit_feed_digest as D

STEP1 = ["snapshot-step1--0", "snapshot-step1--5", "snapshot-step1-final--0"]
STEP2 = ["snapshot-step2--0", "snapshot-step2--5", "snapshot-step2-final--0"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """fit_dgp_labeledonly(maxiters=6) and fit_dgp(..., aug=True), each built inline (PREFETCH_DEPTH 0) and on the prefetch thread (2)"""
    tmp = tmp_path_factory.mktemp("fit")
    return {(name, depth): D.run_case(name, tmp / ("depth%d" % depth), depth) for name in ("labeledonly", "dgp_aug") for depth in (0, 2)}


@pytest.mark.parametrize("name,objective", [("labeledonly", "total_loss_visible"), ("dgp_aug", "total_loss")])
def test_feed_sequence_is_the_same_inline_and_prefetched(runs, name, objective):
    inline, ahead = runs[name, 0], runs[name, 2]
    assert len(inline["digests"]) == 6 and len(set(inline["digests"])) > 1
    assert ahead["digests"] == inline["digests"] and ahead["stdout"] == inline["stdout"]
    assert inline["objectives"] == ahead["objectives"] == [objective]
    assert (inline["uploader_calls"], ahead["uploader_calls"]) == (0, 6)          # no uploader inline; one upload per batch otherwise


@pytest.mark.parametrize("name,expected,done", [("labeledonly", STEP1, "exists! DGP with labeled frames has already been run."),
                                                ("dgp_aug", STEP2, "exists! DGP has already been run.")])
def test_snapshot_names_and_the_skip_if_exists_guard(runs, capsys, name, expected, done):
    for depth in (0, 2):
        assert runs[name, depth]["snapshots"] == expected and runs[name, depth]["returned"] == "None"
    with D.recorders(2) as fitdgp:
        assert D.CASES[name](fitdgp, runs[name, 2]["proj"]) is None               # the final snapshot is there: nothing is trained
        assert D.RecordingSession.digests == [] and D.FakeUploader.calls == 0
    assert done in capsys.readouterr().out


@pytest.mark.parametrize("name,call,snapshots", [
    ("labeledonly", lambda F, proj: F.fit_dgp_labeledonly(D.START, proj, maxiters=6, aug=False),
     ["snapshot-step1--0", "snapshot-step1--2", "snapshot-step1-final--0"]),
    ("dgp", D.CASES["dgp"], ["snapshot-step2--0", "snapshot-step2--2", "snapshot-step2-final--0"])])
def test_two_ranks_interleave_the_schedule_and_rank0_alone_saves(tmp_path, monkeypatch, name, call, snapshots):
    """W = 2: both ranks draw the same 6-entry schedule, iteration `it` of rank r trains on entry (it * 2 + r) % 6 -- the batch the
    single-process run feeds at that iteration -- and rank 0 alone writes.  (Without augmentation, and with the labeled frame that fit_dgp
    draws for a window that has none pinned to the first, a batch is a function of its entry alone.)"""
    from deepgraphpose_amd import dist as ddist
    from deepgraphpose_amd.models import fitdgp
    monkeypatch.setattr(fitdgp, "randint", lambda lo, hi: lo)
    single = D.run_case(name, tmp_path / "single", call=call)["digests"]
    assert len(single) == 6 and len(set(single)) > 1
    monkeypatch.setattr(ddist, "data_parallel", lambda group=None: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    for r in (0, 1):
        monkeypatch.setattr(torch.distributed, "get_rank", lambda group=None: r)
        monkeypatch.setattr(fitdgp, "_dp_setup", lambda: (r, 2, 0))
        rec = D.run_case(name, tmp_path / ("rank%d" % r), call=call)
        assert rec["digests"] == [single[(it * 2 + r) % 6] for it in range(3)], r
        assert rec["snapshots"] == (snapshots if r == 0 else []), r
        assert "Begin Training for 3 iterations" in rec["stdout"]


class _Stream:
    def __init__(self):
        self.waits = []

    def wait_event(self, ev):
        self.waits.append(ev)


class _Trainer:
    device = "cpu"

    def __init__(self, h, w):
        self.net, self.sizes = self, []
        self.in_h, self.in_w = h, w

    def set_input_size(self, h, w):
        self.sizes.append((h, w))
        self.in_h, self.in_w = h, w


def test_staged_pair_carries_its_event_through_a_slice(monkeypatch):
    """_frames_to_device makes the current stream wait for a Staged pair's event and for nothing else; the event is a member of the pair,
    so a tensor derived from the pair's (here a slice, a new tensor object) wrapped with the same event keeps the wait."""
    from deepgraphpose_amd.staged import Staged, _frames_to_device
    cur, recorded = _Stream(), []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: cur)
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, stream: recorded.append((self, stream)), raising=False)
    tr = _Trainer(16, 16)
    ev = object()
    pair = Staged(torch.arange(3 * 8 * 12 * 3, dtype=torch.uint8).reshape(3, 8, 12, 3), ev)
    out = _frames_to_device(tr, pair)
    assert out is pair.tensor and cur.waits == [ev] and tr.sizes == [(8, 12)]
    assert len(recorded) == 1 and recorded[0][0] is pair.tensor and recorded[0][1] is cur
    part = Staged(pair.tensor[:2], pair.ready)
    assert part.tensor is not pair.tensor
    assert _frames_to_device(tr, part) is part.tensor and cur.waits == [ev, ev] and len(recorded) == 2
    assert _frames_to_device(tr, Staged(pair.tensor, None)) is pair.tensor and cur.waits == [ev, ev] and len(recorded) == 3
    with pytest.raises(AttributeError):
        pair.ready = None                                           # immutable
    # no pair, no wait: a bare tensor and a numpy array (here on the host, so they take the upload path; float frames are rounded)
    for bare in (pair.tensor[:2], pair.tensor.numpy(), np.full((1, 8, 12, 3), 7.6)):
        got = _frames_to_device(tr, bare)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), np.clip(np.rint(np.asarray(bare)), 0, 255))
    assert cur.waits == [ev, ev] and len(recorded) == 3 and tr.sizes == [(8, 12)]


def test_session_batch_recognises_the_pair():
    """TrainSession._batch hands a Staged pair on as it is and counts its frames for the nt_batch_pl check."""
    from deepgraphpose_amd.loss import DGPHyper
    from deepgraphpose_amd.models.session import LossGraph, TrainSession
    from deepgraphpose_amd.staged import Staged
    g = LossGraph(DGPHyper(), np.zeros((2, 3)), np.ones(2), np.ones(2), 40, 2, 3)
    ph = g.placeholders
    pair = Staged(torch.zeros((3, 16, 16, 3), dtype=torch.uint8), None)
    feed = {ph[k]: np.zeros(1) for k in ("targets", "locref_map", "locref_mask", "visible_marker_pl", "hidden_marker_pl",
                                         "visible_marker_in_targets_pl")}
    feed.update({ph["inputs"]: pair, ph["nt_batch_pl"]: 3})
    images, _ = TrainSession(None, g)._batch(feed)
    assert images is pair
    feed[ph["nt_batch_pl"]] = 4
    with pytest.raises(ValueError, match="inputs hold 3 frames"):
        TrainSession(None, g)._batch(feed)
    feed.update({ph["inputs"]: [np.zeros((16, 16, 3), np.uint8)] * 4})           # a list of frames is still a host array
    assert TrainSession(None, g)._batch(feed)[0].shape == (4, 16, 16, 3)
