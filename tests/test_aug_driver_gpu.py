"""fit_dgp_labeledonly / fit_dgp with aug_backend="hip" against aug_backend="host" under the same seeds: the stand-in trainer and session
of tests/test_frame_store_gpu.py record the feeds and train nothing; the project is tests/_project.py's."""
import contextlib
import copy
import io
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
H, W = 64, 96


def _host(x):
    from deepgraphpose_amd.staged import Staged, _on_current_stream
    if isinstance(x, Staged) or isinstance(x, torch.Tensor):
        t = _on_current_stream(x)
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return np.asarray(x)


class _Trainer:
    device = DEV

    def get_weights(self):
        return {"pose/part_pred/block4/biases": np.zeros(3, dtype=np.float32)}


class _Session:
    feeds, patched = [], []

    def __init__(self, trainer, graph):
        self.graph = graph

    def run(self, fetches, feed_dict):
        from deepgraphpose_amd.models import fitdgp
        _Session.patched.append((fitdgp.PREP_STATS["frame_store"] or {}).get("patched"))
        _Session.feeds.append({k.name: (None if v is None else _host(v)) for k, v in feed_dict.items()})
        return [{k: 0.0 for k in fetches[0]}, None]


class _Run:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _record(call, root, monkeypatch, depth=2, trainer=_Trainer, **kw):
    """one driver call on a fresh project: its feeds, the device augmentation calls (positions, plans), a twin of its pipeline as built"""
    from scripts import fit_feed_digest as D
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.models import fitdgp, session
    os.makedirs(root)
    proj = D.bare_project(root)
    calls, twins = [], []
    real_pipeline = getattr(fitdgp._aug_pipeline, "real", fitdgp._aug_pipeline)        # (a test records several runs: never spy on a spy)
    real_augment = getattr(engine.augment_frames, "real", engine.augment_frames)

    def pipeline_spy(dgp_cfg, aug_backend="host"):
        p = real_pipeline(dgp_cfg, aug_backend)
        twins.append(copy.deepcopy(p))
        return p

    def augment_spy(frames, plans, positions):
        calls.append(([int(p) for p in positions], list(plans), tuple(frames.shape)))
        return real_augment(frames, plans, positions)

    pipeline_spy.real, augment_spy.real = real_pipeline, real_augment
    monkeypatch.setattr(fitdgp, "PREFETCH_DEPTH", depth)
    monkeypatch.setattr(fitdgp, "_make_trainer", lambda *a, **k: trainer())
    monkeypatch.setattr(fitdgp, "_aug_pipeline", pipeline_spy)
    monkeypatch.setattr(engine, "augment_frames", augment_spy)
    monkeypatch.setattr(session, "TrainSession", _Session)
    monkeypatch.setenv("DGP_SNAPSHOT_FORMAT", "npz")
    _Session.feeds, _Session.patched = [], []
    np.random.seed(0)
    random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        call(fitdgp, proj, kw)
    return _Run(feeds=_Session.feeds, patched=_Session.patched, calls=calls, twin=twins[0] if twins else None,
                stats=copy.deepcopy(fitdgp.PREP_STATS))


_START = "snapshot-step0-final--0"
_DGP = dict(batch_size=4, maxiters=6, gm2=1, gm3=3, n_max_frames=30, ns=3)
DRIVERS = {
    "labeledonly": lambda F, proj, kw: F.fit_dgp_labeledonly(_START, proj, maxiters=6, **kw),
    "dgp": lambda F, proj, kw: F.fit_dgp(_START, proj, **_DGP, **kw),
}


def _stage_names(plan):
    return [s for s, _ in plan]


@pytest.mark.parametrize("frame_store", ["off", "hip"])
@pytest.mark.parametrize("name", list(DRIVERS))
def test_hip_augmentation_feeds_what_the_host_feeds(lib_built, tmp_path, monkeypatch, name, frame_store):
    """6 iterations: labels, locref maps and masks and index sets are the host run's bytes; so is every frame of `inputs` that is not
    labeled, and every labeled one whose plan holds neither elastic nor noise; the statistics are a twin pipeline's plans"""
    from deepgraphpose_amd.augment import plan_stages
    host = _record(DRIVERS[name], str(tmp_path / "host"), monkeypatch, frame_store=frame_store, aug_backend="host")
    hip = _record(DRIVERS[name], str(tmp_path / "hip"), monkeypatch, frame_store=frame_store, aug_backend="hip")
    assert len(host.feeds) == len(hip.feeds) == 6 and not host.calls
    assert len(hip.calls) == 6                                   # every batch of these drivers has a labeled frame
    inexact = 0
    for a, b, (positions, plans, shape) in zip(host.feeds, hip.feeds, hip.calls):
        assert sorted(a) == sorted(b)
        for k in a:
            if k == "inputs":
                continue
            if a[k] is None:
                assert b[k] is None, k
                continue
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
        fa, fb = a["inputs"], b["inputs"]
        assert fb.dtype == np.uint8 and fb.shape == shape and fa.shape == fb.shape
        fa = np.clip(np.rint(fa), 0, 255).astype(np.uint8)
        others = [i for i in range(shape[0]) if i not in positions]
        assert np.array_equal(fa[others], fb[others])
        assert (name == "labeledonly") == (not others)
        for pos, plan in zip(positions, plans):
            assert all(p["key"] is not None and p["field"] is None for s, p in plan if s == "gaussian_noise")
            if {"elastic", "gaussian_noise"} & set(_stage_names(plan)):
                inexact += 1
                assert np.abs(fa[pos].astype(int) - fb[pos]).mean() < 16      # (the same picture under another noise stream)
            else:
                assert np.array_equal(fa[pos], fb[pos]), _stage_names(plan)
    assert inexact > 0
    # the statistics: what a twin of the run's pipeline plans for as many frames
    plans = [p for _, ps, _ in hip.calls for p in ps]
    twin = [hip.twin.plan(H, W, noise="key") for _ in plans]
    assert [_stage_names(p) for p in twin] == [_stage_names(p) for p in plans]
    want = {"frames": len(plans), "stages": plan_stages(twin)}
    assert hip.stats["aug"] == dict(want, backend="hip") and host.stats["aug"] == dict(want, backend="host")
    assert sum(want["stages"].values()) > 0
    if frame_store == "hip":                                     # the augmented frames are made on the device: nothing is patched
        assert hip.stats["frame_store"]["refused"] == 0 and all(p == 0 for p in hip.patched)
        assert any(p for p in host.patched)


def test_prefetch_depth_zero_runs_on_the_current_stream(lib_built, tmp_path, monkeypatch):
    a = _record(DRIVERS["dgp"], str(tmp_path / "a"), monkeypatch, depth=0, frame_store="hip", aug_backend="hip")
    b = _record(DRIVERS["dgp"], str(tmp_path / "b"), monkeypatch, depth=2, frame_store="off", aug_backend="hip")
    assert len(a.feeds) == len(b.feeds) == 6
    for x, y in zip(a.feeds, b.feeds):                           # the same plans, the same keys: the same bytes, inputs included
        assert sorted(x) == sorted(y)
        assert all((x[k] is None and y[k] is None) or np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f") for k in x)


def test_no_augmentation_without_aug_and_with_the_temporal_clique(lib_built, tmp_path, monkeypatch):
    off = _record(DRIVERS["dgp"], str(tmp_path / "off"), monkeypatch, aug=False, aug_backend="hip")
    assert len(off.feeds) == 6 and not off.calls and off.stats["aug"] is None and off.twin is None
    wt = _record(DRIVERS["dgp"], str(tmp_path / "wt"), monkeypatch, wt=50, flow_backend="hip", aug_backend="hip")
    assert len(wt.feeds) == 6 and not wt.calls                   # fitdgp.py:778-779: wt > 0 trains on the frames as they are
    assert wt.stats["aug"] == {"backend": "hip", "frames": 0, "stages": {}}


def test_hip_augmentation_needs_a_gpu_trainer(lib_built, tmp_path, monkeypatch):
    class HostTrainer(_Trainer):
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="aug_backend"):
        _record(DRIVERS["dgp"], str(tmp_path / "cpu"), monkeypatch, trainer=HostTrainer, aug_backend="hip")
    assert not _Session.feeds
    from deepgraphpose_amd.models import fitdgp
    with pytest.raises(ValueError):
        fitdgp.fit_dgp(_START, str(tmp_path / "nowhere"), aug_backend="device")        # (the name is checked before anything is opened)
