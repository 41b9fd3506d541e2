"""The DGP drivers' device frame store (fit_dgp*(frame_store="hip"): staged._FrameStore, engine.gather_frames, csrc/dgp_frames.hip):
the gather against numpy indexing, its refusals, and the drivers' feeds against the frame_store="off" run of the same seeds."""
import contextlib
import io
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0xA5


def _store(rng, n_slots, H, W, pad=True):
    """-> (FrameSlots on the device, its frames as numpy [n_slots, H, W, 3]); the bytes between the frames are random too"""
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.models.staging import slot_stride
    fb = H * W * 3
    stride = slot_stride(fb) + (32 if pad else 0)
    host = rng.integers(0, 256, (n_slots, stride), dtype=np.uint8)
    return engine.FrameSlots(torch.from_numpy(host).to(DEV), (H, W)), host[:, :fb].reshape(n_slots, H, W, 3)


def _tables(rng, nt, n_slots, m):
    every = np.concatenate([np.arange(n_slots), -1 - np.arange(m)])
    mixed = rng.choice(every, nt)
    mixed[0], mixed[-1] = (n_slots - 1, -m) if nt > 1 else (-m, -m)
    return {"all store": rng.integers(0, n_slots, nt), "all patch": -1 - rng.integers(0, m, nt), "mixed": mixed,
            "one slot repeated": np.full(nt, n_slots // 2), "descending": np.sort(rng.integers(0, n_slots, nt))[::-1]}


def _expect(src, frames, patch):
    return np.stack([frames[s] if s >= 0 else patch[-1 - s] for s in src])


@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (33, 21), (64, 96)])
def test_gather_is_numpy_indexing_bit_for_bit(lib_built, hw):
    """every table kind at nt in {1, 2, 11, 12}, written into a view at an odd byte offset of a sentinel-filled buffer whose other bytes
    stay as they were; where the frame size allows 16-byte accesses, also into an aligned batch (the wide kernel)"""
    from deepgraphpose_amd import engine
    H, W = hw
    fb = H * W * 3
    rng = np.random.default_rng(H * 1000 + W)
    store, frames = _store(rng, 5, H, W)
    one, one_frames = _store(rng, 1, H, W, pad=False)
    patch = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    dpatch = torch.from_numpy(patch).to(DEV)
    for nt in (1, 2, 11, 12):
        cases = [(store, frames, k, v) for k, v in _tables(rng, nt, 5, 3).items()]
        cases.append((one, one_frames, "a one-slot store", np.where(np.arange(nt) % 3 == 2, -2, 0)))
        for st, fr, name, src in cases:
            want = _expect(src, fr, patch)
            for off in (7, 16) if fb % 16 == 0 else (7,):
                big = torch.full((off + nt * fb + 41,), SENTINEL, dtype=torch.uint8, device=DEV)
                out = big[off:off + nt * fb].view(nt, H, W, 3)
                got = engine.gather_frames(st, src, dpatch, out=out)
                assert got.data_ptr() == out.data_ptr()
                host = big.cpu().numpy()
                assert np.array_equal(host[off:off + nt * fb].reshape(nt, H, W, 3), want), (name, nt, off)
                assert (host[:off] == SENTINEL).all() and (host[off + nt * fb:] == SENTINEL).all(), (name, nt, off)
            got = engine.gather_frames(st, src, dpatch)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (name, nt)
    got = engine.gather_frames(store, [4, 0, 4])                 # no patch at all
    assert np.array_equal(got.cpu().numpy(), frames[[4, 0, 4]])
    none = engine.FrameSlots(torch.empty((0, store.data.shape[1]), dtype=torch.uint8, device=DEV), (H, W))
    got = engine.gather_frames(none, [-3, -1], dpatch)           # no store at all
    assert np.array_equal(got.cpu().numpy(), patch[[2, 0]])


def test_slot_offsets_are_64_bit(lib_built):
    """a 720 x 1280 store whose last slot starts above 2^32 bytes: slot 0 and the last slot come back"""
    from deepgraphpose_amd import engine
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 6 << 30:
        pytest.skip("needs 6 GiB of free device memory, %d bytes are free" % free)
    H, W = 720, 1280
    fb = H * W * 3
    n = (1 << 32) // fb + 2
    assert (n - 1) * fb > 1 << 32
    data = torch.empty((n, fb), dtype=torch.uint8, device=DEV)                   # (allocation only: nothing touches the middle)
    g = torch.Generator(device=DEV).manual_seed(0)
    first = torch.randint(0, 256, (fb,), dtype=torch.uint8, device=DEV, generator=g)
    last = torch.randint(0, 256, (fb,), dtype=torch.uint8, device=DEV, generator=g)
    data[0], data[n - 1] = first, last
    got = engine.gather_frames(engine.FrameSlots(data, (H, W)), [n - 1, 0])
    assert torch.equal(got[0].reshape(-1), last) and torch.equal(got[1].reshape(-1), first) and not torch.equal(first, last)


def test_refusals_happen_on_the_host(lib_built):
    from deepgraphpose_amd import engine
    from deepgraphpose_amd._lib import DgpError
    H, W = 16, 16
    rng = np.random.default_rng(1)
    store, _ = _store(rng, 4, H, W)
    patch = torch.from_numpy(rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)).to(DEV)
    out = torch.full((3, H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    for src, p in (([0, 4, 1], patch), ([0, -3, 1], patch), ([0, -1, 1], None),
                   ([0, 1, 2], torch.zeros((2, H, W + 1, 3), dtype=torch.uint8, device=DEV)),
                   ([0, 1, 2], torch.zeros((2, H + 1, W, 3), dtype=torch.uint8, device=DEV))):
        with pytest.raises(DgpError):
            engine.gather_frames(store, src, p, out=out)
    assert (out.cpu().numpy() == SENTINEL).all()                 # nothing ran
    with pytest.raises(DgpError):
        engine.gather_frames(engine.FrameSlots(store.data[:, :H * W * 3 - 16].contiguous(), (H, W)), [0])      # a pitch below the frame
    empty = engine.gather_frames(store, [], patch)
    assert tuple(empty.shape) == (0, H, W, 3) and empty.dtype == torch.uint8 and empty.is_cuda


# ---- the drivers: the stand-in trainer and session of tests/test_fit_prep_gpu.py, which record the feeds and train nothing ----------

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
    feeds, on_device, patched, reads = [], [], [], []
    source = None

    def __init__(self, trainer, graph):
        self.graph = graph

    def run(self, fetches, feed_dict):
        from deepgraphpose_amd.models import fitdgp
        from deepgraphpose_amd.staged import Staged
        inputs = [v for k, v in feed_dict.items() if k.name == "inputs"][0]
        inputs = inputs.tensor if isinstance(inputs, Staged) else inputs
        _Session.on_device.append(isinstance(inputs, torch.Tensor) and inputs.is_cuda)
        _Session.patched.append((fitdgp.PREP_STATS["frame_store"] or {}).get("patched"))
        _Session.reads.append(None if _Session.source is None else sum(_Session.source.count.values()))
        _Session.feeds.append({k.name: (None if v is None else _host(v)) for k, v in feed_dict.items()})
        return [{k: 0.0 for k in fetches[0]}, None]


class _CountingSource:
    """the project's ArraySource, counting frame_at per index"""

    def __init__(self, frames):
        from deepgraphpose_amd.frames import ArraySource
        self.inner, self.count = ArraySource(frames), {}
        self.n_frames, self.size, self.fps = self.inner.n_frames, self.inner.size, self.inner.fps

    def frame_at(self, i):
        self.count[int(i)] = self.count.get(int(i), 0) + 1
        return self.inner.frame_at(i)

    def iter_frames(self):
        return self.inner.iter_frames()

    def close(self):
        pass


class _Run:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _record(call, root, depth, frame_store, monkeypatch, counting=False):
    from scripts import fit_feed_digest as D
    from deepgraphpose_amd.models import fitdgp, session
    os.makedirs(root)
    proj = D.bare_project(root)
    monkeypatch.setattr(fitdgp, "PREFETCH_DEPTH", depth)
    monkeypatch.setattr(fitdgp, "_make_trainer", lambda *a, **k: _Trainer())
    monkeypatch.setattr(session, "TrainSession", _Session)
    monkeypatch.setenv("DGP_SNAPSHOT_FORMAT", "npz")
    source = _CountingSource(np.load(os.path.join(proj, "videos", "clip.npy"))) if counting else None
    _Session.feeds, _Session.on_device, _Session.patched, _Session.reads, _Session.source = [], [], [], [], source
    np.random.seed(0)
    random.seed(0)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        call(fitdgp, proj, dict(frame_store=frame_store, frame_sources=[source] if counting else None))
    return _Run(feeds=_Session.feeds, on_device=_Session.on_device, patched=_Session.patched, reads=_Session.reads, source=source,
                stdout=out.getvalue(), stats=fitdgp.PREP_STATS["frame_store"])


_START = "snapshot-step0-final--0"
_DGP = dict(batch_size=4, maxiters=6, gm2=1, gm3=3, n_max_frames=30, ns=3)
DRIVERS = {
    "labeledonly": lambda F, proj, kw: F.fit_dgp_labeledonly(_START, proj, maxiters=6, **kw),
    "dgp_aug": lambda F, proj, kw: F.fit_dgp(_START, proj, aug=True, **_DGP, **kw),
    "dgp": lambda F, proj, kw: F.fit_dgp(_START, proj, aug=False, **_DGP, **kw),
    "dgp_flow": lambda F, proj, kw: F.fit_dgp(_START, proj, aug=False, wt=50, flow_backend="hip", **_DGP, **kw),
}


def _same_feeds(off, hip):
    assert len(off) == len(hip) == 6
    for a, b in zip(off, hip):
        assert sorted(a) == sorted(b)
        for k in a:
            if a[k] is None:
                assert b[k] is None, k
                continue
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
        assert b["inputs"].dtype == np.uint8 and b["inputs"].ndim == 4


def test_each_selected_frame_is_decoded_once(lib_built, tmp_path, monkeypatch):
    from deepgraphpose_amd.models import fitdgp
    selected = {}
    real = fitdgp._frame_stores

    def spy(data_batcher, device, uploader):
        idxs = data_batcher.datasets[0].idxs
        selected["frames"] = sorted(set(int(i) for k in ("chunk", "pv", "ph") for i in idxs[k]))
        selected["before"] = dict(data_batcher.datasets[0].video_clip.count)
        stores = real(data_batcher, device, uploader)
        selected["after"] = dict(data_batcher.datasets[0].video_clip.count)
        return stores

    monkeypatch.setattr(fitdgp, "_frame_stores", spy)
    run = _record(DRIVERS["dgp"], str(tmp_path / "hip"), 2, "hip", monkeypatch, counting=True)
    assert len(run.feeds) == 6 and all(run.on_device)
    assert selected["before"] == {}                                           # selecting the frames reads none through frame_at
    assert selected["after"] == {f: 1 for f in selected["frames"]}            # the fill: every selected frame once, no other frame
    assert run.source.count == selected["after"]                              # the six iterations: none
    assert len(selected["frames"]) > 4 and run.stats["frames"] == len(selected["frames"]) and run.stats["refused"] == 0
    assert run.stats["bytes"] == len(selected["frames"]) * 64 * 96 * 3 and run.stats["patched"] == 0
    assert run.stdout.count("frame store: ") == 1 and "filled in" in run.stdout


@pytest.mark.parametrize("name", list(DRIVERS))
@pytest.mark.parametrize("depth", [0, 2])
def test_feeds_are_the_host_paths(lib_built, tmp_path, monkeypatch, name, depth):
    """6 iterations: every feed of the "hip" run is the "off" run's, bytes and shapes, `inputs` included -- there a device tensor"""
    off = _record(DRIVERS[name], str(tmp_path / "off"), depth, "off", monkeypatch)
    hip = _record(DRIVERS[name], str(tmp_path / "hip"), depth, "hip", monkeypatch)
    assert off.stats is None and hip.stats["frames"] > 0 and hip.stats["refused"] == 0
    _same_feeds(off.feeds, hip.feeds)
    assert all(hip.on_device)
    if name == "dgp_flow":
        assert all(f["vector_field_tf"] is not None and f["vector_field_tf"].any() for f in hip.feeds)
    if name == "dgp_aug":
        assert any(not np.array_equal(a["targets"], b["targets"]) for a, b in zip(hip.feeds, _record(
            DRIVERS["dgp"], str(tmp_path / "plain"), depth, "hip", monkeypatch).feeds))          # (the augmentation did run)


def test_a_store_over_its_budget_patches_the_rest(lib_built, tmp_path, monkeypatch):
    """FRAME_STORE_BYTES for all but 7 of the selected frames: the 4 labeled frames give way first (their host copies are kept), then the
    3 highest unlabeled ones; every batch has a labeled frame, so batches mix slots and patches, and the feeds do not change"""
    from deepgraphpose_amd import staged
    off = _record(DRIVERS["dgp"], str(tmp_path / "off"), 0, "off", monkeypatch)
    full = _record(DRIVERS["dgp"], str(tmp_path / "full"), 0, "hip", monkeypatch, counting=True)
    k = full.stats["frames"] - 7
    assert k > 4
    monkeypatch.setattr(staged, "FRAME_STORE_BYTES", k * 64 * 96 * 3 + 100)
    hip = _record(DRIVERS["dgp"], str(tmp_path / "hip"), 0, "hip", monkeypatch, counting=True)
    _same_feeds(off.feeds, hip.feeds)
    assert all(hip.on_device)
    assert hip.stats["frames"] == k and hip.stats["refused"] == 7 and hip.stats["bytes"] == k * 64 * 96 * 3
    assert hip.stdout.count("do not fit") == 1                                # announced once
    nts = [f["inputs"].shape[0] for f in hip.feeds]
    assert all(p >= 1 for p in hip.patched) and any(0 < p < nt for p, nt in zip(hip.patched, nts))       # (depth 0: patched is this batch's)
    # the fill reads the k stored frames and the 4 labeled ones once each; after it only the 3 refused unlabeled frames are ever read
    selected = sorted(full.source.count)
    refused = sorted(f for f in selected if f not in (3, 11, 19, 30))[-3:]
    assert sorted(set(hip.source.count) - set(refused)) == sorted(set(selected) - set(refused))
    assert all(c == 1 for f, c in hip.source.count.items() if f not in refused)
    assert k + 4 <= hip.reads[0] <= k + 4 + 3 and hip.reads[-1] == sum(hip.source.count.values())


def test_one_real_run(lib_built, tmp_path, monkeypatch):
    """fit_dgp(frame_store="hip") with the real Trainer, 3 iterations on the 64 x 96 synthetic project"""
    from _project import make_project
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.models import fitdgp, session
    from deepgraphpose_amd.models.fitdgp_util import get_snapshot_path
    proj, _, _ = make_project(tmp_path, hw=(64, 96))
    monkeypatch.setenv("DGP_SNAPSHOT_FORMAT", "npz")
    losses = []
    real_run = session.TrainSession.run

    def run(self, fetches, feed_dict):
        res = real_run(self, fetches, feed_dict)
        losses.append(dict(res[0]))
        return res

    monkeypatch.setattr(session.TrainSession, "run", run)
    np.random.seed(0)
    random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        fitdgp.fit_dgp(_START, proj, batch_size=4, maxiters=3, displayiters=1, gm2=1, gm3=3, n_max_frames=30, ns=3, frame_store="hip")
    assert len(losses) == 3 and all(np.isfinite(float(v)) for l in losses for v in l.values())
    assert fitdgp.PREP_STATS["frame_store"]["frames"] > 0
    snap, _ = get_snapshot_path("snapshot-step2-final--0", proj, shuffle=1)
    assert weights_io.exists(snap)
    assert all(np.isfinite(v).all() for v in weights_io.load_weights(snap).values())
