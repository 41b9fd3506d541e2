"""The fit drivers' samples built on the device (prep_backend="hip": staged._device_sample / _device_locref) against the host path of
the same commit: frames and maps bit for bit; the drivers run on it and say which backend ran."""
import contextlib
import io
import os
import random

import numpy as np
import pytest
import torch

import _fit_prep as P

pytestmark = pytest.mark.gpu


def _host(x):
    from deepgraphpose_amd.staged import Staged, _on_current_stream
    if isinstance(x, Staged) or isinstance(x, torch.Tensor):
        t = _on_current_stream(x)
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return np.asarray(x)


@pytest.fixture(scope="module")
def reaching(tmp_path_factory):
    """20 seeded samples of the Reaching project through the host path, computed once"""
    cfg = P.reaching_cfg(tmp_path_factory.mktemp("reaching"))
    ds = P.seeded_dataset(cfg, 3)
    return cfg, [ds.next_batch() for _ in range(20)]


@pytest.mark.parametrize("with_uploader", [False, True])
def test_device_samples_are_the_host_samples_bit_for_bit(lib_built, reaching, with_uploader):
    from deepgraphpose_amd.staged import _FrameUploader, _ImageCache, _device_sample
    cfg, host = reaching
    dev = torch.device("cuda", 0)
    uploader = _FrameUploader(dev) if with_uploader else None
    ds = P.seeded_dataset(cfg, 3)
    cache = _ImageCache(ds, dev, uploader)
    plans = [ds.plan_batch() for _ in range(20)]
    assert sum(p.crop is not None for p in plans) >= 3 and sum(p.crop is None for p in plans) >= 3
    for p, b in zip(plans, host):
        frames, maps = _device_sample(ds, p, cache, uploader, dev)
        assert (frames.ready is not None) == with_uploader and all(m.ready is frames.ready for m in maps.values())
        assert np.array_equal(_host(frames), b["inputs"]), p.item.im_path
        for k in P.MAP_KEYS:
            assert maps[k].tensor.dtype == torch.float32 and np.array_equal(_host(maps[k]), b[k]), (k, p.item.im_path)
    assert 0 < len(cache.images) <= 20 and not cache.refused


def test_an_image_over_the_cache_cap_takes_the_host_pixels(lib_built, reaching, monkeypatch, capsys):
    from deepgraphpose_amd import staged
    cfg, host = reaching
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(staged, "IMAGE_CACHE_BYTES", 1000)                      # below one 747 x 832 image
    ds = P.seeded_dataset(cfg, 3)
    cache = staged._ImageCache(ds, dev, None)
    for b in host[:4]:
        frames, maps = staged._device_sample(ds, ds.plan_batch(), cache, None, dev)
        assert np.array_equal(_host(frames), b["inputs"]) and all(np.array_equal(_host(maps[k]), b[k]) for k in P.MAP_KEYS)
    assert not cache.images and cache.refused and cache.bytes == 0
    assert capsys.readouterr().out.count("does not fit") == 1                   # announced once


def _fit_dlc_project(tmp_path):
    """tests/_project.py's project with its seeded snapshot renamed: fit_dlc starts from it and has its own final snapshot to write"""
    from _project import make_project
    from deepgraphpose_amd.models.fitdgp_util import get_snapshot_path
    proj, _, _ = make_project(tmp_path, hw=(96, 128))
    snap0, _ = get_snapshot_path("snapshot-step0-final--0", proj, shuffle=1)
    for ext in (".index", ".data-00000-of-00001"):
        os.rename(snap0 + ext, os.path.join(os.path.dirname(snap0), "snapshot-start") + ext)
    return proj, snap0


@pytest.mark.parametrize("backend", ["hip", "host"])
def test_fit_dlc_runs_on_either_backend(lib_built, tmp_path, monkeypatch, backend):
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.models import fitdgp
    proj, snap0 = _fit_dlc_project(tmp_path)
    monkeypatch.setenv("DGP_SNAPSHOT_FORMAT", "npz")              # (the run's own snapshots: quicker to write than TF bundles)
    np.random.seed(0)
    random.seed(0)
    fitdgp.PREP_STATS["backend"] = None
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        fitdgp.fit_dlc("snapshot-start", proj, maxiters=5, displayiters=1, prep_backend=backend)
    assert fitdgp.PREP_STATS["backend"] == backend
    assert weights_io.exists(snap0)
    w = weights_io.load_weights(snap0)
    assert all(np.isfinite(v).all() for v in w.values())
    losses = [float(l.split("loss: total loss ")[1].split()[0]) for l in out.getvalue().splitlines() if l.startswith("iteration:")]
    assert len(losses) == 5 and np.isfinite(losses).all()
    with pytest.raises(ValueError, match="prep backend"):
        fitdgp.fit_dlc("snapshot-start", proj, maxiters=5, prep_backend="gpu")


class _Trainer:
    """Stands in for the trainer: the drivers' batches are recorded, nothing is trained (as scripts/fit_feed_digest.py does on the host)"""
    device = torch.device("cuda", 0)

    def get_weights(self):
        return {"pose/part_pred/block4/biases": np.zeros(3, dtype=np.float32)}


class _Session:
    feeds = []

    def __init__(self, trainer, graph):
        self.graph = graph

    def run(self, fetches, feed_dict):
        _Session.feeds.append({k.name: (None if v is None else _host(v)) for k, v in feed_dict.items()})
        return [{k: 0.0 for k in fetches[0]}, None]


def _record(call, root, depth, backend, monkeypatch):
    from scripts import fit_feed_digest as D
    from deepgraphpose_amd.models import fitdgp, session
    os.makedirs(root)
    proj = D.bare_project(root)
    monkeypatch.setattr(fitdgp, "PREFETCH_DEPTH", depth)
    monkeypatch.setattr(fitdgp, "_make_trainer", lambda *a, **k: _Trainer())
    monkeypatch.setattr(session, "TrainSession", _Session)
    monkeypatch.setenv("DGP_SNAPSHOT_FORMAT", "npz")
    _Session.feeds = []
    np.random.seed(0)
    random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        call(fitdgp, proj, backend)
    assert fitdgp.PREP_STATS["backend"] == backend
    return _Session.feeds


DRIVERS = {
    "labeledonly": lambda F, proj, b: F.fit_dgp_labeledonly("snapshot-step0-final--0", proj, maxiters=6, prep_backend=b),
    "dgp_aug": lambda F, proj, b: F.fit_dgp("snapshot-step0-final--0", proj, batch_size=4, maxiters=6, gm2=1, gm3=3, n_max_frames=30,
                                            ns=3, aug=True, prep_backend=b),
}


@pytest.mark.parametrize("name", list(DRIVERS))
@pytest.mark.parametrize("depth", [0, 2])
def test_dgp_drivers_feed_the_host_maps_from_the_device(lib_built, tmp_path, monkeypatch, name, depth):
    """6 iterations: every feed of the "hip" run equals the "host" run's, the two locref maps included (there: _locref_targets' arrays)"""
    host = _record(DRIVERS[name], str(tmp_path / "host"), depth, "host", monkeypatch)
    hip = _record(DRIVERS[name], str(tmp_path / "hip"), depth, "hip", monkeypatch)
    assert len(host) == len(hip) == 6
    seen = False
    for a, b in zip(host, hip):
        assert sorted(a) == sorted(b)
        for k in a:
            if a[k] is None:
                assert b[k] is None
                continue
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
        assert b["locref_map"].dtype == np.float32 and b["locref_map"].ndim == 4
        seen = seen or bool(a["locref_mask"].any())
    assert seen


def test_loss_inputs_take_device_maps_in_place(lib_built):
    """dgp_loss_prepare with Staged / device locref maps: they are used in place, every other field is what the host maps give"""
    from deepgraphpose_amd import dataset as D
    from deepgraphpose_amd.loss import DGPHyper, dgp_loss_prepare
    from deepgraphpose_amd.staged import Staged, _device_locref
    nt, H, W, nj = 3, 6, 8, 3
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    jl = np.stack([rng.uniform(1, H - 2, (1, nj)), rng.uniform(1, W - 2, (1, nj))], -1)
    vm, hm, vt = D.gen_idx_chunk(np.array([1]), np.array([0, 2]), jl)
    lt, lm = D.coord2map(jl, H, W, nj, 17)
    lmap, lmask = np.zeros((nt, H, W, 2 * nj), np.float32), np.zeros((nt, H, W, 2 * nj), np.float32)
    lmap[1], lmask[1] = lt[0], lm[0]
    cfg = type("Cfg", (), dict(pos_dist_thresh=17, locref_stdev=7.2801))
    dmap, dmask = _device_locref(None, dev, jl, nt, [1], H, W, nj, cfg)
    batch = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt)
    S0 = np.zeros((2, nj))
    args = (DGPHyper(), S0, np.ones(2), np.ones(2), 40.0, 4.0, dev)
    ref = dgp_loss_prepare(nt, H, W, nj, batch, *args)
    for maps in ((dmap, dmask), (dmap.tensor, dmask.tensor)):
        li = dgp_loss_prepare(nt, H, W, nj, dict(batch, locref_map=maps[0], locref_mask=maps[1]), *args)
        assert li.lmap.data_ptr() == dmap.tensor.data_ptr() and li.lmask.data_ptr() == dmask.tensor.data_ptr()
        torch.cuda.synchronize()
        for f in ("targets", "lmap", "lmask", "vm", "hm", "vt", "S0", "ws", "ws_max"):
            assert np.array_equal(getattr(li, f).cpu().numpy(), getattr(ref, f).cpu().numpy()), f
        assert bytes(li.desc) == bytes(ref.desc) and li.scratch.numel() == ref.scratch.numel() and li.vf is None
    assert ref.lmask.any().item()
    with pytest.raises(ValueError, match="locref_map"):
        dgp_loss_prepare(nt, H, W, nj, dict(batch, locref_map=Staged(dmap.tensor[:2], None)), *args)
