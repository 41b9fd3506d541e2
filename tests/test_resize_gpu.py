"""HIP resize + crop (csrc/dgp_resize.hip, engine.resize_frames) against Pillow itself, byte for byte, and estimate_pose fed from it
(resize_backend "hip" against "pil")."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _pil_resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BATCH = 3
# the seven shapes of the contract (a ~9 x reduction with windows clipped at both borders and longer than a tile's rows; an upscale;
# the two one-axis shapes where Pillow skips a pass; the identity) + an output width that is no multiple of the 64-pixel tile, its
# tail narrower than a wave
SHAPES = R.SHAPES + [((40, 200), (20, 70))]


@functools.lru_cache(maxsize=None)
def _frames(H, W):
    x = R.test_image(H, W, batch=BATCH)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _pillow(H, W, new_size, crop_size):
    """what estimate_pose's host preparation makes of every frame (computed once per case, never changed)"""
    from PIL import Image
    out = []
    for f in _frames(H, W):
        im = Image.fromarray(f)
        if new_size is not None:
            im = im.resize(size=(new_size[1], new_size[0]))
        if crop_size is not None:
            im = im.crop(crop_size)
        out.append(np.asarray(im))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()


@pytest.mark.parametrize("src,dst", SHAPES, ids=lambda v: "%dx%d" % v)
def test_resize_frames_is_pillow_byte_for_byte(lib_built, src, dst):
    from deepgraphpose_amd import engine
    (H, W) = src
    got = engine.resize_frames(_dev(_frames(H, W)), new_size=dst)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (BATCH,) + dst + (3,)
    want = _pillow(H, W, dst, None)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ, max |d| %d" % ((got != want).sum(), np.abs(got.astype(int) - want).max())


def test_crop_only(lib_built):
    from deepgraphpose_amd import engine
    box = (8, 16, 136, 112)
    got = engine.resize_frames(_dev(_frames(120, 160)), crop_size=box)
    assert tuple(got.shape) == (BATCH, 96, 128, 3)
    assert np.array_equal(got.cpu().numpy(), _pillow(120, 160, None, box))
    assert np.array_equal(got.cpu().numpy(), _frames(120, 160)[:, 16:112, 8:136])


def test_resize_then_crop_partly_outside_writes_zeros(lib_built):
    from deepgraphpose_amd import engine
    box = (-4, -3, 50, 40)
    out = torch.full((BATCH, 43, 54, 3), 77, dtype=torch.uint8, device="cuda")          # (stale bytes must not survive)
    got = engine.resize_frames(_dev(_frames(97, 131)), new_size=(72, 96), crop_size=box, out=out).cpu().numpy()
    want = _pillow(97, 131, (72, 96), box)
    assert np.array_equal(got, want)
    assert not got[:, :3].any() and not got[:, :, :4].any() and got[:, 3:, 4:].any()
    # a box beyond the right / lower edge, and one wholly outside the image
    for box in ((60, 50, 130, 90), (200, 10, 230, 30)):
        got = engine.resize_frames(_dev(_frames(97, 131)), new_size=(72, 96), crop_size=box).cpu().numpy()
        assert np.array_equal(got, _pillow(97, 131, (72, 96), box)), box


def test_out_is_filled_in_place_and_nothing_else(lib_built):
    from deepgraphpose_amd import engine
    fr = _dev(_frames(120, 160))
    big = torch.full((BATCH + 2, 61, 83, 3), 201, dtype=torch.uint8, device="cuda")
    ret = engine.resize_frames(fr, new_size=(61, 83), out=big[1:1 + BATCH])
    assert ret.data_ptr() == big[1].data_ptr()
    assert np.array_equal(big[1:1 + BATCH].cpu().numpy(), _pillow(120, 160, (61, 83), None))
    assert bool((big[0] == 201).all()) and bool((big[-1] == 201).all())              # the frames around the view are untouched
    with pytest.raises(Exception):
        engine.resize_frames(fr, new_size=(61, 83), out=big[:BATCH, :60])


def test_deterministic_and_batch_independent(lib_built):
    from deepgraphpose_amd import engine
    fr = _dev(_frames(97, 131))
    a = engine.resize_frames(fr, new_size=(72, 96), crop_size=(-4, -3, 50, 40))
    b = engine.resize_frames(fr, new_size=(72, 96), crop_size=(-4, -3, 50, 40))
    assert torch.equal(a, b)
    for i in range(BATCH):
        assert torch.equal(engine.resize_frames(fr[i:i + 1], new_size=(72, 96), crop_size=(-4, -3, 50, 40))[0], a[i]), i
    # a frame whose first byte is not dword-aligned in memory (a view into a flat buffer at an odd offset)
    flat = torch.zeros(1 + 33 * 47 * 3, dtype=torch.uint8, device="cuda")
    flat[1:] = _dev(_frames(33, 47))[1].reshape(-1)
    got = engine.resize_frames(flat[1:].view(1, 33, 47, 3), new_size=(7, 5))
    assert np.array_equal(got.cpu().numpy()[0], _pillow(33, 47, (7, 5), None)[1])


def test_argument_errors(lib_built):
    from deepgraphpose_amd import engine, _lib
    fr = _dev(_frames(48, 64))
    with pytest.raises(_lib.DgpError):
        engine.resize_frames(fr.float(), new_size=(24, 32))
    with pytest.raises(_lib.DgpError):
        engine.resize_frames(torch.zeros((2, 48, 64, 4), dtype=torch.uint8, device="cuda"), new_size=(24, 32))
    with pytest.raises(_lib.DgpError):
        engine.resize_frames(fr[0], new_size=(24, 32))
    with pytest.raises(_lib.DgpError):
        engine.resize_frames(fr.cpu(), new_size=(24, 32))
    with pytest.raises(ValueError):
        engine.resize_frames(fr, new_size=(24, 0))
    with pytest.raises(ValueError):
        engine.resize_frames(fr, crop_size=(10, 10, 10, 20))
    with pytest.raises(ValueError):
        engine.resize_frames(fr, new_size=(24, 32, 3))
    # a horizontal reduction whose row segment is beyond the kernel's LDS budget is refused before anything is launched
    wide = torch.zeros((1, 2, 4096, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DgpError, match="LDS"):
        engine.resize_frames(wide, new_size=(2, 16))
    assert engine.resize_frames(torch.zeros((0, 48, 64, 3), dtype=torch.uint8, device="cuda"), new_size=(24, 32)).shape == (0, 24, 32, 3)


def test_plan_cache_evicts_one_entry_and_stays_correct(lib_built):
    """more sizes than the cache holds: it stays bounded, drops its oldest entry only, and a dropped size is rebuilt to the same bytes"""
    from deepgraphpose_amd import engine
    fr = _dev(_frames(48, 64))
    first = engine.resize_frames(fr, new_size=(20, 30)).cpu().numpy()
    for i in range(17):
        engine.resize_frames(fr, new_size=(21 + i, 30))
    keys = list(engine._RESIZE_PLANS)
    assert len(keys) <= 16 and not any(k[3:] == (20, 30) for k in keys) and any(k[3:] == (22, 30) for k in keys)
    assert np.array_equal(engine.resize_frames(fr, new_size=(20, 30)).cpu().numpy(), first)


def _tiny_project(tmp_path, nj=3):
    """the project of test_boundary_gpu.py's _tiny_project: a config, a pose_cfg and a synthetic ResNet-50 snapshot"""
    import yaml
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.synthetic import make_weights
    parts = ["a", "b", "c"][:nj]
    proj = tmp_path / "proj"
    train = proj / "dlc-models" / "iteration-0" / "DemoOct2-trainset95shuffle1" / "train"
    train.mkdir(parents=True)
    (proj / "config.yaml").write_text(yaml.safe_dump(dict(Task="Demo", date="Oct2", iteration=0, TrainingFraction=[0.95],
                                                          bodyparts=parts, skeleton=[], project_path=str(proj))))
    (train / "pose_cfg.yaml").write_text(yaml.safe_dump(dict(num_joints=nj, all_joints_names=parts, net_type="resnet_50")))
    snap = weights_io.save_weights(str(train / "snapshot-step2-final--0"), make_weights(50, nj, False, seed=9, head_std=0.05))
    return proj, snap


def test_estimate_pose_hip_backend_equals_pil_backend(lib_built, tmp_path):
    """new_size = (72, 96) on 120 x 160 frames, T = 3 over batches of 2, then the same with crop_size: the frames the engines see are the
    same bytes whichever backend prepared them, so x, y and likelihoods are equal bit for bit"""
    from deepgraphpose_amd.models import eval as E
    from deepgraphpose_amd.synthetic import make_frames
    proj, snap = _tiny_project(tmp_path)
    np.save(tmp_path / "clip.npy", make_frames(3, 120, 160, 3, seed=43))

    def run(backend, tag, **kw):
        out = E.estimate_pose(str(proj / "config.yaml"), snap, str(tmp_path / "clip.npy"), str(tmp_path / ("pred_%s_%s" % (tag, backend))),
                              shuffle=1, batch_size=2, resize_backend=backend, **kw)
        return out, E.RUN_STATS["prep_backend"]

    for tag, kw in (("resized", dict(new_size=(72, 96))), ("cropped", dict(crop_size=(8, 16, 136, 112))),
                    ("both", dict(new_size=(72, 96), crop_size=(-4, -3, 92, 69)))):
        hip, ran_hip = run("hip", tag, **kw)
        pil, ran_pil = run("pil", tag, **kw)
        assert (ran_hip, ran_pil) == ("hip", "pil")
        for k in ("x", "y", "likelihoods"):
            assert hip[k].shape == (3, 3) and np.array_equal(hip[k], pil[k]), (tag, k)
    auto, ran = run("auto", "auto", new_size=(72, 96))
    assert ran == "hip" and all(np.array_equal(auto[k], hip_k) for k, hip_k in run("hip", "again", new_size=(72, 96))[0].items())
    out, ran = run("auto", "plain")
    assert ran == "none" and out["x"].shape == (3, 3)
    with pytest.raises(ValueError, match="resize_backend"):
        run("opencv", "bad", new_size=(72, 96))


def test_estimate_pose_auto_falls_back_to_pil_for_a_refused_shape(lib_built, tmp_path, capsys):
    """3072 -> 128 columns (24 x) is beyond the kernel's row buffers: "auto" says so in one line and gives what "pil" gives, "hip" raises"""
    from deepgraphpose_amd import _lib
    from deepgraphpose_amd.models import eval as E
    from deepgraphpose_amd.synthetic import make_frames
    proj, snap = _tiny_project(tmp_path)
    np.save(tmp_path / "wide.npy", make_frames(3, 32, 3072, 3, seed=44))

    def run(backend):
        out = E.estimate_pose(str(proj / "config.yaml"), snap, str(tmp_path / "wide.npy"), str(tmp_path / ("pred_" + backend)),
                              shuffle=1, batch_size=2, resize_backend=backend, new_size=(96, 128))
        return out, E.RUN_STATS["prep_backend"]

    capsys.readouterr()
    auto, ran = run("auto")
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("resize_backend auto:")]
    assert ran == "pil" and len(said) == 1 and "Pillow" in said[0] and "LDS" in said[0]
    pil, ran = run("pil")
    assert ran == "pil"
    for k in ("x", "y", "likelihoods"):
        assert auto[k].shape == (3, 3) and np.array_equal(auto[k], pil[k]), k
    with pytest.raises(_lib.DgpError, match="LDS"):
        run("hip")
