"""HIP JPEG reconstruction (csrc/dgp_jpeg.hip, engine.jpeg_decode / jpeg_reconstruct) against Pillow itself, byte for byte, and
estimate_pose fed from it (decode_backend "hip" against "host" and against the .npy stack of the Pillow-decoded frames)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_jpeg_cpu import encoded, pillow  # noqa: E402

pytestmark = pytest.mark.gpu
# 1 x 1: a single partial MCU; 16 x 16: exactly one 4:2:0 MCU (every upsampling edge at once); 17 x 33: one sample into the next MCU on
# both axes; 61 x 83: odd sizes over several MCUs and more than one workgroup of 32 blocks; 480 x 640: a real frame
SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (61, 83), (480, 640)]
SUBS = [0, 1, 2, "L"]


@functools.lru_cache(maxsize=None)
def _want(h, w, sub, q=90, rst=0, seed=0):
    out = pillow(encoded(h, w, sub, q, rst, seed))
    out.setflags(write=False)
    return out


def _diff(got, want):
    return "%d bytes differ, max |d| %d" % ((got != want).sum(), np.abs(got.astype(int) - want).max())


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_jpeg_decode_is_pillow_byte_for_byte(lib_built, h, w):
    from deepgraphpose_amd import engine
    for sub in SUBS:
        got = engine.jpeg_decode([encoded(h, w, sub, 90)])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 3)
        got, want = got.cpu().numpy()[0], _want(h, w, sub)
        assert np.array_equal(got, want), (sub, _diff(got, want))


def test_batch_with_per_frame_tables_and_restart_intervals(lib_built):
    from deepgraphpose_amd import engine
    for sub in SUBS:
        streams = [encoded(61, 83, sub, q, seed=i) for i, q in enumerate((50, 90, 100))]
        got = engine.jpeg_decode(streams).cpu().numpy()
        want = np.stack([_want(61, 83, sub, q, seed=i) for i, q in enumerate((50, 90, 100))])
        assert np.array_equal(got, want), (sub, _diff(got, want))
        streams = [encoded(61, 83, sub, 90, rst, seed=i) for i, rst in enumerate((3, 1, 7))]
        got = engine.jpeg_decode(streams).cpu().numpy()
        want = np.stack([_want(61, 83, sub, 90, rst, seed=i) for i, rst in enumerate((3, 1, 7))])
        assert np.array_equal(got, want), ("restart", sub, _diff(got, want))


def test_out_view_is_written_in_place_and_runs_repeat(lib_built):
    """out = buf[1][:3] of a [2][4]-frame buffer: frames 4 .. 6 are written, every other byte keeps its value; a second call gives the
    same bytes; a frame of another geometry is a ValueError naming it"""
    from deepgraphpose_amd import engine
    h, w = 17, 33
    streams = [encoded(h, w, 2, 90, seed=i) for i in range(3)]
    buf = torch.full((2, 4, h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    out = engine.jpeg_decode(streams, out=buf[1][:3])
    assert out.data_ptr() == buf[1].data_ptr()
    got = buf.cpu().numpy()
    want = np.full((2, 4, h, w, 3), 0xA5, np.uint8)
    want[1, :3] = np.stack([_want(h, w, 2, seed=i) for i in range(3)])
    assert np.array_equal(got, want), _diff(got, want)
    # frames one slot apart inside a larger allocation: dst_frame_stride is the slot pitch
    wide = torch.full((3, 2, h, w, 3), 0x3C, dtype=torch.uint8, device="cuda")
    engine.jpeg_decode(streams, out=wide[:, 1])
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 1], want[1, :3]) and (got[:, 0] == 0x3C).all()
    a = engine.jpeg_decode(streams).cpu().numpy()
    b = engine.jpeg_decode(streams).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, want[1, :3])
    with pytest.raises(ValueError, match="frame 1 is 33 x 17 4:4:4"):
        engine.jpeg_decode([streams[0], encoded(h, w, 0, 90)])


# ------------------------------------------------------------------------ estimate_pose
T, HW, NJ, BATCH = 43, (96, 128), 3, 8


def _tiny_project(tmp_path, nj=NJ):
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


def _material(tmp_path):
    """43 frames as an MJPEG .avi, as the .npy stack of its Pillow-decoded frames, and as a directory of the same JPEG files"""
    from deepgraphpose_amd.frames import MjpegAviSource, write_mjpeg_avi
    from deepgraphpose_amd.synthetic import make_frames
    avi = str(tmp_path / "clip.avi")
    assert write_mjpeg_avi(avi, make_frames(T, HW[0], HW[1], NJ, seed=45), fps=30.0, quality=90, subsampling="4:2:0") == T
    src = MjpegAviSource(avi)
    np.save(tmp_path / "clip.npy", np.stack([src.frame_at(i) for i in range(T)]))
    d = tmp_path / "jpegs"
    d.mkdir()
    for i in range(T):
        (d / ("f%04d.jpg" % i)).write_bytes(src.jpeg_bytes(i))
    src.close()
    return avi, str(tmp_path / "clip.npy"), str(d)


def _run(proj, snap, tmp_path, video, tag, **kw):
    from deepgraphpose_amd.models import eval as E
    out = E.estimate_pose(str(proj / "config.yaml"), snap, video, str(tmp_path / ("pred_" + tag)), shuffle=1, batch_size=BATCH, **kw)
    return out, E.RUN_STATS["decode_backend"]


def _same(a, b):
    return all(a[k].shape == (T, NJ) and np.array_equal(a[k], b[k]) for k in ("x", "y", "likelihoods"))


def test_estimate_pose_hip_decode_equals_host_decode(lib_built, tmp_path):
    """43 frames over batches of 8 (a short last batch): the labels of decode_backend "hip" equal those of "host" and of the .npy stack of
    the Pillow-decoded frames bit for bit; the same JPEG files as a directory give the same labels; "auto" picks "hip" for both"""
    proj, snap = _tiny_project(tmp_path)
    avi, npy, jdir = _material(tmp_path)
    hip, ran = _run(proj, snap, tmp_path, avi, "hip", decode_backend="hip")
    assert ran == "hip"
    host, ran = _run(proj, snap, tmp_path, avi, "host", decode_backend="host")
    assert ran == "host" and _same(hip, host)
    stack, ran = _run(proj, snap, tmp_path, npy, "npy")
    assert ran == "host" and _same(hip, stack)
    dhip, ran = _run(proj, snap, tmp_path, jdir, "dir_hip", decode_backend="hip")
    assert ran == "hip" and _same(hip, dhip)
    auto, ran = _run(proj, snap, tmp_path, avi, "auto")
    assert ran == "hip" and _same(hip, auto)
    with pytest.raises(ValueError, match="decode_backend"):
        _run(proj, snap, tmp_path, avi, "bad", decode_backend="ffmpeg")
    with pytest.raises(ValueError, match="no JPEG streams"):
        _run(proj, snap, tmp_path, npy, "npy_hip", decode_backend="hip")


def test_estimate_pose_hip_decode_feeds_the_hip_resize(lib_built, tmp_path):
    """new_size with resize_backend "hip": reconstruct and resize share the copy stream; the labels equal the host decode's and the stack's"""
    from deepgraphpose_amd.models import eval as E
    proj, snap = _tiny_project(tmp_path)
    avi, npy, _ = _material(tmp_path)
    kw = dict(new_size=(72, 96), resize_backend="hip")
    hip, ran = _run(proj, snap, tmp_path, avi, "hip", decode_backend="hip", **kw)
    assert ran == "hip" and E.RUN_STATS["prep_backend"] == "hip"
    host, ran = _run(proj, snap, tmp_path, avi, "host", decode_backend="host", **kw)
    assert ran == "host" and _same(hip, host)
    stack, _ = _run(proj, snap, tmp_path, npy, "npy", **kw)
    assert _same(hip, stack)
    # a host resize stands between the decoder and the engines: "hip" cannot run, "auto" says so
    with pytest.raises(ValueError, match="resized with Pillow"):
        _run(proj, snap, tmp_path, avi, "pil_hip", decode_backend="hip", new_size=(72, 96), resize_backend="pil")


def test_a_png_among_the_jpegs_keeps_the_host_decoder(lib_built, tmp_path, capsys):
    from PIL import Image
    proj, snap = _tiny_project(tmp_path)
    avi, npy, jdir = _material(tmp_path)
    last = os.path.join(jdir, "f%04d.jpg" % (T - 1))
    Image.fromarray(pillow(open(last, "rb").read())).save(os.path.join(jdir, "f%04d.png" % (T - 1)))     # the same pixels, losslessly
    os.remove(last)
    capsys.readouterr()
    auto, ran = _run(proj, snap, tmp_path, jdir, "auto")
    said = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("decode_backend auto:")]
    assert ran == "host" and len(said) == 1 and "host" in said[0] and ".jpg" in said[0]
    stack, _ = _run(proj, snap, tmp_path, npy, "npy")
    assert _same(auto, stack)
    with pytest.raises(ValueError, match="not every frame"):
        _run(proj, snap, tmp_path, jdir, "hip", decode_backend="hip")
