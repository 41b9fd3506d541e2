"""The HIP JPEG forward (csrc/dgp_jpeg.hip: dgp_jpeg_forward_u8, engine.jpeg_forward / jpeg_encode) against Pillow itself: the
coefficients read out of Pillow's stream element for element, the coded bytes byte for byte, markers against the numpy overlay, and
the annotated movie (render.write_annotated_movie "hip" against "host", plot_dgp(movie_backend="hip")) read back by this package."""
import io
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _jpeg_enc_ref as E  # noqa: E402
from test_jpeg_enc_cpu import ALIGNED_SIZES, EDGE_SIZES, SAMPLINGS, picture, pillow_bytes, save  # noqa: E402

pytestmark = pytest.mark.gpu
# the edge sizes walk through every padding case (a partial block, a partial MCU with dummy blocks on the right, below and both, an even
# and an odd height under 4:2:0, widths past and short of the aligned 8-pixel read); 480 x 640 is a real frame over many workgroups
SIZES = EDGE_SIZES + ALIGNED_SIZES + [(480, 640)]
NAMES = {E.S444: "4:4:4", E.S422: "4:2:2", E.S420: "4:2:0"}


def pillow_coef(b):
    """the coefficients of a Pillow stream through the C-ABI's decoder (tests/test_jpeg_cpu.py holds it to the restatement)"""
    from deepgraphpose_amd import jpeg
    info = jpeg.probe(b)
    coef, qt = np.zeros((info.total_blocks, 64), np.int16), np.zeros((info.ncomp, 64), np.uint16)
    jpeg.entropy_decode(b, info, coef, qt)
    return coef


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_forward_and_encode_are_pillow_exactly(lib_built, h, w):
    from deepgraphpose_amd import engine
    kinds = ["noise"] if h * w > 10000 else ["noise", "smooth", "saturated"]
    frames = torch.from_numpy(np.stack([picture(h, w, k) for k in kinds])).cuda()
    for sampling in SAMPLINGS:
        for q in (50, 90, 100):
            coef = engine.jpeg_forward(frames, quality=q, subsampling=NAMES[sampling])
            assert coef.dtype == torch.int16 and coef.is_cuda and coef.shape[0] == len(kinds) and coef.shape[2] == 64
            coef = coef.cpu().numpy()
            streams = engine.jpeg_encode(frames, quality=q, subsampling=NAMES[sampling])
            for i, kind in enumerate(kinds):
                want = pillow_bytes(h, w, kind, sampling, q)
                pc = pillow_coef(want)
                assert coef[i].shape == pc.shape and np.array_equal(coef[i], pc), (sampling, q, kind, int((coef[i] != pc).sum()))
                assert streams[i] == want, (sampling, q, kind)


def test_strided_batch_is_read_in_place_and_runs_repeat(lib_built):
    """3 different frames one slot apart inside a larger buffer: the buffer keeps every byte, two runs give the same bits, and Pillow's"""
    from deepgraphpose_amd import engine
    for (h, w) in ((17, 23), (47, 52)):
        host = np.full((3, 2, h, w, 3), 0x3C, np.uint8)
        for i in range(3):
            host[i, 1] = picture(h, w, "noise", seed=i + 1)
        buf = torch.from_numpy(host).cuda()
        view = buf[:, 1]
        assert not view.is_contiguous()
        a = engine.jpeg_forward(view, quality=90, subsampling="4:2:0")
        b = engine.jpeg_forward(view, quality=90, subsampling="4:2:0", out=torch.empty_like(a))
        assert np.array_equal(buf.cpu().numpy(), host)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b)
        for i in range(3):
            assert np.array_equal(a[i], pillow_coef(save(host[i, 1], 90, E.S420))), i
        assert engine.jpeg_encode(view[1:2], 75, "4:2:2") == [save(host[1, 1], 75, E.S422)]
    assert tuple(engine.jpeg_forward(view[:0]).shape[:1]) == (0,)


def _marker_rows(h, w):
    """one table row per frame: overlap in both orders, squares partly outside each edge and corner, wholly outside (by one pixel and by
    2^30), a marker that is off, none at all"""
    far = 1 << 30
    rows = [
        [[4, 5, 10, 20, 30, 1], [5, 6, 40, 50, 60, 1], [h // 2, w // 2, 1, 2, 3, 0], [h - 1, w - 1, 250, 0, 128, 1]],
        [[5, 6, 40, 50, 60, 1], [4, 5, 10, 20, 30, 1], [0, 0, 9, 8, 7, 1], [-1, w, 200, 100, 0, 1]],
        [[-3, 5, 7, 8, 9, 1], [5, -3, 17, 18, 19, 1], [h + 2, 7, 27, 28, 29, 1], [7, w + 2, 37, 38, 39, 1]],
        [[-4, 5, 7, 8, 9, 1], [5, -4, 7, 8, 9, 1], [h + 3, 5, 7, 8, 9, 1], [5, w + 3, 7, 8, 9, 1]],
        [[-far, far, 7, 8, 9, 1], [far, -far, 7, 8, 9, 1], [h // 2, far, 7, 8, 9, 1], [-far, w // 2, 7, 8, 9, 1]],
        [[h // 2, w // 2, 255, 255, 255, 1], [h // 2, w // 2, 0, 0, 0, 1], [h // 2 + 1, w // 2 - 1, 0, 255, 0, 1], [1, 1, 5, 5, 5, 0]],
    ]
    return np.array(rows, np.int32)


@pytest.mark.parametrize("h,w", [(17, 23), (47, 52)], ids=lambda v: str(v))
def test_markers_equal_the_host_overlay(lib_built, h, w):
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.models.render import draw_markers_host
    table = _marker_rows(h, w)
    host = np.stack([picture(h, w, "noise", seed=i) for i in range(len(table))])
    frames = torch.from_numpy(host).cuda()
    for dotsize in (3, 0, 1):
        drawn = np.stack([draw_markers_host(host[i], table[i], dotsize) for i in range(len(table))])
        assert not np.array_equal(drawn[3], drawn[2]) and np.array_equal(drawn[3], host[3]) and np.array_equal(drawn[4], host[4])
        for sampling in SAMPLINGS:
            got = engine.jpeg_encode(frames, 90, NAMES[sampling], markers=table, dotsize=dotsize)
            again = engine.jpeg_encode(torch.from_numpy(drawn).cuda(), 90, NAMES[sampling])
            want = [save(d, 90, sampling) for d in drawn]
            bad = [i for i in range(len(table)) if got[i] != want[i]]
            assert got == again and not bad, (dotsize, sampling, bad)
        assert np.array_equal(frames.cpu().numpy(), host)            # the overlay lives in registers: the frames are as they were
    # a device table, and no markers at all
    got = engine.jpeg_encode(frames, 90, "4:2:0", markers=torch.from_numpy(table).cuda(), dotsize=3)
    assert got == [save(draw_markers_host(host[i], table[i], 3), 90, E.S420) for i in range(len(table))]
    assert engine.jpeg_encode(frames, 90, "4:2:0", markers=table[:, :0]) == engine.jpeg_encode(frames, 90, "4:2:0")


def test_refusals_name_their_reason(lib_built):
    from deepgraphpose_amd import _lib, engine
    frames = torch.from_numpy(np.stack([picture(17, 23, "noise")])).cuda()
    for sub in ("gray", "L", 3):
        with pytest.raises(ValueError, match="grey and other samplings are not written"):
            engine.jpeg_forward(frames, subsampling=sub)
    for q in (0, 101):
        with pytest.raises(_lib.DgpError, match="quality must be in 1..100"):
            engine.jpeg_forward(frames, quality=q)
    lib = _lib.load()
    assert lib.dgp_jpeg_forward_scratch_bytes(1, 17, 23, 0) == 0 and lib.dgp_jpeg_forward_scratch_bytes(1, 17, 23, 3) > 0
    assert lib.dgp_jpeg_forward_u8(None, 1, 17, 23, 17 * 23 * 3, 0, None, None, 0, 3, None, None, 0, None) != 0
    assert b"grey" in lib.dgp_last_error()
    with pytest.raises(_lib.DgpError, match="device uint8"):
        engine.jpeg_forward(frames.cpu())
    with pytest.raises(_lib.DgpError, match="markers must be int32 \\[1, n, 6\\]"):
        engine.jpeg_forward(frames, markers=np.zeros((2, 1, 6), np.int32))
    with pytest.raises(_lib.DgpError, match="dotsize"):
        engine.jpeg_forward(frames, dotsize=-1)
    with pytest.raises(_lib.DgpError, match="must not overlap"):
        engine.jpeg_forward(frames.expand(2, 17, 23, 3))


# ------------------------------------------------------------------------ the annotated movie
def _labels(nj, T, h, w, seed=2):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-4, w + 4, (nj, T)), rng.uniform(-4, h + 4, (nj, T))
    x[0, 1] = np.nan
    mask = rng.random((nj, T)) > 0.2
    return x, y, mask


def test_movie_hip_equals_host_on_an_array_and_on_an_avi(lib_built, tmp_path, monkeypatch):
    from deepgraphpose_amd.frames import MjpegAviSource, write_mjpeg_avi
    from deepgraphpose_amd.models import render
    frames = np.stack([picture(24, 40, "smooth") // 2 + picture(24, 40, "noise", seed=i) // 2 for i in range(5)])
    x, y, mask = _labels(3, 4, 24, 40)                                   # one column short: the last frame repeats the last column
    table = render.marker_table(x, y, mask, 2)
    avi = str(tmp_path / "src.avi")
    write_mjpeg_avi(avi, frames, fps=25.0, quality=95, subsampling="4:4:4")
    for tag, source, fps in (("array", frames, 30.0), ("avi", avi, 25.0)):
        hip, host = str(tmp_path / (tag + "_hip.avi")), str(tmp_path / (tag + "_host.avi"))
        assert render.write_annotated_movie(source, x, y, mask, hip, dotsize=2, quality=90, subsampling="4:2:0", backend="hip") == hip
        render.write_annotated_movie(source, x, y, mask, host, dotsize=2, quality=90, subsampling="4:2:0", backend="host")
        assert open(hip, "rb").read() == open(host, "rb").read(), tag
        back = MjpegAviSource(hip)
        assert (back.n_frames, back.fps, back.size) == (5, fps, (40, 24))
        if tag == "array":
            for i in range(5):
                assert back.jpeg_bytes(i) == save(render.draw_markers_host(frames[i], table[min(i, 3)], 2), 90, E.S420), i
        back.close()
    # more frames than one batch and one slot ring hold, a short last batch
    old = render.MOVIE_BATCH
    render.MOVIE_BATCH = 2
    try:
        many = np.concatenate([frames, frames[::-1], frames])[:13]
        xm, ym, mm = _labels(3, 13, 24, 40, seed=5)
        hip, host = str(tmp_path / "many_hip.avi"), str(tmp_path / "many_host.avi")
        render.write_annotated_movie(many, xm, ym, mm, hip, dotsize=1, quality=75, subsampling="4:2:2", backend="hip")
        render.write_annotated_movie(many, xm, ym, mm, host, dotsize=1, quality=75, subsampling="4:2:2", backend="host")
        assert open(hip, "rb").read() == open(host, "rb").read()
        # an error on the way ends the run with that error
        with pytest.raises(ValueError, match="frame 5 is"):
            render.write_annotated_movie(_OddSource(many), xm, ym, mm, str(tmp_path / "odd.avi"), backend="hip")
        # ... from a coding thread (the 8th frame's) and from the writer thread (at the 4th frame) alike, and nothing is left waiting
        import threading
        from deepgraphpose_amd import frames as F, jpeg
        real_encode, real_add, calls, lock = jpeg.entropy_encode, F.MjpegAviWriter.add, [], threading.Lock()

        def coder_down(coef, *a, **k):
            with lock:
                calls.append(0)
                mine = len(calls)
            if mine == 8:
                raise RuntimeError("coder down")
            return real_encode(coef, *a, **k)

        def disk_full(self, data):
            if self.n == 3:
                raise OSError("disk full")
            return real_add(self, data)

        monkeypatch.setattr(jpeg, "entropy_encode", coder_down)
        with pytest.raises(RuntimeError, match="coder down"):
            render.write_annotated_movie(many, xm, ym, mm, str(tmp_path / "down.avi"), backend="hip")
        monkeypatch.setattr(jpeg, "entropy_encode", real_encode)
        monkeypatch.setattr(F.MjpegAviWriter, "add", disk_full)
        with pytest.raises(OSError, match="disk full"):
            render.write_annotated_movie(many, xm, ym, mm, str(tmp_path / "full.avi"), backend="hip")
        monkeypatch.setattr(F.MjpegAviWriter, "add", real_add)
        assert not [t for t in threading.enumerate() if t.name == "dgp-movie-writer"]
        render.write_annotated_movie(many, xm, ym, mm, hip, dotsize=1, quality=75, subsampling="4:2:2", backend="hip")      # and the next run is whole
        assert open(hip, "rb").read() == open(host, "rb").read()
    finally:
        render.MOVIE_BATCH = old


class _OddSource:
    """an open source whose sixth frame has another size: two batches are under way when it turns up"""

    def __init__(self, frames):
        self.frames, self.fps, self.n_frames, self.size = frames, 30.0, len(frames), (frames.shape[2], frames.shape[1])

    def iter_frames(self):
        for i, f in enumerate(self.frames):
            yield f[:-1] if i == 5 else f


@pytest.fixture(scope="module")
def plotted(lib_built, tmp_path_factory):
    """a tiny project, an 11-frame 96 x 128 clip, its labels, and plot_dgp(movie_backend="hip") over them"""
    from test_jpeg_gpu import _tiny_project
    from deepgraphpose_amd.models import eval as Ev
    from deepgraphpose_amd.synthetic import make_frames
    tmp = tmp_path_factory.mktemp("plot")
    proj, snap = _tiny_project(tmp)
    frames = make_frames(11, 96, 128, 3, seed=45)
    np.save(tmp / "clip.npy", frames)
    out_dir = str(tmp / "pred")
    Ev.estimate_pose(str(proj / "config.yaml"), snap, str(tmp / "clip.npy"), out_dir, shuffle=1, batch_size=8)
    movie = Ev.plot_dgp(str(tmp / "clip.npy"), out_dir, proj_cfg_file=str(proj / "config.yaml"), dgp_model_file=snap, dotsize=4,
                        mask_threshold=0.0, movie_backend="hip", movie_quality=85)
    return dict(proj=proj, snap=snap, frames=frames, out_dir=out_dir, movie=movie, backend=Ev.RUN_STATS["movie_backend"], tmp=tmp)


def test_plot_dgp_writes_the_movie_on_the_gpu(plotted):
    from PIL import Image
    from deepgraphpose_amd.frames import MjpegAviSource
    from deepgraphpose_amd.models import eval as Ev
    from deepgraphpose_amd.models.render import draw_markers_host, marker_table
    assert plotted["movie"] == os.path.join(plotted["out_dir"], "clip_labeled.avi") and plotted["backend"] == "hip"
    labels = Ev.load_pose_from_dlc_to_dict(os.path.join(plotted["out_dir"], "clip_labeled.csv"))
    table = marker_table(labels["x"].T, labels["y"].T, labels["likelihoods"].T > 0.0, 4)
    assert table[:, :, 5].any()
    src = MjpegAviSource(plotted["movie"])
    assert src.n_frames == 11 and src.size == (128, 96)
    drawn = draw_markers_host(plotted["frames"][0], table[0], 4)
    assert not np.array_equal(drawn, plotted["frames"][0])
    want = save(drawn, 85, E.S420)
    assert src.jpeg_bytes(0) == want
    assert np.array_equal(src.frame_at(0), np.asarray(Image.open(io.BytesIO(want)).convert("RGB")))
    src.close()


def test_estimate_pose_reads_the_written_movie(plotted):
    from deepgraphpose_amd.models import eval as Ev
    out = Ev.estimate_pose(str(plotted["proj"] / "config.yaml"), plotted["snap"], plotted["movie"], str(plotted["tmp"] / "again"), shuffle=1,
                           batch_size=8, decode_backend="hip")
    assert Ev.RUN_STATS["decode_backend"] == "hip"
    assert all(out[k].shape == (11, 3) and np.isfinite(out[k]).all() for k in ("x", "y", "likelihoods"))
