"""The JPEG encoder on the host: the restatement (tests/_jpeg_enc_ref.py) against Pillow's save byte for byte, the C-ABI's quality
tables and entropy encoder (dgp_jpeg_quality_tables / dgp_jpeg_entropy_encode, host only) against both, the AVI writer, the marker
table and its numpy overlay, plot_dgp's movie_backend without a GPU, and a sanitizer build of the stand-alone encoder program."""
import functools
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _jpeg_enc_ref as E  # noqa: E402
import _jpeg_ref as R  # noqa: E402

EDGE_SIZES = [(1, 1), (7, 9), (8, 8), (17, 23), (9, 41), (30, 50), (33, 16), (25, 8), (47, 52)]
ALIGNED_SIZES = [(16, 16), (48, 64)]
SIZES = EDGE_SIZES + ALIGNED_SIZES
SAMPLINGS = [E.S444, E.S422, E.S420]
QUALITIES = [10, 50, 75, 90, 95, 100]
KINDS = ["noise", "smooth", "saturated"]


@functools.lru_cache(maxsize=None)
def picture(h, w, kind, seed=0):
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(yy * 5 + xx * 3) % 256, (xx * 7) % 256, (yy * 11 + xx) % 256], -1).astype(np.uint8)
    else:
        a = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pillow_bytes(h, w, kind, sampling, q, seed=0):
    return save(picture(h, w, kind, seed), q, sampling)


def save(a, q, sampling):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.asarray(a)).save(b, "JPEG", quality=q, subsampling=E.PILLOW_SUBSAMPLING[sampling])
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def ref_coef(h, w, kind, sampling, q):
    c = E.forward(picture(h, w, kind), sampling, E.quality_tables(q))
    c.setflags(write=False)
    return c


def c_encode(coef, h, w, sampling, qt, slack=8):
    from deepgraphpose_amd import jpeg
    out = np.full(jpeg.encode_bound(h, w, sampling) + slack, 0xA5, np.uint8)
    n = jpeg.entropy_encode(np.ascontiguousarray(coef), h, w, sampling, qt, out, cap=out.size - slack)
    assert (out[out.size - slack:] == 0xA5).all()
    return out[:n].tobytes()


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_restatement_is_pillow_byte_for_byte(h, w):
    for sampling in SAMPLINGS:
        for q in QUALITIES:
            for kind in KINDS:
                want = pillow_bytes(h, w, kind, sampling, q)
                coef = ref_coef(h, w, kind, sampling, q)
                pc, pq, info = R.entropy_decode(want)
                assert info["sampling"] == sampling and np.array_equal(pq[:2], E.quality_tables(q))
                assert coef.shape == pc.shape and np.array_equal(coef, pc), (sampling, q, kind, int((coef != pc).sum()))
                assert E.entropy_encode(coef, h, w, sampling, E.quality_tables(q)) == want, (sampling, q, kind)


def test_quality_tables_equal_pillows(lib_built):
    from PIL import Image
    from deepgraphpose_amd import _lib, jpeg
    for q in range(1, 101):
        t = Image.open(io.BytesIO(save(np.zeros((8, 8, 3), np.uint8), q, E.S444))).quantization
        want = np.stack([np.array(t[0]), np.array(t[1])]).astype(np.uint16)      # (Pillow hands them out in natural order)
        got = jpeg.quality_tables(q)
        assert got.dtype == np.uint16 and got.shape == (2, 64) and np.array_equal(got, want), q
        assert np.array_equal(E.quality_tables(q), want), q
    for bad in (0, 101, -1):
        with pytest.raises(_lib.DgpError, match="quality must be in 1..100"):
            jpeg.quality_tables(bad)


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_c_entropy_encoder_writes_pillows_bytes(lib_built, h, w):
    from deepgraphpose_amd import jpeg
    for sampling in SAMPLINGS:
        for q in QUALITIES:
            for kind in KINDS:
                got = c_encode(ref_coef(h, w, kind, sampling, q), h, w, sampling, jpeg.quality_tables(q))
                assert got == pillow_bytes(h, w, kind, sampling, q), (sampling, q, kind)


def test_decode_of_encode_is_the_identity(lib_built):
    """coefficients Pillow would never produce (every category, long zero runs, full blocks) survive the C encoder and both decoders"""
    from deepgraphpose_amd import jpeg
    rng = np.random.default_rng(3)
    qt = jpeg.quality_tables(100)                          # all ones: the decoder's |coefficient x table entry| limit is no obstacle
    for (h, w), sampling in (((17, 23), E.S420), ((9, 41), E.S422), ((16, 16), E.S444)):
        g = R.geometry(w, h, sampling)
        coef = np.zeros((g["total_blocks"], 64), np.int16)
        for blk in coef:
            k = int(rng.integers(0, 4))
            if k == 0:
                blk[:] = rng.integers(-1023, 1024, 64)
            elif k == 1:
                blk[rng.integers(1, 64, 3)] = rng.integers(-1023, 1024, 3)
            elif k == 2:
                blk[63] = (1, -1, 1023, -1023)[int(rng.integers(0, 4))]
        coef[:, 0] = np.clip(np.cumsum(rng.integers(-300, 301, len(coef))), -1023, 1023)
        b = c_encode(coef, h, w, sampling, qt)
        assert b == E.entropy_encode(coef, h, w, sampling, qt)
        back, bq, _ = R.entropy_decode(b)
        assert np.array_equal(back, coef) and np.array_equal(bq, qt[[0, 1, 1]])
        info = jpeg.probe(b)
        c2, q2 = np.zeros_like(coef), np.zeros((3, 64), np.uint16)
        jpeg.entropy_decode(b, info, c2, q2)
        assert np.array_equal(c2, coef)


def test_refusals_and_the_output_bound(lib_built):
    from deepgraphpose_amd import _lib, jpeg
    h, w, sampling, q = 17, 23, E.S420, 90
    coef, qt = np.ascontiguousarray(ref_coef(h, w, "noise", sampling, q)), jpeg.quality_tables(q)
    want = pillow_bytes(h, w, "noise", sampling, q)
    # a cap one byte short: refused, and nothing at or past the cap is written
    out = np.full(len(want) + 16, 0xA5, np.uint8)
    with pytest.raises(_lib.DgpError, match="output buffer is smaller"):
        jpeg.entropy_encode(coef, h, w, sampling, qt, out, cap=len(want) - 1)
    assert (out[len(want) - 1:] == 0xA5).all()
    assert jpeg.entropy_encode(coef, h, w, sampling, qt, out, cap=len(want)) == len(want) and out[:len(want)].tobytes() == want
    assert (out[len(want):] == 0xA5).all()
    with pytest.raises(_lib.DgpError, match="output buffer is smaller"):
        jpeg.entropy_encode(coef, h, w, sampling, qt, out, cap=100)                # inside the header
    # what no Huffman category codes
    bad = coef.copy()
    bad[1, 5] = 1024
    with pytest.raises(_lib.DgpError, match="category 10"):
        jpeg.entropy_encode(bad, h, w, sampling, qt, out)
    bad = coef.copy()
    bad[0, 0], bad[1, 0] = -1024, 1024
    with pytest.raises(_lib.DgpError, match="category 11"):
        jpeg.entropy_encode(bad, h, w, sampling, qt, out)
    # geometry and tables
    with pytest.raises(_lib.DgpError, match="grey"):
        jpeg.entropy_encode(coef, h, w, R.GRAY, qt, out)
    with pytest.raises(_lib.DgpError, match="1..65535"):
        jpeg.entropy_encode(coef, 0, w, sampling, qt, out)
    with pytest.raises(_lib.DgpError, match="elements"):
        jpeg.entropy_encode(coef[:-1], h, w, sampling, qt, out)
    zero = qt.copy()
    zero[1, 7] = 0
    with pytest.raises(_lib.DgpError, match="outside 1..255"):
        jpeg.entropy_encode(coef, h, w, sampling, zero, out)
    with pytest.raises(_lib.DgpError):
        jpeg.encode_bound(h, w, R.GRAY)
    for s in SAMPLINGS:                                   # the bound holds for the densest blocks there are
        g = R.geometry(w, h, s)
        dense = np.tile(np.where(np.arange(64) % 2, 1023, -1023).astype(np.int16), (g["total_blocks"], 1))
        dense[:, 0] = np.where(np.arange(len(dense)) % 2, 1023, -1023)
        big = np.zeros(jpeg.encode_bound(h, w, s), np.uint8)
        assert 0 < jpeg.entropy_encode(dense, h, w, s, jpeg.quality_tables(100), big) <= big.size
    for name, want_id in (("4:4:4", 1), ("4:2:2", 2), ("4:2:0", 3), (0, 1), (1, 2), (2, 3)):
        assert jpeg.sampling_id(name) == want_id
    for name in ("gray", "L", 3, -1, None, "4:1:1"):
        with pytest.raises(ValueError, match="grey and other samplings are not written"):
            jpeg.sampling_id(name)


def test_avi_writer_fed_pillows_streams_equals_write_mjpeg_avi(tmp_path):
    from deepgraphpose_amd.frames import MjpegAviSource, MjpegAviWriter, write_mjpeg_avi
    frames = [picture(24, 40, "smooth") // 2 + picture(24, 40, "noise", seed=i) // 2 for i in range(5)]
    for tag, kw in (("plain", {}), ("noidx", dict(index=False)), ("split", dict(segment_bytes=2500))):
        a, b = str(tmp_path / (tag + "_a.avi")), str(tmp_path / (tag + "_b.avi"))
        seq = frames[:2] + [None] + frames[2:]
        assert write_mjpeg_avi(a, seq, fps=25.0, quality=90, subsampling="4:2:0", **kw) == 6
        w = MjpegAviWriter(b, fps=25.0, **kw)               # (the size comes from the first stream's frame header)
        for f in seq:
            w.add(None if f is None else save(f, 90, E.S420))
        assert w.close() == 6 and w.close() == 6
        assert open(a, "rb").read() == open(b, "rb").read(), tag
        with pytest.raises(ValueError, match="after close"):
            w.add(b"")
    assert open(str(tmp_path / "split_a.avi"), "rb").read().count(b"RIFF") > 1
    src = MjpegAviSource(str(tmp_path / "split_b.avi"))
    assert src.n_frames == 6 and src.size == (40, 24) and src.jpeg_bytes(3) == save(frames[2], 90, E.S420)
    src.close()
    with pytest.raises(ValueError, match="no frames"):
        MjpegAviWriter(str(tmp_path / "empty.avi")).close()


def test_marker_table_and_host_overlay():
    from deepgraphpose_amd.models.render import _palette, create_annotated_movie, draw_markers_host, marker_table  # noqa: F401
    nj, T = 4, 3
    x = np.array([[5.0, 2.5, np.nan], [6.0, 3.5, 1.0], [-50.0, 1e12, 0.0], [22.0, np.inf, 4.4]])       # columns
    y = np.array([[4.0, 0.5, 1.0], [5.0, 1.5, np.nan], [3.0, 2.0, -1e12], [16.0, 2.0, 4.6]])           # rows
    mask = np.ones((nj, T), bool)
    mask[1, 0] = False
    tab = marker_table(x, y, mask, 2)
    assert tab.dtype == np.int32 and tab.shape == (T, nj, 6)
    pal = _palette(nj)
    assert np.array_equal(tab[:, :, 2:5], np.broadcast_to(pal[None], (T, nj, 3)))
    assert tab[:, :, 5].tolist() == [[1, 0, 1, 1], [1, 1, 1, 0], [0, 0, 1, 1]]                           # masked, NaN and inf are off
    assert tab[0, 0, :2].tolist() == [4, 5] and tab[1, 0, :2].tolist() == [0, 2] and tab[1, 1, :2].tolist() == [2, 4]   # halves to even
    assert tab[2, 3, :2].tolist() == [5, 4] and tab[1, 2, 1] == 1 << 30 and tab[2, 2, 0] == -(1 << 30)
    assert (tab[tab[:, :, 5] == 0][:, :2] == 0).all()
    assert np.array_equal(marker_table(x, y, None, 2)[:, :, 5], (np.isfinite(x) & np.isfinite(y)).T)
    with pytest.raises(ValueError, match="dotsize"):
        marker_table(x, y, mask, -1)
    with pytest.raises(ValueError, match="mask must be"):
        marker_table(x, y, mask[:2], 2)

    frame = picture(17, 23, "noise")
    # frame 0: marker 0 at (4, 5); marker 1 masked; marker 2 wholly outside on the left; marker 3 at (16, 22): the bottom-right corner
    got = draw_markers_host(frame, tab[0], 2)
    want = frame.copy()
    want[2:7, 3:8] = pal[0]
    want[14:17, 20:23] = pal[3]
    assert np.array_equal(got, want) and got is not frame and got.flags.writeable
    # overlap: the higher index wins where both cover; with the order swapped the other one does
    both = np.array([[4, 5, 10, 20, 30, 1], [5, 6, 40, 50, 60, 1]], np.int32)
    got = draw_markers_host(frame, both, 2)
    want = frame.copy()
    want[2:7, 3:8] = (10, 20, 30)
    want[3:8, 4:9] = (40, 50, 60)
    assert np.array_equal(got, want)
    assert not np.array_equal(draw_markers_host(frame, both[::-1], 2), want)
    # dotsize 0: one pixel; partly outside at the top-left: clipped, not wrapped to the far edge; a negative end paints nothing
    one = draw_markers_host(frame, np.array([[0, 0, 1, 2, 3, 1], [16, 22, 4, 5, 6, 1], [17, 5, 9, 9, 9, 1]], np.int32), 0)
    want = frame.copy()
    want[0, 0], want[16, 22] = (1, 2, 3), (4, 5, 6)
    assert np.array_equal(one, want)
    part = draw_markers_host(frame, np.array([[-1, -2, 7, 8, 9, 1]], np.int32), 3)
    want = frame.copy()
    want[0:3, 0:2] = (7, 8, 9)
    assert np.array_equal(part, want)
    for far in ([-4, 5], [5, -4], [20, 5], [5, 26], [-(1 << 30), 1 << 30]):
        assert np.array_equal(draw_markers_host(frame, np.array([far + [7, 8, 9, 1]], np.int32), 3), frame), far
    assert np.array_equal(draw_markers_host(frame, np.array([[-3, 5, 7, 8, 9, 1]], np.int32), 3)[0, 2:9], np.tile([7, 8, 9], (7, 1)))
    assert np.array_equal(draw_markers_host(frame, np.array([[4, 5, 7, 8, 9, 0]], np.int32), 3), frame)


def test_host_backend_writes_the_drawn_frames(tmp_path):
    """backend "host" on an array source: frame i of the file is Pillow's stream of draw_markers_host(frame i, table row min(i, T - 1))"""
    from deepgraphpose_amd.frames import MjpegAviSource
    from deepgraphpose_amd.models.render import draw_markers_host, marker_table, write_annotated_movie
    frames = np.stack([picture(24, 40, "noise", seed=i) for i in range(5)])
    x = np.array([[3.0, 10.0, 39.0], [20.0, np.nan, -1.0]])
    y = np.array([[3.0, 12.0, 23.0], [11.0, 5.0, 2.0]])
    out = write_annotated_movie(frames, x, y, None, str(tmp_path / "m.avi"), dotsize=2, quality=75, subsampling="4:2:2", backend="host")
    tab = marker_table(x, y, None, 2)
    src = MjpegAviSource(out)
    assert src.n_frames == 5 and src.fps == 30.0
    for i in range(5):
        assert src.jpeg_bytes(i) == save(draw_markers_host(frames[i], tab[min(i, 2)], 2), 75, E.S422), i
    src.close()
    with pytest.raises(ValueError, match="backend"):
        write_annotated_movie(frames, x, y, None, str(tmp_path / "n.avi"), backend="ffmpeg")


def test_plot_dgp_hip_movie_needs_a_gpu(tmp_path, monkeypatch):
    import torch
    from deepgraphpose_amd.models import eval as E_
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # (where there is one, tests/test_jpeg_enc_gpu.py runs 'hip')
    with pytest.raises(ValueError, match="movie_backend 'hip' needs a GPU"):
        E_.plot_dgp(str(tmp_path / "clip.avi"), str(tmp_path), proj_cfg_file=str(tmp_path / "config.yaml"), movie_backend="hip")
    with pytest.raises(ValueError, match="movie_backend must be"):
        E_.plot_dgp(str(tmp_path / "clip.avi"), str(tmp_path), movie_backend="ffmpeg")
    from deepgraphpose_amd.models.render import write_annotated_movie
    with pytest.raises(ValueError, match="backend 'hip' needs a GPU"):
        write_annotated_movie(np.zeros((1, 8, 8, 3), np.uint8), np.zeros((1, 1)), np.zeros((1, 1)), None, str(tmp_path / "m.avi"), backend="hip")


def test_cabi_declares_the_encoder_entry_points():
    from deepgraphpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dgp_hip.h")).read()
    for name in ("dgp_jpeg_quality_tables", "dgp_jpeg_encode_bound", "dgp_jpeg_entropy_encode", "dgp_jpeg_forward_scratch_bytes",
                 "dgp_jpeg_forward_u8"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
    from deepgraphpose_amd import jpeg
    for name in ("quality_tables", "encode_bound", "entropy_encode", "sampling_id"):
        assert callable(getattr(jpeg, name))
    src = open(os.path.join(ROOT, "deepgraphpose_amd", "jpeg.py")).read()
    assert "import torch" not in src


def test_host_encoder_under_sanitizers(tmp_path):
    """tests/jpeg_enc_host_main.cpp (its own main, csrc/dgp_jpeg_host.h included) built with ASan + UBSan by the system C++ compiler and
    run, in its own process, over coefficient files: the restatement's, extreme ones, ones no category codes, wrong lengths and bad
    geometries.  Exit status 0: every stream fitted its bound, an exact cap was enough and one byte less refused, the decoder gave the
    coefficients back, and the sanitizers found nothing"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path / "jpeg_enc_host_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(HERE, "jpeg_enc_host_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.skip("the compiler cannot build with -fsanitize=address,undefined: " + r.stderr[-300:])
    d = tmp_path / "coef"
    d.mkdir()
    n = good = 0

    def put(h, w, sampling, q, coef):
        nonlocal n
        open(d / ("c%04d.bin" % n), "wb").write(struct.pack("<iiii", h, w, sampling, q) + np.ascontiguousarray(coef, np.int16).tobytes())
        n += 1

    rng = np.random.default_rng(8)
    for (h, w) in SIZES:
        for sampling in SAMPLINGS:
            for q, kind in ((10, "smooth"), (90, "noise"), (100, "saturated")):
                put(h, w, sampling, q, ref_coef(h, w, kind, sampling, q))
                good += 1
            blocks = R.geometry(w, h, sampling)["total_blocks"]
            dense = rng.integers(-1023, 1024, (blocks, 64))
            dense[:, 0] = rng.integers(-1023, 1024, blocks)
            put(h, w, sampling, 100, dense)                          # every coefficient set: the bound's worst case
            good += 1
            put(h, w, sampling, 50, rng.integers(-32768, 32768, (blocks, 64)))       # no category codes these: refused
            put(h, w, sampling, 90, np.zeros((blocks + 1, 64)))                      # a wrong length: skipped
    put(17, 23, R.GRAY, 90, np.zeros((6, 64)))
    put(0, 23, E.S420, 90, np.zeros((6, 64)))
    put(17, 70000, E.S444, 90, np.zeros((6, 64)))
    put(17, 23, 7, 90, np.zeros((6, 64)))
    put(17, 23, E.S420, 0, np.zeros((12, 64)))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    files, encoded, wrong = (int(v) for v in r.stdout.split()[0::2][:3])
    assert files == n and encoded == good and wrong == 0, r.stdout
