"""Baseline JPEG on the host: the restatement (tests/_jpeg_ref.py) against Pillow byte for byte, the C-ABI's parser and entropy decoder
(dgp_jpeg_probe / dgp_jpeg_entropy_decode, host only) against the restatement coefficient for coefficient, refusals and malformed
streams, the Motion-JPEG AVI reader and writer, and a sanitizer build of the stand-alone decoder program."""
import functools
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _jpeg_ref as R  # noqa: E402

SIZES = [(1, 1), (7, 9), (16, 16), (33, 48), (61, 83)]
SUBS = [0, 1, 2, "L"]           # Pillow's subsampling 4:4:4 / 4:2:2 / 4:2:0, and a mode-L image
MAX_BLOCKS = 1 << 16            # a corrupted size field may ask for gigabytes of coefficients: such a probe result is not decoded


def image(h, w, gray=False, seed=0):
    """smooth gradients under noise: every frequency band carries something, DC differences of both signs"""
    from PIL import Image
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(yy * 5 + xx * 3) % 256, (xx * 7) % 256, (yy * 11 + xx) % 256], -1) * 0.6 + rng.random((h, w, 3)) * 255 * 0.4
    a = a.astype(np.uint8)
    return Image.fromarray(a[..., 0] if gray else a)


@functools.lru_cache(maxsize=None)
def encoded(h, w, sub, quality, restart=0, seed=0):
    kw = dict(quality=quality)
    if sub != "L":
        kw["subsampling"] = sub
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    image(h, w, sub == "L", seed).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow(b):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


def strip_dht(b):
    """the stream without its DHT segments (what a plain MJPEG frame looks like)"""
    out, p = bytearray(b[:2]), 2
    while b[p + 1] != 0xDA:
        L = (b[p + 2] << 8) | b[p + 3]
        if b[p + 1] != 0xC4:
            out += b[p:p + 2 + L]
        p += 2 + L
    return bytes(out + b[p:])


def c_decode(b):
    """(coef, qt, info) through the C-ABI, buffers sized from the probe"""
    from deepgraphpose_amd import jpeg
    info = jpeg.probe(b)
    if info.total_blocks > MAX_BLOCKS:
        return None, None, info
    coef = np.full((info.total_blocks, 64), 0x5555, np.int16)
    qt = np.zeros((info.ncomp, 64), np.uint16)
    jpeg.entropy_decode(b, info, coef, qt)
    return coef, qt, info


CASES = [(h, w, sub, q, 0) for (h, w) in SIZES for sub in SUBS for q in (50, 90, 100)] + [(h, w, sub, 90, 3) for (h, w) in SIZES for sub in SUBS]


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_restatement_is_pillow_byte_for_byte(h, w):
    for sub in SUBS:
        for q, rst in ((50, 0), (90, 0), (100, 0), (90, 3)):
            b = encoded(h, w, sub, q, rst)
            got, want = R.decode(b), pillow(b)
            assert got.shape == want.shape == (h, w, 3) and np.array_equal(got, want), (sub, q, rst, int((got != want).sum()))
        b = strip_dht(encoded(h, w, sub, 90))
        assert b.count(b"\xff\xc4") == 0 and np.array_equal(R.decode(b), pillow(b)), ("no DHT", sub)
        assert np.array_equal(pillow(b), pillow(encoded(h, w, sub, 90)))


@pytest.mark.parametrize("h,w", SIZES, ids=lambda v: str(v))
def test_c_entropy_decoder_equals_the_restatement(lib_built, h, w):
    for sub in SUBS:
        streams = [encoded(h, w, sub, q, rst) for q, rst in ((50, 0), (90, 0), (100, 0), (90, 3))] + [strip_dht(encoded(h, w, sub, 90))]
        for b in streams:
            coef, qt, info = c_decode(b)
            rc, rq, ri = R.entropy_decode(b)
            assert (info.width, info.height, info.ncomp, info.sampling) == (w, h, ri["ncomp"], ri["sampling"])
            assert (info.mcus_x, info.mcus_y, info.total_blocks) == (ri["mcus_x"], ri["mcus_y"], ri["total_blocks"])
            assert list(info.blocks)[:info.ncomp] == ri["blocks"] and info.restart_interval == ri["restart"] and info.scan_offset == ri["scan_offset"]
            assert np.array_equal(coef, rc) and np.array_equal(qt, rq), (sub, len(b))
    assert info.sampling == R.GRAY and info.ncomp == 1           # (the last one was the mode-L image)


def test_probe_names_what_it_refuses(lib_built):
    from PIL import Image
    from deepgraphpose_amd import _lib, jpeg
    b = io.BytesIO()
    image(33, 48).save(b, "JPEG", progressive=True)
    with pytest.raises(_lib.DgpError, match="progressive"):
        jpeg.probe(b.getvalue())
    with pytest.raises(R.JpegError):
        R.parse(b.getvalue())
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 4), np.uint8), "CMYK").save(b, "JPEG")
    with pytest.raises(_lib.DgpError, match="4 components"):
        jpeg.probe(b.getvalue())
    good = encoded(33, 48, 2, 90)
    sof = good.index(b"\xff\xc0")
    with pytest.raises(_lib.DgpError, match="sampling"):
        jpeg.probe(good[:sof + 11] + b"\x41" + good[sof + 12:])             # luma 4 x 1
    with pytest.raises(_lib.DgpError, match="precision"):
        jpeg.probe(good[:sof + 4] + b"\x0c" + good[sof + 5:])
    dqt = good.index(b"\xff\xdb")
    with pytest.raises(_lib.DgpError, match="16-bit"):
        jpeg.probe(good[:dqt + 4] + b"\x10" + good[dqt + 5:])
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"              # transform 0: the three components are RGB
    with pytest.raises(_lib.DgpError, match="Adobe"):
        jpeg.probe(good[:2] + adobe + good[2:])
    assert jpeg.probe(good[:2] + adobe[:-1] + b"\x01" + good[2:]).sampling == R.S420
    with pytest.raises(_lib.DgpError):
        jpeg.probe(b"")
    # the info must be the stream's own: the caller sized its buffers from it
    info = jpeg.probe(encoded(16, 16, 0, 90))
    with pytest.raises(_lib.DgpError, match="does not belong"):
        jpeg.entropy_decode(good, info, np.zeros((info.total_blocks, 64), np.int16), np.zeros((3, 64), np.uint16))
    with pytest.raises(_lib.DgpError, match="coef_out"):
        jpeg.entropy_decode(good, jpeg.probe(good), np.zeros((3, 64), np.int16), np.zeros((3, 64), np.uint16))


def _cuts(b, n=50, seed=5):
    """n seeded cut positions, every one before the EOI marker"""
    return sorted(int(v) for v in np.random.default_rng(seed).integers(0, len(b) - 2, n))


def _corruptions(b, n=200, seed=6):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p, v = int(rng.integers(2, len(b))), int(rng.integers(0, 256))
        out.append(b[:p] + bytes([v]) + b[p + 1:])
    return out


def test_truncated_streams_are_refused(lib_built):
    from deepgraphpose_amd import _lib
    for sub, rst in ((2, 0), (0, 3)):
        b = encoded(33, 48, sub, 90, rst)
        for cut in _cuts(b):
            with pytest.raises(_lib.DgpError):
                c_decode(b[:cut])
            with pytest.raises(R.JpegError):
                R.entropy_decode(b[:cut])


def test_corrupted_streams_return(lib_built):
    """a corrupted byte may leave a decodable stream: the call returns either way, and what it decodes is what the restatement decodes
    from the same bytes (or the restatement refuses them)"""
    from deepgraphpose_amd import _lib
    decoded = refused = 0
    for sub, rst in ((2, 0), (1, 3)):
        for bad in _corruptions(encoded(16, 24, sub, 50, rst), 200, seed=6 + rst):
            try:
                coef, qt, info = c_decode(bad)
            except _lib.DgpError:
                refused += 1
                continue
            if coef is None:
                continue
            decoded += 1
            try:
                rc, rq, _ = R.entropy_decode(bad)
            except R.JpegError:
                continue
            assert np.array_equal(coef, rc) and np.array_equal(qt, rq)
    assert decoded > 0 and refused > 0, (decoded, refused)


# ------------------------------------------------------------------------ the AVI container
def _clip(n=5, h=24, w=40):
    return [np.asarray(image(h, w, seed=i)) for i in range(n)]


def test_mjpeg_avi_round_trip(tmp_path):
    from PIL import Image
    from deepgraphpose_amd.frames import MjpegAviSource, open_frame_source, write_mjpeg_avi
    frames = _clip()
    path = str(tmp_path / "clip.avi")
    assert write_mjpeg_avi(path, frames, fps=25.0, quality=90, subsampling="4:2:0") == 5
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI " and b"idx1" in raw and int.from_bytes(raw[4:8], "little") == len(raw) - 8
    src = open_frame_source(path)                    # (moviepy is absent here: the new source)
    assert isinstance(src, MjpegAviSource)
    assert (src.n_frames, src.fps, src.size) == (5, 25.0, (40, 24))
    for i, fr in enumerate(frames):
        b = io.BytesIO()
        Image.fromarray(fr).save(b, "JPEG", quality=90, subsampling="4:2:0")
        assert src.jpeg_bytes(i) == b.getvalue()
        assert np.array_equal(src.frame_at(i), pillow(b.getvalue()))
    assert np.array_equal(np.stack(list(src.iter_frames())), np.stack([src.frame_at(i) for i in range(5)]))
    src.close()

    # without idx1, with another rate
    write_mjpeg_avi(str(tmp_path / "noidx.avi"), frames, fps=29.97, index=False)
    raw2 = open(tmp_path / "noidx.avi", "rb").read()
    assert b"idx1" not in raw2
    s2 = MjpegAviSource(str(tmp_path / "noidx.avi"))
    assert (s2.n_frames, s2.fps, s2.size) == (5, 29.97, (40, 24))
    assert all(s2.jpeg_bytes(i) == MjpegAviSource(path).jpeg_bytes(i) for i in range(5))

    # a zero-length chunk repeats the previous frame
    write_mjpeg_avi(str(tmp_path / "drop.avi"), [frames[0], None, frames[2], None], quality=90)
    s3 = MjpegAviSource(str(tmp_path / "drop.avi"))
    assert s3.n_frames == 4 and b"00dc\0\0\0\0" in open(tmp_path / "drop.avi", "rb").read()
    assert np.array_equal(s3.frame_at(1), s3.frame_at(0)) and np.array_equal(s3.frame_at(3), s3.frame_at(2))
    assert not np.array_equal(s3.frame_at(2), s3.frame_at(0))

    # forced into two RIFF segments (OpenDML): the frame table comes from the chunk headers of both
    three = sum(len(MjpegAviSource(path).jpeg_bytes(i)) for i in range(3))
    write_mjpeg_avi(str(tmp_path / "split.avi"), frames, fps=25.0, segment_bytes=600 + three)      # headers + index < 600: the 4th frame does not fit
    raw4 = open(tmp_path / "split.avi", "rb").read()
    assert raw4.count(b"RIFF") == 2 and b"AVIX" in raw4
    s4 = MjpegAviSource(str(tmp_path / "split.avi"))
    assert s4.n_frames == 5 and all(s4.jpeg_bytes(i) == MjpegAviSource(path).jpeg_bytes(i) for i in range(5))


def test_another_codec_needs_moviepy(tmp_path):
    from deepgraphpose_amd.frames import open_frame_source, write_mjpeg_avi
    path = str(tmp_path / "clip.avi")
    write_mjpeg_avi(path, _clip(2))
    raw = open(path, "rb").read()
    other = str(tmp_path / "h264.avi")
    open(other, "wb").write(raw.replace(b"MJPG", b"H264"))
    with pytest.raises(ImportError, match="moviepy.*Motion-JPEG"):
        open_frame_source(other)
    open(str(tmp_path / "lower.avi"), "wb").write(raw.replace(b"MJPG", b"mjpg"))
    assert open_frame_source(str(tmp_path / "lower.avi")).n_frames == 2
    open(str(tmp_path / "junk.mp4"), "wb").write(b"\0\0\0\x18ftypmp42" + b"\0" * 64)
    with pytest.raises(ImportError, match="moviepy.*Motion-JPEG"):
        open_frame_source(str(tmp_path / "junk.mp4"))


def test_image_dir_source_hands_out_jpeg_files(tmp_path):
    from deepgraphpose_amd.frames import ImageDirSource
    for i in range(2):
        open(tmp_path / ("f%02d.jpg" % i), "wb").write(encoded(24, 40, 2, 90, seed=i))
    src = ImageDirSource(str(tmp_path))
    assert src.jpeg_only and src.jpeg_bytes(1) == encoded(24, 40, 2, 90, seed=1)
    image(24, 40).save(tmp_path / "f02.png")
    src = ImageDirSource(str(tmp_path))
    assert not src.jpeg_only and src.jpeg_bytes(2) is None and src.jpeg_bytes(0) is not None


def test_stage_jpeg_fills_coefficient_slots(lib_built):
    """the staging producer on its own (no GPU): three threads, a short last batch, a frame of another geometry"""
    import threading
    from deepgraphpose_amd import jpeg
    from deepgraphpose_amd.models import staging

    class Src:
        def __init__(self, streams):
            self.streams = streams

        def jpeg_bytes(self, i):
            return self.streams[i]

    streams = [encoded(16, 24, 2, 90, seed=i) for i in range(7)]
    info0 = jpeg.probe(streams[0])
    ce, qe = info0.total_blocks * 64, info0.ncomp * 64
    ring = staging.StagingRing([(np.zeros((3, ce), np.int16), np.zeros((3, qe), np.uint16)) for _ in range(2)])
    ring.set_total(3)
    threads = [threading.Thread(target=staging.stage_jpeg, args=(ring, Src(streams), info0, 0, 7, 3, t, 3)) for t in range(3)]
    for th in threads:
        th.start()
    held = []
    for k in range(3):
        slot, nb = ring.get(k, lambda: ring.give_back(held.pop(0)))
        assert nb == (3, 3, 1)[k]
        for i in range(nb):
            rc, rq, _ = R.entropy_decode(streams[3 * k + i])
            assert np.array_equal(ring.bufs[slot][0][i], rc.ravel()) and np.array_equal(ring.bufs[slot][1][i], rq.ravel())
        held.append(slot)
    assert ring.get(3, None) is None
    for th in threads:
        th.join()
    ring = staging.StagingRing([(np.zeros((3, ce), np.int16), np.zeros((3, qe), np.uint16))])
    ring.set_total(1)
    staging.stage_jpeg(ring, Src(streams[:2] + [encoded(16, 24, 0, 90)]), info0, 0, 3, 3, 0, 1, "clip.avi")
    with pytest.raises(ValueError, match="frame 2 of clip.avi is 24 x 16 4:4:4"):
        ring.get(0, None)


def test_cabi_declares_the_jpeg_entry_points():
    from deepgraphpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dgp_hip.h")).read()
    for name in ("dgp_jpeg_probe", "dgp_jpeg_entropy_decode", "dgp_jpeg_scratch_bytes", "dgp_jpeg_reconstruct_u8"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
    from deepgraphpose_amd import build
    assert "dgp_jpeg.hip" in build.SOURCES and "dgp_jpeg_host.h" in build.HEADERS


def test_host_decoder_under_sanitizers(tmp_path):
    """tests/jpeg_host_main.cpp (its own main, csrc/dgp_jpeg_host.h included) built with ASan + UBSan by the system C++ compiler and run,
    in its own process, over the valid, truncated and corrupted streams of the tests above: exit status 0"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path / "jpeg_host_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(HERE, "jpeg_host_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.skip("the compiler cannot build with -fsanitize=address,undefined: " + r.stderr[-300:])
    d = tmp_path / "streams"
    d.mkdir()
    n = 0
    for (h, w, sub, q, rst) in CASES:
        open(d / ("ok%04d.jpg" % n), "wb").write(encoded(h, w, sub, q, rst))
        n += 1
    for sub in SUBS:
        open(d / ("nodht%04d.jpg" % n), "wb").write(strip_dht(encoded(33, 48, sub, 90)))
        n += 1
    for sub, rst in ((2, 0), (0, 3)):
        b = encoded(33, 48, sub, 90, rst)
        for cut in _cuts(b):
            open(d / ("cut%04d.jpg" % n), "wb").write(b[:cut])
            n += 1
    for sub, rst in ((2, 0), (1, 3)):
        for bad in _corruptions(encoded(16, 24, sub, 50, rst), 200, seed=6 + rst):
            open(d / ("bad%04d.jpg" % n), "wb").write(bad)
            n += 1
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    files, decoded = (int(v) for v in r.stdout.split()[0::2][:2])
    assert files == sum(os.path.getsize(d / f) > 0 for f in os.listdir(d)) and decoded >= len(CASES) + len(SUBS), r.stdout
