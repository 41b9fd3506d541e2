"""Frame sources.  Video DECODE is out of scope for every codec but one (the reference uses moviepy's VideoFileClip,
DGP/models/eval.py:256, and this path leaves it untouched): a real video is opened through moviepy
when it is installed; directories of images, .npy/.npz stacks and in-memory arrays are accepted so the
pipeline also runs where no decoder exists (e.g. the bundled demo project ships only labeled PNGs).
The one codec: Motion-JPEG in an .avi (MjpegAviSource; write_mjpeg_avi makes one), read here without moviepy -- its frames are
independent baseline JPEGs, which Pillow decodes on the host and csrc/dgp_jpeg.hip on the GPU, to the same bytes."""
from __future__ import annotations

import glob
import os
from typing import Iterator, Tuple

import numpy as np


class ArraySource:
    def __init__(self, frames: np.ndarray, fps: float = 30.0):
        assert frames.ndim == 4 and frames.shape[-1] == 3
        self.frames, self.fps = frames, fps
        self.n_frames = frames.shape[0]
        self.size = (frames.shape[2], frames.shape[1])          # (width, height) like VideoFileClip.size

    def iter_frames(self) -> Iterator[np.ndarray]:
        for f in self.frames:
            yield f

    def frame_at(self, i: int) -> np.ndarray:
        return self.frames[int(i)]

    def iter_batches(self, n: int) -> Iterator[np.ndarray]:
        """Contiguous runs of up to n frames (views): lets the staging thread fill a pinned batch with one copy."""
        for i in range(0, self.n_frames, n):
            yield self.frames[i:i + n]

    def close(self):
        pass


class ImageDirSource:
    def __init__(self, path: str, fps: float = 30.0):
        from PIL import Image
        self._Image = Image
        self.files = sorted(f for ext in ("png", "jpg", "jpeg", "bmp") for f in glob.glob(os.path.join(path, "*." + ext)))
        if not self.files:
            raise FileNotFoundError("no image frames in %s" % path)
        self.fps, self.n_frames = fps, len(self.files)
        with Image.open(self.files[0]) as im:
            self.size = im.size

    @property
    def jpeg_only(self) -> bool:
        """every frame is a .jpg / .jpeg file (jpeg_bytes never returns None)"""
        return all(f.lower().endswith((".jpg", ".jpeg")) for f in self.files)

    def _read(self, f):
        with self._Image.open(f) as im:
            return np.asarray(im.convert("RGB"))

    def frame_at(self, i: int) -> np.ndarray:
        return self._read(self.files[int(i)])

    def jpeg_bytes(self, i: int):
        """frame i's file as it is when it is a .jpg / .jpeg (for the HIP decoder; thread-safe), None for any other format"""
        f = self.files[int(i)]
        if not f.lower().endswith((".jpg", ".jpeg")):
            return None
        with open(f, "rb") as fh:
            return fh.read()

    def iter_frames(self):
        for f in self.files:
            yield self._read(f)

    def close(self):
        pass


class LabeledDirSource(ImageDirSource):
    """Pseudo-video from a DLC `labeled-data/<video>/` folder (img<NNN>.png = frame NNN of the video): n_frames = last
    labeled frame number + 1 and frame t shows the labeled image with the largest number <= t (the first one before that).
    Labeled frame NNN is therefore exactly img<NNN>.png, so the project's labels stay aligned.  Plumbing only -- the bundled
    Reaching demo project ships its 55 labeled PNGs but not its video (BASELINE configs[0])."""

    def __init__(self, path: str, fps: float = 30.0):
        super().__init__(path, fps)
        import re
        nums = []
        for f in self.files:
            m = re.match(r"img(\d+)\.", os.path.basename(f))
            if m:
                nums.append((int(m.group(1)), f))
        if not nums:
            raise FileNotFoundError("no img<NNN> frames in %s" % path)
        nums.sort()
        self.numbers = np.array([n for n, _ in nums])
        self.files = [f for _, f in nums]
        self.n_frames = int(self.numbers[-1]) + 1
        # a video has ONE frame size: the most common size of the labeled images (the Reaching project mixes 832 x 747 frames with
        # 640 x 470 crops); images of another size are resized to it
        from collections import Counter
        sizes = []
        for f in self.files:
            with self._Image.open(f) as im:
                sizes.append(im.size)
        self.size = Counter(sizes).most_common(1)[0][0]

    def _read(self, f):
        with self._Image.open(f) as im:
            im = im.convert("RGB")
            if im.size != self.size:
                im = im.resize(self.size, self._Image.BILINEAR)
            return np.asarray(im)

    jpeg_only = False                     # frames repeat and may be resized: always read through frame_at

    def jpeg_bytes(self, i: int):
        return None

    def _file_for(self, t: int) -> str:
        k = int(np.searchsorted(self.numbers, t, side="right")) - 1
        return self.files[max(k, 0)]

    def frame_at(self, i: int) -> np.ndarray:
        return self._read(self._file_for(int(i)))

    def iter_frames(self):
        last, img = None, None
        for t in range(self.n_frames):
            f = self._file_for(t)
            if f != last:
                img, last = self._read(f), f
            yield img


class MoviepySource:
    def __init__(self, path: str):
        from moviepy.editor import VideoFileClip           # third-party decode, untouched
        self.clip = VideoFileClip(str(path))
        self.fps = self.clip.fps
        self.n_frames = int(np.ceil(self.clip.fps * self.clip.duration))     # eval.py:257
        self.size = tuple(self.clip.size)

    def frame_at(self, i: int) -> np.ndarray:
        return np.asarray(self.clip.get_frame(int(i) * 1.0 / self.clip.fps))      # seek by time like DGP/dataset.py:811-821

    def iter_frames(self):
        return self.clip.iter_frames()

    def close(self):
        self.clip.close()


def _needs_moviepy(path, why="") -> ImportError:
    return ImportError("decoding %s needs moviepy%s (of video codecs only Motion-JPEG in an .avi is decoded by this package itself: "
                       "transcode once with `ffmpeg -c:v mjpeg`); or pass a directory of frames or a .npy stack instead"
                       % (path, " (%s)" % why if why else ""))


class MjpegAviSource:
    """A Motion-JPEG .avi read without any video library: a RIFF walk finds every frame's JPEG bytes, Pillow (frame_at) or the HIP
    decoder (jpeg_bytes -> engine.jpeg_decode / estimate_pose(decode_backend="hip")) turns them into pixels.  Every MJPEG frame is a key
    frame, so frames are read in any order and from any number of threads.

    Layout read: every RIFF segment of the file ('AVI ' and OpenDML's 'AVIX'), in each its 'movi' lists (and 'rec ' lists inside);
    the frame table is built from the chunk headers themselves -- 'idx1' is neither needed nor trusted (it covers the first segment
    only).  Chunks are word-aligned.  Only the first video stream counts (its '##dc' / '##db' chunks); a zero-length chunk repeats the
    previous frame (how AVI writers keep the rate over a dropped frame).  fps = dwRate / dwScale of the stream header, size and codec
    from its 'strf' (BITMAPINFOHEADER).  Another codec raises the ImportError open_frame_source raises for any video without moviepy."""

    def __init__(self, path: str):
        import struct
        from PIL import Image
        self._Image = Image
        self.path = str(path)
        self._fd = None
        table, streams = [], []                    # (offset, size) per frame; (fccType, scale, rate, strf bytes) per 'strl'
        with open(self.path, "rb") as f:
            end = os.fstat(f.fileno()).st_size

            def header(pos):
                f.seek(pos)
                h = f.read(12)
                return (h[:4], struct.unpack("<I", h[4:8])[0], h[8:12]) if len(h) >= 8 else (b"", 0, b"")

            def walk(pos, stop, want):
                """the chunks of [pos, stop): lists are entered, (id, offset of the data, size) is handed to want()"""
                while pos + 8 <= stop:
                    cid, size, form = header(pos)
                    if cid == b"LIST":
                        if form in (b"hdrl", b"strl", b"movi", b"rec "):
                            if form == b"strl":
                                streams.append([b"", 1, 30, b""])
                            walk(pos + 12, min(pos + 8 + size, stop), want)
                    elif len(cid) == 4:
                        want(cid, pos + 8, min(size, max(stop - pos - 8, 0)))
                    else:
                        return
                    pos += 8 + size + (size & 1)

            def want(cid, off, size):
                if cid == b"strh" and streams and size >= 32:
                    f.seek(off)
                    h = f.read(32)
                    streams[-1][0] = h[:4]
                    streams[-1][1], streams[-1][2] = struct.unpack("<II", h[20:28])
                elif cid == b"strf" and streams:
                    f.seek(off)
                    streams[-1][3] = f.read(min(size, 40))
                elif cid[2:] in (b"dc", b"db") and cid[:2] == b"%02d" % first_video():
                    table.append((off, size) if size else (table[-1] if table else (0, 0)))

            def first_video():                     # (the header list precedes every 'movi' list: the streams are known by then)
                return next((k for k, s in enumerate(streams) if s[0] == b"vids"), -1)

            pos = 0
            while pos + 12 <= end:
                cid, size, form = header(pos)
                if cid != b"RIFF" or form not in (b"AVI ", b"AVIX"):
                    break
                walk(pos + 12, min(pos + 8 + size, end), want)
                pos += 8 + size + (size & 1)
            if pos == 0:
                raise _needs_moviepy(self.path, "not a RIFF AVI file")
            video = first_video()
            if video < 0:
                raise _needs_moviepy(self.path, "no video stream in the AVI")
        _, scale, rate, strf = streams[video]
        if len(strf) < 20:
            raise _needs_moviepy(self.path, "no stream format in the AVI")
        width, height = struct.unpack("<ii", strf[4:12])
        fourcc = strf[16:20]
        if fourcc.upper() != b"MJPG":
            raise _needs_moviepy(self.path, "its codec is %r, not MJPG" % fourcc.decode("latin-1"))
        if not table:
            raise ValueError("no frames in %s" % self.path)
        self._table = table
        self.n_frames = len(table)
        self.fps = rate / scale if scale else 30.0
        self.size = (int(width), abs(int(height)))
        self._fd = os.open(self.path, os.O_RDONLY)

    def jpeg_bytes(self, i: int) -> bytes:
        """frame i's JPEG stream as stored (thread-safe: one positioned read, no shared file position)"""
        off, size = self._table[int(i)]
        if size == 0:
            raise ValueError("frame %d of %s is empty and no frame precedes it" % (int(i), self.path))
        b = os.pread(self._fd, size, off)
        if len(b) != size:
            raise ValueError("frame %d of %s is cut short" % (int(i), self.path))
        return b

    def frame_at(self, i: int) -> np.ndarray:
        import io
        with self._Image.open(io.BytesIO(self.jpeg_bytes(i))) as im:
            return np.asarray(im.convert("RGB"))

    def iter_frames(self):
        for i in range(self.n_frames):
            yield self.frame_at(i)

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _jpeg_size(data: bytes):
    """(width, height) from the frame header (SOFn) of a JPEG stream"""
    p, n = 2, len(data)
    while p + 4 <= n and data[p] == 0xFF:
        m, L = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) and p + 9 <= n:
            return ((data[p + 7] << 8) | data[p + 8], (data[p + 5] << 8) | data[p + 6])
        if m == 0xDA:
            break
        p += 2 + L
    raise ValueError("MjpegAviWriter: no frame header in the first JPEG stream (pass size=(width, height))")


class MjpegAviWriter:
    """The container half of a Motion-JPEG .avi: add(data) appends one frame's JPEG stream as a '00dc' chunk (None or b"": a zero-length
    chunk, which repeats the previous frame), close() patches the sizes and headers -- 'hdrl' (main header, one 'vids' / MJPG stream,
    an OpenDML 'dmlh' with the total), 'movi', 'idx1'.  No RIFF segment grows past segment_bytes (1 GiB: the OpenDML rule); further
    frames go to 'AVIX' segments.  index=False leaves 'idx1' out (readers of this package never need it).  size = (width, height); when
    it is not given it is read from the first stream's frame header.  Who encodes the frames is the caller's business: write_mjpeg_avi
    feeds it Pillow's streams, models/render.py's write_annotated_movie the HIP encoder's.  One thread at a time."""

    def __init__(self, path, fps: float = 30.0, index: bool = True, segment_bytes: int = 1 << 30, size=None):
        import struct
        self._struct = struct
        self.fps, self.index, self.segment_bytes, self.size = fps, index, segment_bytes, size
        self.n = 0
        self._f = f = open(path, "wb")
        f.write(b"RIFF\0\0\0\0AVI LIST\0\0\0\0hdrl")
        hdrl_size_at = 16
        f.write(b"avih" + struct.pack("<I", 56))
        self._avih_at = f.tell()
        f.write(b"\0" * 56)
        f.write(b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 40) + b"strl")
        f.write(b"strh" + struct.pack("<I", 56))
        self._strh_at = f.tell()
        f.write(b"\0" * 56)
        f.write(b"strf" + struct.pack("<I", 40))
        self._strf_at = f.tell()
        f.write(b"\0" * 40)
        f.write(b"LIST" + struct.pack("<I", 4 + 8 + 4) + b"odmldmlh" + struct.pack("<I", 4))
        self._dmlh_at = f.tell()
        f.write(b"\0" * 4)
        self._patch(hdrl_size_at, f.tell() - hdrl_size_at - 4)
        self._seg_start, self._first = 0, True
        f.write(b"LIST\0\0\0\0movi")
        self._movi_at = f.tell() - 4                # (of the 'movi' tag: idx1 offsets count from here)
        self._idx = []
        self._n_first = 0

    def _patch(self, pos, value):
        f = self._f
        here = f.tell()
        f.seek(pos)
        f.write(self._struct.pack("<I", value))
        f.seek(here)

    def _close_segment(self):
        f, struct = self._f, self._struct
        self._patch(self._movi_at - 4, f.tell() - self._movi_at)
        if self._first and self.index:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._idx)))
            for off, ln in self._idx:
                f.write(b"00dc" + struct.pack("<III", 0x10 if ln else 0, off, ln))
        self._patch(self._seg_start + 4, f.tell() - self._seg_start - 8)

    def add(self, data) -> None:
        f, struct = self._f, self._struct
        if f is None:
            raise ValueError("MjpegAviWriter: add after close")
        data = b"" if data is None else data
        if self.size is None and len(data):
            self.size = _jpeg_size(data)
        tail = 16 * (len(self._idx) + 1) + 8 if self._first and self.index else 0
        if f.tell() - self._seg_start + 8 + len(data) + 1 + tail > self.segment_bytes and f.tell() > self._movi_at + 4:
            self._close_segment()
            if self._first:
                self._n_first = self.n
            self._first = False
            self._seg_start = f.tell()
            f.write(b"RIFF\0\0\0\0AVIXLIST\0\0\0\0movi")
            self._movi_at = f.tell() - 4
        if self._first:
            self._idx.append((f.tell() - self._movi_at, len(data)))
        f.write(b"00dc" + struct.pack("<I", len(data)))
        f.write(data)
        if len(data) & 1:
            f.write(b"\0")
        self.n += 1

    def abort(self) -> None:
        """close the file as it is (after an error: the file is incomplete)"""
        if self._f is not None:
            self._f.close()
            self._f = None

    def close(self) -> int:
        """-> the number of frames written"""
        from fractions import Fraction
        f, struct = self._f, self._struct
        if f is None:
            return self.n
        try:
            if self.size is None:
                raise ValueError("write_mjpeg_avi: no frames")
            fr = Fraction(float(self.fps)).limit_denominator(1000000)
            n = self.n
            self._close_segment()
            if self._first:
                self._n_first = n
            w, h = self.size
            self._patch(self._avih_at, int(round(1e6 / float(self.fps))))
            f.seek(self._avih_at + 12)
            f.write(struct.pack("<IIIIIII", 0x10 if self.index else 0, self._n_first, 0, 1, 0, w, h))
            f.seek(self._strh_at)
            f.write(b"vidsMJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, fr.denominator, fr.numerator, 0, n, 0, 0xFFFFFFFF, 0) +
                    struct.pack("<hhhh", 0, 0, w, h))
            f.seek(self._strf_at)
            f.write(struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0))
            self._patch(self._dmlh_at, n)
        finally:
            self.abort()
        return self.n

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()


def write_mjpeg_avi(path, frames, fps: float = 30.0, quality: int = 90, subsampling="4:2:0", index: bool = True,
                    segment_bytes: int = 1 << 30) -> int:
    """Write frames (an iterable of uint8 [H, W, 3] RGB or [H, W] grey arrays of one size) as a Motion-JPEG .avi: every frame encoded by
    Pillow (quality, subsampling as Image.save takes them) and handed to MjpegAviWriter, which describes the container.  A .npy stack
    becomes a file about a tenth its size that MjpegAviSource (and any player) reads.  A frame given as None is written as a
    zero-length chunk: it repeats the previous frame.  -> the number of frames written."""
    import io
    from PIL import Image
    size = None
    with MjpegAviWriter(path, fps=fps, index=index, segment_bytes=segment_bytes) as w:
        for frame in frames:
            if frame is None:
                data = b""
            else:
                a = np.asarray(frame)
                if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
                    raise ValueError("write_mjpeg_avi: frame %d is %s %s, not uint8 [H, W, 3] or [H, W]" % (w.n, a.dtype, a.shape))
                if size is None:
                    size = w.size = (a.shape[1], a.shape[0])
                elif size != (a.shape[1], a.shape[0]):
                    raise ValueError("write_mjpeg_avi: frame %d is %d x %d, the first one %d x %d" % (w.n, a.shape[1], a.shape[0], size[0], size[1]))
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, "JPEG", quality=quality, **({"subsampling": subsampling} if a.ndim == 3 else {}))
                data = buf.getvalue()
            w.add(data)
        return w.close()


def open_frame_source(video_file):
    if isinstance(video_file, np.ndarray):
        return ArraySource(video_file)
    p = str(video_file)
    if os.path.isdir(p):
        return ImageDirSource(p)
    if p.endswith(".npy"):
        return ArraySource(np.load(p))
    if p.endswith(".npz"):
        z = np.load(p)
        return ArraySource(z[z.files[0]])
    if not os.path.exists(p):
        # <proj>/videos/<name>.avi missing but <proj>/labeled-data/<name>/ present: the labeled frames as a pseudo-video
        stem = os.path.basename(p).rsplit(".", 1)[0]
        cand = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(p))), "labeled-data", stem)
        if os.path.isdir(cand):
            print("video %s is missing: using the labeled frames in %s as a pseudo-video" % (p, cand), flush=True)
            return LabeledDirSource(cand)
        raise FileNotFoundError(p)
    try:
        return MoviepySource(p)
    except ImportError:
        return MjpegAviSource(p)                 # (anything but a Motion-JPEG .avi: the ImportError that names moviepy)
