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


def write_mjpeg_avi(path, frames, fps: float = 30.0, quality: int = 90, subsampling="4:2:0", index: bool = True,
                    segment_bytes: int = 1 << 30) -> int:
    """Write frames (an iterable of uint8 [H, W, 3] RGB or [H, W] grey arrays of one size) as a Motion-JPEG .avi: every frame encoded by
    Pillow (quality, subsampling as Image.save takes them) into a '00dc' chunk of a minimal AVI -- 'hdrl' (main header, one 'vids' / MJPG
    stream, an OpenDML 'dmlh' with the total), 'movi', 'idx1'.  A .npy stack becomes a file about a tenth its size that
    MjpegAviSource (and any player) reads.  A frame given as None is written as a zero-length chunk: it repeats the previous frame.
    No RIFF segment grows past segment_bytes (1 GiB: the OpenDML rule); further frames go to 'AVIX' segments.  index=False leaves
    'idx1' out (readers of this package never need it).  -> the number of frames written."""
    import io
    import struct
    from fractions import Fraction
    from PIL import Image
    fr = Fraction(float(fps)).limit_denominator(1000000)
    n = 0
    size = None
    with open(path, "wb") as f:
        def patch(pos, value):
            here = f.tell()
            f.seek(pos)
            f.write(struct.pack("<I", value))
            f.seek(here)

        f.write(b"RIFF\0\0\0\0AVI LIST\0\0\0\0hdrl")
        hdrl_size_at = 16
        f.write(b"avih" + struct.pack("<I", 56))
        avih_at = f.tell()
        f.write(b"\0" * 56)
        f.write(b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 40) + b"strl")
        f.write(b"strh" + struct.pack("<I", 56))
        strh_at = f.tell()
        f.write(b"\0" * 56)
        f.write(b"strf" + struct.pack("<I", 40))
        strf_at = f.tell()
        f.write(b"\0" * 40)
        f.write(b"LIST" + struct.pack("<I", 4 + 8 + 4) + b"odmldmlh" + struct.pack("<I", 4))
        dmlh_at = f.tell()
        f.write(b"\0" * 4)
        patch(hdrl_size_at, f.tell() - hdrl_size_at - 4)
        seg_start, first = 0, True
        f.write(b"LIST\0\0\0\0movi")
        movi_at = f.tell() - 4                      # (of the 'movi' tag: idx1 offsets count from here)
        idx = []
        n_first = 0

        def close_segment():
            patch(movi_at - 4, f.tell() - movi_at)
            if first and index:
                f.write(b"idx1" + struct.pack("<I", 16 * len(idx)))
                for off, ln in idx:
                    f.write(b"00dc" + struct.pack("<III", 0x10 if ln else 0, off, ln))
            patch(seg_start + 4, f.tell() - seg_start - 8)

        for frame in frames:
            if frame is None:
                data = b""
            else:
                a = np.asarray(frame)
                if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
                    raise ValueError("write_mjpeg_avi: frame %d is %s %s, not uint8 [H, W, 3] or [H, W]" % (n, a.dtype, a.shape))
                if size is None:
                    size = (a.shape[1], a.shape[0])
                elif size != (a.shape[1], a.shape[0]):
                    raise ValueError("write_mjpeg_avi: frame %d is %d x %d, the first one %d x %d" % (n, a.shape[1], a.shape[0], size[0], size[1]))
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, "JPEG", quality=quality, **({"subsampling": subsampling} if a.ndim == 3 else {}))
                data = buf.getvalue()
            tail = 16 * (len(idx) + 1) + 8 if first and index else 0
            if f.tell() - seg_start + 8 + len(data) + 1 + tail > segment_bytes and f.tell() > movi_at + 4:
                close_segment()
                if first:
                    n_first = n
                first = False
                seg_start = f.tell()
                f.write(b"RIFF\0\0\0\0AVIXLIST\0\0\0\0movi")
                movi_at = f.tell() - 4
            if first:
                idx.append((f.tell() - movi_at, len(data)))
            f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))
            n += 1
        if size is None:
            raise ValueError("write_mjpeg_avi: no frames")
        close_segment()
        if first:
            n_first = n
        w, h = size
        patch(avih_at, int(round(1e6 / float(fps))))
        f.seek(avih_at + 12)
        f.write(struct.pack("<IIIIIII", 0x10 if index else 0, n_first, 0, 1, 0, w, h))
        f.seek(strh_at)
        f.write(b"vidsMJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, fr.denominator, fr.numerator, 0, n, 0, 0xFFFFFFFF, 0) +
                struct.pack("<hhhh", 0, 0, w, h))
        f.seek(strf_at)
        f.write(struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0))
        patch(dmlh_at, n)
    return n


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
