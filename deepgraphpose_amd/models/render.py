"""The annotated movie (DGP/models/eval.py:46-119 draws with matplotlib + moviepy): square dots over every frame, written as a video.

Two writers.  create_annotated_movie is the thin moviepy wrapper (an .mp4, when moviepy is installed).  write_annotated_movie needs no
video library: it writes a Motion-JPEG .avi whose frames are, byte for byte, what Pillow's save(quality=, subsampling=) writes for the
frame with its markers drawn.  backend "host" does exactly that (draw_markers_host + frames.write_mjpeg_avi, one thread); backend "hip"
draws the markers and computes the quantised DCT coefficients on the GPU (csrc/dgp_jpeg.hip: dgp_jpeg_forward_u8), Huffman-codes them
on ENCODE_THREADS host threads (csrc/dgp_jpeg_host.h) and hands the streams to frames.MjpegAviWriter in frame order.  Every decision
about a marker (rounding, colour, visibility) is made on the host, once, in marker_table: both backends draw from the same table."""
from __future__ import annotations

import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ENCODE_THREADS = 8          # host threads that Huffman-code coefficient slots (as staging's DECODE_THREADS on the way in)
MOVIE_BATCH = 32            # frames per forward call and per pinned coefficient slot
MOVIE_SLOTS = 3             # pinned coefficient slots: one being filled, one being coded, one in between
_COORD_LIMIT = 1 << 30      # marker coordinates are clamped here: far outside any frame, and row +- dotsize stays inside int32


def _palette(nj: int) -> np.ndarray:
    """the colours create_annotated_movie draws with: uint8 [nj, 3]"""
    return (np.stack([np.linspace(0, 255, nj), np.linspace(255, 0, nj), np.full(nj, 128)], 1)).astype(np.uint8)


def create_annotated_movie(video_file, x, y, mask_array=None, filename="movie.mp4", dotsize=3, colormap="jet"):
    from moviepy.editor import VideoFileClip
    clip = VideoFileClip(str(video_file))
    nj, T = x.shape
    if mask_array is None:
        mask_array = ~np.isnan(x)
    palette = _palette(nj)
    fps = clip.fps

    def draw(get_frame, t):
        img = get_frame(t).copy()
        i = min(int(round(t * fps)), T - 1)
        for j in range(nj):
            if mask_array[j, i]:
                r, c = int(round(y[j, i])), int(round(x[j, i]))
                img[max(r - dotsize, 0):r + dotsize + 1, max(c - dotsize, 0):c + dotsize + 1] = palette[j]
        return img

    clip.fl(draw).write_videofile(filename, fps=fps, codec="mpeg4", audio=False)
    clip.close()
    return filename


def _check_dotsize(dotsize) -> int:
    if isinstance(dotsize, bool) or not isinstance(dotsize, (int, np.integer)) or not 0 <= int(dotsize) <= 65535:
        raise ValueError("dotsize must be an integer in 0..65535, got %r" % (dotsize,))
    return int(dotsize)


def marker_table(x, y, mask=None, dotsize: int = 3) -> np.ndarray:
    """x, y: [nj, T] marker coordinates (column, row) in pixels, mask: bool [nj, T] or None (= every finite marker) -> int32 [T, nj, 6] =
    row, col, r, g, b, on: what both movie backends draw.  row = int(round(y)) and col = int(round(x)) as create_annotated_movie's draw
    computes them (halves to even), colours from its palette; a marker that is masked out or has a non-finite coordinate is off (and its
    coordinates 0).  Coordinates are clamped to +-2^30, which is outside any frame by more than any dotsize."""
    _check_dotsize(dotsize)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError("marker_table: x and y must both be [nj, T], got %s and %s" % (x.shape, y.shape))
    nj, T = x.shape
    on = np.isfinite(x) & np.isfinite(y)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != x.shape:
            raise ValueError("marker_table: mask must be [nj, T] = %s, got %s" % (x.shape, mask.shape))
        on &= mask.astype(bool)
    table = np.zeros((T, nj, 6), np.int32)
    table[:, :, 0] = np.clip(np.rint(np.where(on, y, 0.0)), -_COORD_LIMIT, _COORD_LIMIT).T
    table[:, :, 1] = np.clip(np.rint(np.where(on, x, 0.0)), -_COORD_LIMIT, _COORD_LIMIT).T
    table[:, :, 2:5] = _palette(nj)[None]
    table[:, :, 5] = on.T
    return table


def draw_markers_host(frame: np.ndarray, table_row: np.ndarray, dotsize: int = 3) -> np.ndarray:
    """The numpy statement of the kernel's overlay: a copy of frame (uint8 [H, W, 3]) in which every pixel inside [row - dotsize, row +
    dotsize] x [col - dotsize, col + dotsize] of a marker of table_row (int32 [nj, 6], one row of marker_table) that is on has that
    marker's colour; markers are painted in index order, so the highest index wins; squares are clipped to the frame and one wholly
    outside it paints nothing."""
    dotsize = _check_dotsize(dotsize)
    img = np.array(frame, copy=True)
    H, W = img.shape[:2]
    for row, col, r, g, b, on in np.asarray(table_row).reshape(-1, 6).tolist():
        if not on:
            continue
        r0, r1, c0, c1 = max(row - dotsize, 0), min(row + dotsize + 1, H), max(col - dotsize, 0), min(col + dotsize + 1, W)
        if r0 < r1 and c0 < c1:
            img[r0:r1, c0:c1] = (r & 255, g & 255, b & 255)
    return img


def _all_jpeg(src) -> bool:
    """the source hands out a JPEG stream for every frame (an MJPEG .avi, a directory of .jpg files)"""
    return hasattr(src, "jpeg_bytes") and getattr(src, "jpeg_only", True)


def _write_host(src, table, filename, dotsize, quality, subsampling) -> int:
    from ..frames import write_mjpeg_avi
    T = table.shape[0]
    drawn = (draw_markers_host(f, table[min(i, T - 1)], dotsize) for i, f in zip(range(src.n_frames), src.iter_frames()))
    return write_mjpeg_avi(filename, drawn, fps=src.fps, quality=quality, subsampling=subsampling)


def _write_hip(src, table, filename, dotsize, quality, subsampling) -> int:
    """Batches of MOVIE_BATCH frames: onto the device (engine.jpeg_decode of the source's own JPEG streams, else pinned upload), the
    forward with this batch's markers, the coefficients into a pinned slot -- all on one stream, batch k + 1 issued before batch k's
    copy is waited for -- then one task per frame on ENCODE_THREADS threads, and a writer thread that takes the streams in frame order.
    An error anywhere ends the run: tasks report through their futures, the writer stops at the first one it meets, this thread stops
    issuing, closes the file as it is and raises."""
    import torch
    from .. import engine, jpeg
    from ..frames import MjpegAviWriter
    if not torch.cuda.is_available():
        raise ValueError("write_annotated_movie: backend 'hip' needs a GPU, and none is visible (backend 'host' writes the same file)")
    sampling = jpeg.sampling_id(subsampling)
    qt = jpeg.quality_tables(quality)
    n, T = int(src.n_frames), table.shape[0]
    W, H = (int(v) for v in src.size)
    nblk, _ = engine.jpeg_block_count(H, W, sampling)
    bound = jpeg.encode_bound(H, W, sampling)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(dev)
    from_jpeg = _all_jpeg(src)
    slots = [torch.empty((MOVIE_BATCH, nblk * 64), dtype=torch.int16).pin_memory() for _ in range(MOVIE_SLOTS)]
    slot_np = [s.numpy() for s in slots]
    slot_futures = [[] for _ in range(MOVIE_SLOTS)]
    d_coef = torch.empty((MOVIE_BATCH, nblk, 64), dtype=torch.int16, device=dev)
    d_frames = torch.empty((MOVIE_BATCH, H, W, 3), dtype=torch.uint8, device=dev)
    pinned_in = None if from_jpeg else [torch.empty((MOVIE_BATCH, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
    in_events = [None, None]
    local = threading.local()

    def code(slot, i):
        buf = getattr(local, "buf", None)
        if buf is None:
            buf = local.buf = np.empty(bound, np.uint8)
        m = jpeg.entropy_encode(slot_np[slot][i], H, W, sampling, qt, buf)
        return buf[:m].tobytes()

    todo = queue.Queue()                    # futures in frame order; None ends the writer
    failed = []

    def write():
        try:
            while True:
                fut = todo.get()
                if fut is None:
                    return
                writer.add(fut.result())
        except BaseException as e:          # noqa: BLE001 -- handed to the caller's thread
            failed.append(e)

    frames_it = None if from_jpeg else src.iter_frames()
    writer = MjpegAviWriter(filename, fps=src.fps, size=(W, H))
    pool = ThreadPoolExecutor(ENCODE_THREADS)
    wthread = threading.Thread(target=write, name="dgp-movie-writer")
    wthread.start()
    pending = None                          # (slot, frames in it, the event after its copy)
    try:
        def finish(p):
            slot, nb, ev = p
            ev.synchronize()
            slot_futures[slot] = [pool.submit(code, slot, i) for i in range(nb)]
            for fut in slot_futures[slot]:
                todo.put(fut)

        for k, t0 in enumerate(range(0, n, MOVIE_BATCH)):
            if failed:
                break
            nb = min(MOVIE_BATCH, n - t0)
            slot = k % MOVIE_SLOTS
            for fut in slot_futures[slot]:  # the slot's last user has been coded
                fut.result()
            rows = np.minimum(np.arange(t0, t0 + nb), T - 1)
            with torch.cuda.stream(stream):
                if from_jpeg:
                    engine.jpeg_decode([src.jpeg_bytes(i) for i in range(t0, t0 + nb)], out=d_frames[:nb])
                else:
                    pin = pinned_in[k % 2]
                    if in_events[k % 2] is not None:
                        in_events[k % 2].synchronize()
                    host = pin.numpy()
                    for i in range(nb):
                        f = np.asarray(next(frames_it))
                        if f.dtype != np.uint8 or f.shape != (H, W, 3):
                            raise ValueError("write_annotated_movie: frame %d is %s %s, not uint8 %s" % (t0 + i, f.dtype, f.shape, (H, W, 3)))
                        host[i] = f
                    d_frames[:nb].copy_(pin[:nb], non_blocking=True)
                    in_events[k % 2] = torch.cuda.Event()
                    in_events[k % 2].record(stream)
                markers = torch.from_numpy(np.ascontiguousarray(table[rows])).to(dev)
                engine.jpeg_forward(d_frames[:nb], quality, subsampling, markers, dotsize, out=d_coef[:nb])
                slots[slot][:nb].copy_(d_coef[:nb].view(nb, nblk * 64), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
            if pending is not None:
                finish(pending)
            pending = (slot, nb, ev)
        if pending is not None and not failed:
            finish(pending)
        todo.put(None)
        wthread.join()
        if failed:
            raise failed[0]
        return writer.close()
    except BaseException:
        todo.put(None)
        wthread.join()
        writer.abort()
        raise
    finally:
        pool.shutdown(wait=True)
        stream.synchronize()


def write_annotated_movie(video_file, x, y, mask_array=None, filename="movie.avi", dotsize=3, quality=90, subsampling="4:2:0",
                          backend="hip") -> str:
    """The annotated movie of video_file (anything frames.open_frame_source takes, or an open source) as a Motion-JPEG .avi at the
    source's rate: frame i with the markers of column min(i, T - 1) of x, y ([nj, T]; mask_array bool [nj, T], None = the finite ones)
    drawn as squares of half-width dotsize, encoded at `quality` / `subsampling` as Pillow's save takes them.  backend "hip" (a GPU) and
    "host" (Pillow, the reference and the CPU fallback) write the same bytes.  -> filename."""
    from ..frames import open_frame_source
    if backend not in ("hip", "host"):
        raise ValueError("write_annotated_movie: backend must be 'hip' or 'host', got %r" % (backend,))
    dotsize = _check_dotsize(dotsize)
    table = marker_table(x, y, mask_array, dotsize)
    if table.shape[0] == 0:
        raise ValueError("write_annotated_movie: no marker columns (T = 0)")
    own = not hasattr(video_file, "iter_frames")
    src = open_frame_source(video_file) if own else video_file
    try:
        (_write_hip if backend == "hip" else _write_host)(src, table, str(filename), dotsize, quality, subsampling)
    finally:
        if own:
            src.close()
    return str(filename)
