"""Which frames to label: k-means selection before the fit, outlier frames after it.

  kmeans_select, uniform_select      deeplabcut/utils/frameselectiontools.py:139-246 (KmeansbasedFrameselectioncv2), :45-69 (UniformFramescv2)
  extract_frames                     deeplabcut/generate_training_dataset/frame_extraction.py as DGP/utils_data.py:52-71 (local_extract_frames) drives it
  outlier_indices                    deeplabcut/refine_training_dataset/outlier_frames.py:136-174 ("jump", "uncertain")
  extract_outlier_frames             outlier_frames.py:119-193 + ExtractFramesbasedonPreselection, :293-396

The reference reads the video with cv2 or moviepy; this package reads it through frames.open_frame_source (Motion-JPEG decoded on the
device) and does the hot path -- every candidate frame shrunk to a thumbnail, the thumbnails clustered -- in csrc/dgp_select.hip.

Departures from the reference, all deliberate:
  * thumbnails are exact AREA AVERAGES over boxes (integer sums, one division).  The cv2 variant point-samples (INTER_NEAREST), the moviepy
    variant resamples with a filter; neither library exists on the ROCm images this package targets, so parity with either was never
    measured.  The frames are on the device already: the full average costs one read of bytes that were uploaded anyway and does not alias.
  * the clustering is Lloyd's algorithm with a k-means++ start drawn on the host (kmeans_host / kmeans_hip: one algorithm, two executors,
    the same bits), not MiniBatchKMeans -- unless backend="sklearn", which calls MiniBatchKMeans as the reference does.
  * config.yaml is never rewritten (the reference's add_new_videos); a line naming the video to add is printed instead.
  * not built: the labeled preview plots (savelabeled), the GUIs, refine_labels, merge_datasets, the "fitting" (statsmodels) and "manual" methods.

This module imports numpy only; torch and the HIP library are loaded by the "hip" backend alone.
"""
from __future__ import annotations

import os
import time
from pathlib import Path
from typing import Optional

import numpy as np

# ---- limits and fixed orders of csrc/dgp_select.hip (include/dgp_hip.h states them; tests compare the two executors bit for bit)
KMEANS_MAX_K, KMEANS_MAX_D, KMEANS_MAX_SLABS = 160, 8192, 64        # DGP_KMEANS_MAX_K, _MAX_D, _MAX_SLABS
FEATURES_MAX_WINDOW, FEATURES_MAX_WIDTH = 16384, 1024               # the widest window and thumbnail dgp_frame_features_u8 takes
FEATURES_MAX_BOX = 0xFFFFFFFF // 765                                # pixels of a box whose all-255 sum over three channels fits 32 bits
FEATURE_BYTES = 4 << 30       # the largest feature matrix kmeans_select builds (a choice, not a measurement)
DECODE_THREADS = 8            # host threads that Huffman-decode a chunk's JPEG frames (as models/eval.py's)

SELECT_STATS: dict = {}       # of the last kmeans_select: backend, frames_read, candidates, iterations, seconds per stage


# =====================================================================================================
# thumbnails
# =====================================================================================================
def feature_geometry(H: int, W: int, resizewidth: int = 30, color: bool = False, crop=None):
    """(x1, x2, y1, y2, oh, ow, D) of the thumbnails of H x W frames: crop = (x1, x2, y1, y2) selects frame[y1:y2, x1:x2]
    (frameselectiontools.py:181), ow = resizewidth, oh = max(1, Hc ow / Wc rounded half to even), D = oh ow (x 3 with color).  Every
    refusal of the kernel's host code is raised here first, as a ValueError that names the limit."""
    x1, x2, y1, y2 = (0, int(W), 0, int(H)) if crop is None else (int(v) for v in crop)
    if not (0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H):
        raise ValueError("frame features: crop (x1, x2, y1, y2) = %r is empty or leaves the %d x %d frame" % ((x1, x2, y1, y2), W, H))
    Wc, Hc, ow = x2 - x1, y2 - y1, int(resizewidth)
    if ow < 1:
        raise ValueError("frame features: resizewidth must be positive, not %d" % ow)
    if ow > Wc:
        raise ValueError("frame features: resizewidth %d actually upsamples a window %d pixels wide" % (ow, Wc))
    if Wc > FEATURES_MAX_WINDOW or ow > FEATURES_MAX_WIDTH:
        raise ValueError("frame features: a window %d wide reduced to %d is outside the limits (window <= %d, resizewidth <= %d)"
                         % (Wc, ow, FEATURES_MAX_WINDOW, FEATURES_MAX_WIDTH))
    q, rem = divmod(Hc * ow, Wc)
    oh = max(1, q + 1 if 2 * rem > Wc or (2 * rem == Wc and q & 1) else q)
    box = -(-Wc // ow) * -(-Hc // oh)
    if box > FEATURES_MAX_BOX:
        raise ValueError("frame features: a box of %d pixels could overflow its 32-bit sum (limit %d pixels)" % (box, FEATURES_MAX_BOX))
    return x1, x2, y1, y2, oh, ow, oh * ow * (3 if color else 1)


def box_edges(n: int, o: int) -> np.ndarray:
    """the o + 1 edges of o boxes over n pixels: box i is [floor(i n / o), floor((i + 1) n / o))"""
    return (np.arange(o + 1, dtype=np.int64) * n) // o


def features_host(frames, resizewidth: int = 30, color: bool = False, crop=None) -> np.ndarray:
    """The numpy statement of dgp_frame_features_u8: uint8 frames [N, H, W, 3] -> float32 [N, D].  int64 sums over the same boxes,
    float32(float64(sum) / count): the kernel's bits."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError("features_host: frames must be uint8 [N, H, W, 3], got %s %s" % (frames.dtype, frames.shape))
    N, H, W = frames.shape[:3]
    x1, x2, y1, y2, oh, ow, D = feature_geometry(H, W, resizewidth, color, crop)
    ye, xe = box_edges(y2 - y1, oh), box_edges(x2 - x1, ow)
    count = (np.diff(ye)[:, None] * np.diff(xe)[None, :]).astype(np.float64)            # pixels of box (r, i)
    out = np.empty((N, D), np.float32)
    for f0 in range(0, N, 64):
        win = frames[f0:f0 + 64, y1:y2, x1:x2]
        s = np.add.reduceat(win, ye[:-1], axis=1, dtype=np.int64)
        s = np.add.reduceat(s, xe[:-1], axis=2)                                          # [n, oh, ow, 3]
        if color:
            v = s.transpose(0, 1, 3, 2).astype(np.float64) / count[None, :, None, :]     # [n, oh, 3, ow]
        else:
            v = s.sum(axis=3).astype(np.float64) / (count * 3.0)[None]
        out[f0:f0 + 64] = v.astype(np.float32).reshape(len(win), D)
    return out


# =====================================================================================================
# k-means: one algorithm (k-means++ start drawn on the host, Lloyd iterations), two executors
# =====================================================================================================
def kmeans_slabs(N: int):
    """(S, rows per slab) of the double sums: S = min(64, ceil(N / 256)) slabs of ceil(N / S) rows"""
    S = max(1, min(KMEANS_MAX_SLABS, -(-N // 256)))
    return S, -(-N // S)


def kmeans_chunk(k: int) -> int:
    """columns per chunk of the distance sums: what fits 40 KB of LDS beside k centres, a multiple of 64, at most 512"""
    return min(512, 10240 // k // 64 * 64)


_LANE = np.arange(64)


def assign_host(X: np.ndarray, C: np.ndarray):
    """dgp_kmeans_assign restated: (labels int32 [N], dist float32 [N]).  fp32 throughout, in the kernel's order: per chunk of DC columns
    lane l adds its columns l, l + 64, ... in turn, a butterfly over the 64 lanes, chunk totals added in chunk order."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    (N, D), k = X.shape, C.shape[0]
    DC = kmeans_chunk(k)
    per_lane = DC // 64
    labels, dist = np.empty(N, np.int32), np.empty(N, np.float32)
    rows = max(1, (16 << 20) // (k * DC))
    for r0 in range(0, N, rows):
        xb = X[r0:r0 + rows]
        acc = np.zeros((len(xb), k), np.float32)
        for d0 in range(0, D, DC):
            w = min(DC, D - d0)
            xc = np.zeros((len(xb), DC), np.float32)
            cc = np.zeros((k, DC), np.float32)
            xc[:, :w], cc[:, :w] = xb[:, d0:d0 + w], C[:, d0:d0 + w]
            diff = xc[:, None, :] - cc[None, :, :]
            sq = (diff * diff).reshape(len(xb), k, per_lane, 64)
            part = sq[:, :, 0, :]
            for j in range(1, per_lane):
                part = part + sq[:, :, j, :]
            for o in (32, 16, 8, 4, 2, 1):
                part = part + part[:, :, _LANE ^ o]
            acc = acc + part[:, :, 0]
        lab = np.argmin(acc, axis=1)                  # the first minimum: the lowest index wins a tie
        labels[r0:r0 + rows] = lab
        dist[r0:r0 + rows] = acc[np.arange(len(xb)), lab]
    return labels, dist


def _slab_sums(X: np.ndarray, rows: np.ndarray, S: int, per: int) -> np.ndarray:
    """double column sums of X[rows] (ascending row numbers): one accumulator per slab walked in row order, slabs added in slab order"""
    total = np.zeros(X.shape[1], np.float64)
    for s in range(S):
        m = rows[(rows >= s * per) & (rows < (s + 1) * per)]
        part = np.add.accumulate(X[m].astype(np.float64), axis=0)[-1] if len(m) else np.zeros(X.shape[1], np.float64)
        total = total + part
    return total


def center_host(X: np.ndarray):
    """dgp_kmeans_center restated: (X - mean32 in float32, mean32)"""
    X = np.asarray(X, np.float32)
    S, per = kmeans_slabs(len(X))
    mean = (_slab_sums(X, np.arange(len(X)), S, per) / float(len(X))).astype(np.float32)
    return X - mean[None, :], mean


def update_host(X: np.ndarray, labels: np.ndarray, C: np.ndarray):
    """dgp_kmeans_update restated: (new centres float32 [k, D], counts int32 [k + 1])"""
    X, C = np.asarray(X, np.float32), np.array(C, np.float32)
    k = len(C)
    S, per = kmeans_slabs(len(X))
    counts = np.zeros(k + 1, np.int32)
    counts[k] = int(((labels < 0) | (labels >= k)).sum())
    for c in range(k):
        m = np.nonzero(labels == c)[0]
        counts[c] = len(m)
        if len(m):
            C[c] = (_slab_sums(X, m, S, per) / float(len(m))).astype(np.float32)
    return C, counts


class _HostExecutor:
    name = "host"

    def __init__(self, X):
        self.X = np.ascontiguousarray(X, np.float32)
        self.labels = np.full(len(self.X), -1, np.int32)
        self.C = None

    def dist_to_row(self, i: int) -> np.ndarray:
        return assign_host(self.X, self.X[i:i + 1])[1]

    def start(self, rows):
        self.C = self.X[np.asarray(rows)].copy()

    def assign(self) -> int:
        new, _ = assign_host(self.X, self.C)
        changed = int((new != self.labels).sum())
        self.labels = new
        return changed

    def update(self):
        self.C, counts = update_host(self.X, self.labels, self.C)
        if counts[-1]:
            raise ValueError("kmeans: %d labels are outside [0, %d)" % (counts[-1], len(self.C)))

    def result(self):
        return self.labels.copy(), self.C.copy()


class _HipExecutor:
    name = "hip"

    def __init__(self, X):
        import torch
        from . import engine
        self.torch, self.engine = torch, engine
        self.X = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, np.float32)).to("cuda")
        N, dev = int(self.X.shape[0]), self.X.device
        self.labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
        self.dist = torch.empty(N, dtype=torch.float32, device=dev)
        self.scratch_labels = torch.empty(N, dtype=torch.int32, device=dev)
        self.C = self.counts = None

    def dist_to_row(self, i: int) -> np.ndarray:
        self.engine.kmeans_assign(self.X, self.X[i:i + 1], self.scratch_labels, self.dist)
        return self.dist.cpu().numpy()

    def start(self, rows):
        self.C = self.X[self.torch.as_tensor(np.asarray(rows), device=self.X.device)].contiguous()
        self.counts = self.torch.empty(len(rows) + 1, dtype=self.torch.int32, device=self.X.device)

    def assign(self) -> int:
        return self.engine.kmeans_assign(self.X, self.C, self.labels, self.dist)

    def update(self):
        self.engine.kmeans_update(self.X, self.labels, self.C, self.counts)

    def result(self):
        return self.labels.cpu().numpy(), self.C.cpu().numpy()


def _kmeans(ex, N: int, k: int, seed, max_iter: int):
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError("kmeans: k = %d is outside 1 .. %d" % (k, KMEANS_MAX_K))
    if max_iter < 1:
        raise ValueError("kmeans: max_iter must be at least 1")
    rng = np.random.default_rng(seed)
    # k-means++: the first centre uniformly, every further one with probability proportional to the squared distance to the nearest
    # centre so far.  Every draw is made here, from distances both executors give with the same bits
    rows = [int(rng.integers(N))]
    mind = ex.dist_to_row(rows[0]).astype(np.float64)
    for _ in range(1, k):
        cum = np.cumsum(mind)
        if cum[-1] > 0:
            nxt = min(int(np.searchsorted(cum, rng.random() * cum[-1], side="right")), N - 1)
        else:                                           # fewer distinct rows than centres: a duplicate, its cluster will be empty
            nxt = int(rng.integers(N))
        rows.append(nxt)
        mind = np.minimum(mind, ex.dist_to_row(nxt).astype(np.float64))
    ex.start(rows)
    iterations = 0
    for _ in range(max_iter):
        iterations += 1
        if ex.assign() == 0:
            break
        ex.update()
    labels, centres = ex.result()
    return labels, centres, iterations


def kmeans_host(X, k: int, seed=None, max_iter: int = 50):
    """Lloyd's k-means of the rows of X [N, D] (float32) with a k-means++ start: -> (labels int32 [N], centres float32 [k, D], iterations).
    Every draw comes from np.random.default_rng(seed).  Iterations (assign; stop when no label changed; else move every centre to the
    mean of its members, an empty cluster keeping its centre) run at most max_iter times.  The numpy executor: every sum in the order
    of the HIP kernels, so kmeans_hip returns the same bits."""
    X = np.asarray(X, np.float32)
    if X.ndim != 2 or not len(X):
        raise ValueError("kmeans_host: X must be a non-empty [N, D] matrix")
    return _kmeans(_HostExecutor(X), len(X), int(k), seed, int(max_iter))


def kmeans_hip(X, k: int, seed=None, max_iter: int = 50):
    """kmeans_host on the GPU (engine.kmeans_assign / kmeans_update): X is a numpy array or a float32 device tensor [N, D].  The k-means++
    draws stay on the host: the N distances to each new centre are downloaded (k copies of 4 N bytes) and the running minimum is kept
    in numpy."""
    ex = _HipExecutor(X)
    if ex.X.dim() != 2 or not ex.X.shape[0]:
        raise ValueError("kmeans_hip: X must be a non-empty [N, D] matrix")
    return _kmeans(ex, int(ex.X.shape[0]), int(k), seed, int(max_iter))


# =====================================================================================================
# selection
# =====================================================================================================
def _window(n_frames: int, start: float, stop: float):
    return int(np.floor(n_frames * start)), int(np.ceil(n_frames * stop))


def candidate_indices(n_frames: int, start: float = 0., stop: float = 1., index=None, step: int = 1) -> np.ndarray:
    """frameselectiontools.py:158-165: arange(startindex, stopindex, step), or a given index cropped to the entries STRICTLY inside
    (startindex, stopindex)"""
    a, b = _window(n_frames, start, stop)
    if index is None:
        return np.arange(a, b, step)
    index = np.array(index, dtype=np.int64).reshape(-1)
    return index[(index > a) & (index < b)]


def uniform_select(n_frames: int, numframes2pick: int, start: float = 0., stop: float = 1., index=None, seed=None) -> list:
    """UniformFramescv2 (frameselectiontools.py:45-69): numframes2pick frames drawn without replacement from [floor(n start), ceil(n stop));
    with an index, a random numframes2pick of its entries strictly inside the window, or all of them when there are fewer."""
    rng = np.random.default_rng(seed)
    a, b = _window(n_frames, start, stop)
    if index is None:
        return [int(v) for v in rng.choice(np.arange(a, b), size=numframes2pick, replace=False)]
    idx = candidate_indices(n_frames, start, stop, index)
    if len(idx) >= numframes2pick:
        return [int(v) for v in rng.permutation(idx)[:numframes2pick]]
    return [int(v) for v in idx]


def _frame_shape(source):
    W, H = source.size
    return int(H), int(W)


def _has_jpeg(source) -> bool:
    return hasattr(source, "jpeg_bytes") and bool(getattr(source, "jpeg_only", True))


def device_frame_pass(source, idx, reduce, chunk: int = 256, stats: Optional[dict] = None) -> None:
    """The "hip" backend's read loop: the frames idx of `source`, chunk by chunk, as device uint8 [n, H, W, 3] handed to
    reduce(first position in idx, frames).  Only those frames are read.  A JPEG source (jpeg_bytes: a Motion-JPEG .avi, a directory of
    .jpg files) is Huffman-decoded on at most DECODE_THREADS host threads and reconstructed on the device (engine.jpeg_reconstruct); any
    other source is staged through two pinned buffers, each refilled only after its copy has completed."""
    import torch
    from . import engine
    stats = stats if stats is not None else {}
    stats.setdefault("read_s", 0.0)
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = _frame_shape(source)
    chunk = max(1, int(chunk))
    if _has_jpeg(source):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max(1, min(int(DECODE_THREADS), 8))) as pool:
            for p0 in range(0, len(idx), chunk):
                t0 = time.perf_counter()
                part = [int(i) for i in idx[p0:p0 + chunk]]
                blobs = list(pool.map(source.jpeg_bytes, part))
                infos = list(pool.map(engine.jpeg_probe, blobs))
                i0 = infos[0]
                for i, inf in zip(part, infos):
                    if (inf.width, inf.height, inf.sampling) != (W, H, i0.sampling):
                        raise ValueError("frame %d is %d x %d (sampling %d), the video is %d x %d (sampling %d)"
                                         % (i, inf.width, inf.height, inf.sampling, W, H, i0.sampling))
                coef = np.empty((len(part), i0.total_blocks, 64), np.int16)
                qt = np.empty((len(part), i0.ncomp, 64), np.uint16)
                list(pool.map(lambda j: engine.jpeg_entropy_decode(blobs[j], infos[j], coef[j], qt[j]), range(len(part))))
                stats["read_s"] += time.perf_counter() - t0
                frames = engine.jpeg_reconstruct(torch.from_numpy(coef).to(dev), torch.from_numpy(qt.view(np.int16)).to(dev), H, W, i0.sampling)
                reduce(p0, frames)
        return
    pinned = [torch.empty((chunk, H, W, 3), dtype=torch.uint8).pin_memory() for _ in range(2 if len(idx) > chunk else 1)]
    copied = [None] * len(pinned)
    stack = getattr(source, "frames", None)
    for n, p0 in enumerate(range(0, len(idx), chunk)):
        t0 = time.perf_counter()
        part = np.asarray(idx[p0:p0 + chunk], dtype=np.int64)
        slot = n % len(pinned)
        if copied[slot] is not None:
            copied[slot].synchronize()
        host = pinned[slot].numpy()[:len(part)]
        if isinstance(stack, np.ndarray) and stack.dtype == np.uint8:
            np.take(stack, part, axis=0, out=host)
        else:
            for j, i in enumerate(part):
                np.copyto(host[j], np.asarray(source.frame_at(int(i)), dtype=np.uint8))
        stats["read_s"] += time.perf_counter() - t0
        frames = pinned[slot][:len(part)].to(dev, non_blocking=True)
        copied[slot] = torch.cuda.Event()
        copied[slot].record()
        reduce(p0, frames)
    torch.cuda.synchronize(dev)


def _read_host(source, idx) -> np.ndarray:
    stack = getattr(source, "frames", None)
    if isinstance(stack, np.ndarray) and stack.dtype == np.uint8:
        return stack[np.asarray(idx, dtype=np.int64)]
    return np.stack([np.asarray(source.frame_at(int(i)), dtype=np.uint8) for i in idx])


def kmeans_select(source, numframes2pick: int, start: float = 0., stop: float = 1., index=None, step: int = 1, resizewidth: int = 30,
                  color: bool = False, crop=None, max_iter: int = 50, seed=None, backend: str = "auto", chunk: int = 256) -> list:
    """KmeansbasedFrameselectioncv2 (frameselectiontools.py:139-246) on a frame source (frames.open_frame_source): the candidates
    (candidate_indices) are shrunk to thumbnails resizewidth wide, centred, clustered into numframes2pick clusters, and one member of
    every non-empty cluster is drawn at random -- so fewer than numframes2pick frames may come back.  Fewer than numframes2pick - 1
    candidates are returned as they are.  crop = (x1, x2, y1, y2).  Every random draw is the host's, from `seed`.

    backend "hip": only the candidates are read (device_frame_pass), reduced chunk by chunk into one device feature matrix
    (engine.frame_features), centred and clustered there (kmeans_hip); "host": features_host + kmeans_host, the same picks for the same
    seed -- the CPU fallback and the tests' reference; "sklearn": features_host + MiniBatchKMeans(n_clusters, tol=1e-3, batch_size,
    max_iter) as the reference calls it; "auto": "hip" when a GPU is visible (then the HIP library must load), else "host".
    SELECT_STATS describes the run."""
    if backend == "auto":
        import torch
        backend = "hip" if torch.cuda.is_available() else "host"
    if backend not in ("hip", "host", "sklearn"):
        raise ValueError("kmeans_select: backend must be auto | hip | host | sklearn, not %r" % (backend,))
    numframes2pick = int(numframes2pick)
    t_all = time.perf_counter()
    idx = candidate_indices(source.n_frames, start, stop, index, step)
    SELECT_STATS.clear()
    SELECT_STATS.update(backend=backend, candidates=int(len(idx)), frames_read=0, iterations=0, read_s=0.0, features_s=0.0, kmeans_s=0.0,
                        total_s=0.0)
    if numframes2pick < 1:
        return []
    if len(idx) < numframes2pick - 1 or len(idx) == 0:
        return [int(v) for v in idx]
    if ((idx < 0) | (idx >= source.n_frames)).any():
        raise ValueError("kmeans_select: the index leaves the video's %d frames" % source.n_frames)
    H, W = _frame_shape(source)
    D = feature_geometry(H, W, resizewidth, color, crop)[-1]
    if len(idx) * D * 4 > FEATURE_BYTES:
        raise ValueError("kmeans_select: %d candidates x %d values are %d bytes of features, above FEATURE_BYTES = %d: raise `step` "
                         "(or narrow start / stop)" % (len(idx), D, len(idx) * D * 4, FEATURE_BYTES))
    s_kmeans, s_pick = np.random.SeedSequence(seed).spawn(2)
    k = numframes2pick
    if k > KMEANS_MAX_K and backend != "sklearn":
        raise ValueError("kmeans_select: numframes2pick = %d is above the limit of %d clusters" % (numframes2pick, KMEANS_MAX_K))
    t0 = time.perf_counter()
    if backend == "hip":
        import torch
        from . import engine
        X = torch.empty((len(idx), D), dtype=torch.float32, device="cuda")
        device_frame_pass(source, idx, lambda p0, fr: engine.frame_features(fr, resizewidth, color, crop, out=X[p0:p0 + fr.shape[0]]), chunk,
                          SELECT_STATS)
        torch.cuda.synchronize()
        SELECT_STATS["features_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        engine.kmeans_center(X)
        labels, _, iters = kmeans_hip(X, k, s_kmeans, max_iter)
    else:
        frames = _read_host(source, idx)
        SELECT_STATS["read_s"] = time.perf_counter() - t0
        X = features_host(frames, resizewidth, color, crop)
        del frames
        SELECT_STATS["features_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        X = center_host(X)[0]
        if backend == "host":
            labels, _, iters = kmeans_host(X, k, s_kmeans, max_iter)
        else:
            from sklearn.cluster import MiniBatchKMeans
            batch = 100 if len(idx) >= 100 else int(len(idx) / 2)                  # (:167-169)
            km = MiniBatchKMeans(n_clusters=numframes2pick, tol=1e-3, batch_size=max(batch, 1), max_iter=max_iter,
                                 random_state=int(s_kmeans.generate_state(1)[0]))
            km.fit(X)
            labels, iters = km.labels_, int(km.n_iter_)
    SELECT_STATS["kmeans_s"] = time.perf_counter() - t0
    rng = np.random.default_rng(s_pick)
    picks = []
    for c in range(numframes2pick):                     # one frame per non-empty cluster (:237-242)
        members = np.nonzero(labels == c)[0]
        if len(members):
            picks.append(int(idx[members[int(rng.integers(len(members)))]]))
    SELECT_STATS.update(frames_read=int(len(idx)), iterations=int(iters), total_s=time.perf_counter() - t_all)
    return picks


# =====================================================================================================
# outlier frames
# =====================================================================================================
def _load_labels(labels):
    if isinstance(labels, (str, os.PathLike)):
        from .models.eval import load_pose_from_dlc_to_dict
        labels = load_pose_from_dlc_to_dict(str(labels))
    return {key: np.asarray(labels[key], dtype=np.float64) for key in ("x", "y", "likelihoods")}


def outlier_indices(labels, method: str = "jump", epsilon: float = 20, p_bound: float = .01, start: float = 0., stop: float = 1.,
                    bodyparts="all") -> np.ndarray:
    """The putative outlier frames of a labeled video (outlier_frames.py:136-174).  labels: estimate_pose's dict (x, y, likelihoods as
    [n_frames, n_bodyparts]) or the path of its csv.  The window is [max(floor(n start), 0), min(ceil(n stop), n)).
    "jump": frames where a body part moved more than epsilon pixels since the frame before (dx^2 + dy^2 > epsilon^2 between consecutive
    frames of the window; reported at the LATER frame); "uncertain": frames where a body part's likelihood < p_bound.  bodyparts: "all" or
    the column numbers to look at.  -> the union over the body parts, sorted and unique (int64)."""
    if method == "fitting":
        raise ValueError("outlier_indices: method 'fitting' fits SARIMAX models with statsmodels, which this package does not depend on; "
                         "use 'jump' or 'uncertain'")
    if method == "manual":
        raise ValueError("outlier_indices: method 'manual' is the reference's GUI, which is not part of this package")
    if method not in ("jump", "uncertain"):
        raise ValueError("outlier_indices: method must be jump | uncertain, not %r" % (method,))
    lab = _load_labels(labels)
    n, nj = lab["x"].shape
    a, b = max(int(np.floor(n * start)), 0), min(int(np.ceil(n * stop)), n)
    parts = range(nj) if isinstance(bodyparts, str) and bodyparts == "all" else [int(j) for j in bodyparts]
    found = []
    for j in parts:
        if not 0 <= j < nj:
            raise ValueError("outlier_indices: body part %d is not one of the %d columns" % (j, nj))
        if method == "uncertain":
            found.extend(np.nonzero(lab["likelihoods"][a:b, j] < p_bound)[0] + a)
        else:
            dx, dy = np.diff(lab["x"][a:b, j]), np.diff(lab["y"][a:b, j])
            found.extend(np.nonzero(dx ** 2 + dy ** 2 > epsilon ** 2)[0] + a + 1)
    return np.array(sorted(set(int(v) for v in found)), dtype=np.int64)


# =====================================================================================================
# drivers: pick, write the frames (and the machine labels) into <project>/labeled-data/<video stem>/
# =====================================================================================================
def _project(config):
    from .config import read_config
    cfg = read_config(config)
    root = Path(cfg.get("project_path") or Path(config).resolve().parent)
    if not root.is_dir():
        root = Path(config).resolve().parent
    coords = tuple(int(cfg[key]) for key in ("x1", "x2", "y1", "y2")) if cfg.get("cropping") else None
    return cfg, root, coords


def image_name(index: int, n_frames: int) -> str:
    """img<index zero-filled to ceil(log10 n_frames)>.png (utils_data.py:57, outlier_frames.py:350)"""
    return "img" + str(int(index)).zfill(int(np.ceil(np.log10(n_frames)))) + ".png"


def _write_frames(source, picks, folder: Path, coords) -> None:
    from PIL import Image
    folder.mkdir(parents=True, exist_ok=True)
    for i in picks:
        frame = np.asarray(source.frame_at(int(i)), dtype=np.uint8)
        if coords is not None:
            frame = frame[coords[2]:coords[3], coords[0]:coords[1]]
        Image.fromarray(np.ascontiguousarray(frame)).save(str(folder / image_name(i, source.n_frames)))


def _select(source, cfg, algo, numframes2pick, coords, index, select_kw):
    n2p = int(cfg["numframes2pick"] if numframes2pick is None else numframes2pick)
    kw = dict(select_kw)
    start, stop = kw.pop("start", cfg.get("start", 0.)), kw.pop("stop", cfg.get("stop", 1.))
    if algo == "kmeans":
        return kmeans_select(source, n2p, start, stop, index=index, crop=coords, **kw)
    if algo == "uniform":
        return uniform_select(source.n_frames, n2p, start, stop, index=index, seed=kw.get("seed"))
    raise ValueError("the extraction algorithm must be kmeans | uniform, not %r" % (algo,))


def extract_frames(config, video, numframes2pick=None, algo: str = "kmeans", crop=None, **select_kw) -> list:
    """Pick frames of `video` to label and write them as <project>/labeled-data/<video stem>/img<NNN>.png (DGP/utils_data.py:52-71 over
    DLC's extract_frames).  numframes2pick, start, stop and the crop (cropping, x1, x2, y1, y2) default to config.yaml's keys; crop =
    (x1, x2, y1, y2) overrides the file's, crop=False switches it off.  The crop bounds the thumbnails AND the written images, as in the
    reference.  select_kw goes to kmeans_select (seed, backend, step, resizewidth, color, ...).  -> the picked frame numbers."""
    from .frames import open_frame_source
    cfg, root, coords = _project(config)
    if crop is not None:
        coords = tuple(int(v) for v in crop) if crop else None
    source = open_frame_source(video)
    try:
        picks = _select(source, cfg, algo, numframes2pick, coords, None, select_kw)
        _write_frames(source, picks, root / "labeled-data" / Path(str(video)).stem, coords)
    finally:
        source.close()
    return [int(i) for i in picks]


def _machine_labels(label_file, rows, names):
    """the rows `rows` of a DLC-format csv as a DataFrame in its layout (export_pose_like_dlc's columns), index = names"""
    import pandas as pd
    df = pd.read_csv(label_file, header=[0, 1, 2], index_col=0)
    out = df.iloc[list(rows)].copy()
    out.index = list(names)
    return out


def extract_outlier_frames(config, video, label_file=None, outlieralgorithm: str = "jump", extractionalgorithm: str = "kmeans",
                           epsilon: float = 20, p_bound: float = .01, comparisonbodyparts="all", **select_kw) -> list:
    """Find the frames of a labeled video the model most likely got wrong, pick numframes2pick of them and write them with their machine
    labels for refinement (outlier_frames.py:119-193, :293-396).  The labels are read from <video folder>/<stem>_labeled.csv, what
    estimate_pose / plot_dgp write (label_file: another path).  outlier_indices(outlieralgorithm, epsilon, p_bound, config's start / stop,
    comparisonbodyparts: "all" or names out of config's bodyparts) gives the candidates, kmeans_select / uniform_select
    (extractionalgorithm) picks among them, and <project>/labeled-data/<stem>/ gets img<NNN>.png per pick, machinelabels.csv and -- when
    pytables imports -- machinelabels-iter<iteration>.h5: the picked rows of the label file, index = the image paths, merged with an
    existing file (duplicates dropped, the first kept).  config.yaml is NOT rewritten: like the reference when its own rewrite fails,
    a printed line names the video and the crop to add by hand.  -> the picked frame numbers."""
    import pandas as pd
    from .frames import open_frame_source
    cfg, root, coords = _project(config)
    stem = Path(str(video)).stem
    if label_file is None:
        label_file = str(Path(str(video)).parent / (stem + "_labeled.csv"))
    lab = _load_labels(label_file)
    names = list(cfg.get("bodyparts") or [])
    if isinstance(comparisonbodyparts, str) and comparisonbodyparts == "all":
        parts = "all"
    else:
        parts = [names.index(bp) for bp in comparisonbodyparts if bp in names]          # (:145 "who knows what users put in")
    found = outlier_indices(lab, outlieralgorithm, epsilon, p_bound, cfg.get("start", 0.), cfg.get("stop", 1.), parts)
    print("Method ", outlieralgorithm, " found ", len(found), " putative outlier frames.")
    source = open_frame_source(video)
    try:
        picks = [int(i) for i in _select(source, cfg, extractionalgorithm, None, coords, found, select_kw)]
        folder = root / "labeled-data" / stem
        _write_frames(source, picks, folder, coords)
        n_frames = source.n_frames
    finally:
        source.close()
    if not picks:
        print("No frames were extracted.")
        return picks
    rel = [os.path.join("labeled-data", stem, image_name(i, n_frames)) for i in picks]
    df = _machine_labels(label_file, picks, rel)
    csv = folder / "machinelabels.csv"
    if csv.is_file():
        old = pd.read_csv(csv, header=[0, 1, 2], index_col=0)
        old.columns = df.columns
        df = pd.concat([old, df])
        df = df[~df.index.duplicated(keep="first")]                                      # (:374-376)
    try:
        df.to_hdf(str(folder / ("machinelabels-iter%s.h5" % cfg.get("iteration", 0))), key="df_with_missing", mode="w")
    except ImportError:
        print("pytables not installed: skipping machinelabels-iter%s.h5 (machinelabels.csv is written)" % cfg.get("iteration", 0))
    df.to_csv(csv)
    print("config.yaml is not rewritten: add this video to its video_sets by hand before the next training set is made.")
    print("Video path:", video, "-- crop (x1, x2, y1, y2):", coords)
    return picks
