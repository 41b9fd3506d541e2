"""Inputs shared by tests/test_frame_selection_cpu.py and tests/test_frame_selection_gpu.py: built once, never modified."""
import functools

import numpy as np

# (N, H, W, resizewidth, k): k noisy copies of k base frames; SEED is one for which kmeans_host recovers the partition of both
PLANTED = ((67, 37, 53, 7, 5), (300, 48, 64, 30, 20))
SEED = 1

# (N, D, k) of the assign tests
ASSIGN_SHAPES = ((1, 1, 1), (67, 35, 5), (300, 690, 20), (257, 2070, 33), (1000, 7, 100))


@functools.lru_cache(maxsize=None)
def planted(N, H, W, k):
    """(frames uint8 [N, H, W, 3], the planted cluster of every frame)"""
    r = np.random.default_rng(1)
    base = r.integers(0, 256, (k, H, W, 3))
    member = np.arange(N) % k
    r.shuffle(member)
    frames = np.clip(base[member] + r.integers(-12, 13, (N, H, W, 3)), 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return frames, member


@functools.lru_cache(maxsize=None)
def planted_features(N, H, W, ow, k):
    """the centred thumbnails of planted(): what both executors cluster"""
    from deepgraphpose_amd import frame_selection as F
    X = F.center_host(F.features_host(planted(N, H, W, k)[0], ow))[0]
    X.setflags(write=False)
    return X


def same_partition(a, b) -> bool:
    """two labelings group the rows alike (cluster numbers may differ)"""
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


@functools.lru_cache(maxsize=None)
def assign_case(N, D, k):
    """(X float32 [N, D], C float32 [k, D]): centres drawn at random with the spread of centred thumbnails, row i a noisy copy of centre
    i % k (noise as wide as the centres: at large D every row is clearly nearest to its own centre, at D = 7 many are not)"""
    r = np.random.default_rng(1000 * N + D + k)
    C = (r.standard_normal((k, D)) * 30.0).astype(np.float32)
    X = (C[np.arange(N) % k] + r.standard_normal((N, D)) * 30.0).astype(np.float32)
    X.setflags(write=False)
    C.setflags(write=False)
    return X, C


def dist_bound(D: int) -> float:
    """relative error bound of an fp32 sum of D non-negative terms (x - c)^2, each with its own two roundings"""
    return (D + 4) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def assign_reference(N, D, k):
    """float64: (labels, distance to the nearest centre, mask of the rows whose relative gap (d2 - d1) / d2 to the second nearest centre
    is at least twice dist_bound -- the rows on which an fp32 executor must agree)"""
    X, C = assign_case(N, D, k)
    d = ((X.astype(np.float64)[:, None, :] - C.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    order = np.sort(d, axis=1)
    if k > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.where(order[:, 1] > 0, (order[:, 1] - order[:, 0]) / order[:, 1], 0.0)
    else:
        gap = np.full(N, np.inf)
    return d.argmin(1), order[:, 0], gap >= 2 * dist_bound(D)


def frames_for(N, H, W, value=None):
    if value is not None:
        return np.full((N, H, W, 3), value, np.uint8)
    return np.random.default_rng(H * 1000 + W + N).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
