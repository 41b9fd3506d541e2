"""Frame selection on the device (csrc/dgp_select.hip): thumbnails bit for bit against the numpy statement, the three k-means kernels
against float64, the two executors of one algorithm against each other."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _selection_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    return engine


@pytest.fixture(scope="module")
def F():
    from deepgraphpose_amd import frame_selection
    return frame_selection


def dev(a):
    """a numpy array (the shared inputs are read-only) as a device tensor"""
    return torch.from_numpy(np.array(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ frame_features
# (5, 7, 7): ow == Wc, one pixel per column box; (37, 53, 7): odd sizes, byte loads; (48, 64, 30): the 16-byte path, oh at a half-way case;
# (33, 21, 4): 63-byte rows; (256, 256, 2) all 255: the largest sums; (16, 20, 5): rows of 60 bytes, the 4-byte path
FEATURE_CASES = [(5, 7, 7, None), (37, 53, 7, None), (48, 64, 30, None), (33, 21, 4, None), (256, 256, 2, 255), (16, 20, 5, None)]


@pytest.mark.parametrize("color", [False, True], ids=["grey", "color"])
@pytest.mark.parametrize("N", [1, 2, 33])
@pytest.mark.parametrize("H,W,ow,value", FEATURE_CASES, ids=lambda v: str(v))
def test_frame_features_equal_the_host_statement(eng, F, H, W, ow, value, N, color):
    frames = S.frames_for(N, H, W, value)
    want = F.features_host(frames, ow, color)
    got = eng.frame_features(dev(frames), ow, color)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    if value is not None:
        assert (want == float(value)).all()


@pytest.mark.parametrize("color", [False, True], ids=["grey", "color"])
@pytest.mark.parametrize("H,W,ow,crop", [(37, 53, 7, (3, 48, 2, 30)),         # odd x1, 45 pixels = 135 bytes wide
                                         (48, 64, 9, (5, 62, 1, 47)),         # the 16-byte path: the window starts and ends inside a unit
                                         (16, 20, 5, (1, 19, 0, 16)),         # the 4-byte path likewise
                                         (48, 64, 1, (63, 64, 0, 48))])       # one column
def test_frame_features_crop(eng, F, H, W, ow, crop, color):
    frames = S.frames_for(3, H, W)
    want = F.features_host(frames, ow, color, crop)
    got = eng.frame_features(dev(frames), ow, color, crop)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


@pytest.mark.parametrize("offset,pad", [(1, 0), (3, 5), (16, 7), (4, 4)])
def test_frame_features_of_a_view_at_any_byte_offset(eng, F, offset, pad):
    """frames that start `offset` bytes into an allocation and lie H W 3 + pad bytes apart"""
    N, H, W = 5, 48, 64
    frames = S.frames_for(N, H, W)
    fb = H * W * 3
    buf = torch.zeros(offset + N * (fb + pad) + 16, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (N, H, W, 3), (fb + pad, W * 3, 3, 1), offset)
    view.copy_(dev(frames))
    assert view.data_ptr() % 16 == offset % 16
    for color in (False, True):
        got = eng.frame_features(view, 30, color, (1, 64, 0, 48))
        assert np.array_equal(bits(got.cpu().numpy()), bits(F.features_host(frames, 30, color, (1, 64, 0, 48))))


def test_frame_features_writes_only_its_values(eng, F):
    N, H, W, ow = 4, 37, 53, 7
    frames = S.frames_for(N, H, W)
    want = F.features_host(frames, ow, True)
    D = want.shape[1]
    buf = torch.full((N + 2, D + 5), -7.0, dtype=torch.float32, device="cuda")
    out = buf[1:N + 1, 2:D + 2]
    assert eng.frame_features(dev(frames), ow, True, out=out) is out
    host = buf.cpu().numpy()
    assert np.array_equal(bits(host[1:N + 1, 2:D + 2]), bits(want))
    host[1:N + 1, 2:D + 2] = -7.0
    assert (host == -7.0).all()


def test_frame_features_refusals(eng):
    from deepgraphpose_amd._lib import DgpError
    fr = torch.zeros((2, 12, 20, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="upsamples"):
        eng.frame_features(fr, 21)
    with pytest.raises(ValueError, match="upsamples"):
        eng.frame_features(fr, 8, crop=(2, 9, 0, 12))
    for crop in ((0, 21, 0, 12), (5, 5, 0, 12), (0, 20, 3, 2), (-1, 20, 0, 12)):
        with pytest.raises(ValueError, match="crop"):
            eng.frame_features(fr, 4, crop=crop)
    with pytest.raises(ValueError, match="positive"):
        eng.frame_features(fr, 0)
    with pytest.raises(ValueError, match="limit"):
        eng.frame_features(torch.empty((1, 2400, 2400, 3), dtype=torch.uint8, device="cuda"), 1)        # a box of 5.76 M pixels
    with pytest.raises(ValueError, match="limits"):
        eng.frame_features(torch.empty((1, 1, 16385, 3), dtype=torch.uint8, device="cuda"), 30)
    with pytest.raises(DgpError):
        eng.frame_features(fr.float(), 4)
    with pytest.raises(DgpError):
        eng.frame_features(fr.cpu(), 4)
    with pytest.raises(DgpError):
        eng.frame_features(fr[..., :2], 4)
    with pytest.raises(DgpError):
        eng.frame_features(fr[:, :, ::2], 4)
    with pytest.raises(DgpError, match="out"):
        eng.frame_features(fr, 4, out=torch.empty((2, 7), dtype=torch.float32, device="cuda"))
    with pytest.raises(DgpError, match="stride"):
        eng.frame_features(fr, 4, out=torch.empty((8, 2), dtype=torch.float32, device="cuda").t()[:, :8][:2])
    assert eng.frame_features(fr[:0], 4).shape == (0, 8)


def test_frame_features_c_abi_checks_before_launch(eng):
    """the C entry point refuses on its own what the wrapper never lets through"""
    import ctypes as C
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    fr = torch.zeros((1, 12, 20, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    call = lambda *a: lib.dgp_frame_features_u8(C.c_void_p(fr.data_ptr()), *a, C.c_void_p(out.data_ptr()), 64, None)
    assert call(1, 12, 20, 720, 0, 20, 0, 12, 4, 2, 0) == 0
    assert call(1, 12, 20, 720, 0, 20, 0, 12, 4, 3, 0) != 0 and b"rule" in lib.dgp_last_error()      # oh is 12 * 4 / 20 = 2.4 -> 2
    assert call(1, 12, 20, 720, 0, 20, 0, 12, 21, 13, 0) != 0 and b"upsamples" in lib.dgp_last_error()
    assert call(1, 12, 20, 719, 0, 20, 0, 12, 4, 2, 0) != 0 and b"stride" in lib.dgp_last_error()
    assert call(1, 12, 20, 720, 0, 21, 0, 12, 4, 2, 0) != 0 and b"window" in lib.dgp_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ kmeans_assign
@pytest.mark.parametrize("N,D,k", S.ASSIGN_SHAPES, ids=lambda v: str(v))
def test_kmeans_assign_against_float64(eng, F, N, D, k):
    X, C = S.assign_case(N, D, k)
    ref_labels, ref_dist, clear = S.assign_reference(N, D, k)
    Xd, Cd = dev(X), dev(C)
    labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    dist = torch.full((N,), -1.0, dtype=torch.float32, device="cuda")
    changed = eng.kmeans_assign(Xd, Cd, labels, dist)
    got_l, got_d = labels.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    assert changed == N                                               # every label was -1
    assert ((got_l >= 0) & (got_l < k)).all()
    # the reported distance is the one to the REPORTED centre, within the bound of an fp32 sum of D terms
    to_own = ((X.astype(np.float64) - C.astype(np.float64)[got_l]) ** 2).sum(1)
    rel = np.abs(got_d - to_own) / np.maximum(to_own, np.finfo(np.float64).tiny)
    print("max relative distance error %.3g (bound %.3g), rows left out %d of %d" % (rel.max(), S.dist_bound(D), (~clear).sum(), N))
    assert rel.max() <= S.dist_bound(D)
    assert (~clear).sum() <= 0.01 * N
    assert np.array_equal(got_l[clear], ref_labels[clear])
    assert (np.abs(got_d - ref_dist)[clear] <= S.dist_bound(D) * ref_dist[clear]).all()
    # the numpy executor states the same order of sums: the same bits
    host_l, host_d = F.assign_host(X, C)
    assert np.array_equal(host_l, got_l) and np.array_equal(bits(host_d), bits(dist.cpu().numpy()))
    # changed counts exactly the rows whose label differs from the one that was there
    assert eng.kmeans_assign(Xd, Cd, labels, dist) == 0
    if k > 1:
        moved = np.arange(0, N, 3)
        wrong = got_l.copy()
        wrong[moved] = (wrong[moved] + 1) % k
        wrong[N // 2] = 12345                                         # any value may have been there
        labels.copy_(torch.from_numpy(wrong).cuda())
        assert eng.kmeans_assign(Xd, Cd, labels, dist) == int((wrong != got_l).sum())
        assert np.array_equal(labels.cpu().numpy(), got_l)


def test_kmeans_assign_tie_goes_to_the_lower_index(eng):
    X, C = S.assign_case(300, 690, 20)
    popular = int(np.bincount(S.assign_reference(300, 690, 20)[0], minlength=20).argmax())
    lo, mid, hi = 4, 9, 17
    C = C.copy()
    C[lo] = C[mid] = C[hi] = C[popular]                               # the centre most rows are nearest to, three times
    labels = torch.full((300,), -1, dtype=torch.int32, device="cuda")
    dist = torch.empty(300, dtype=torch.float32, device="cuda")
    eng.kmeans_assign(dev(X), dev(C), labels, dist)
    got = labels.cpu().numpy()
    assert (got == min(lo, popular)).any() and not (got == mid).any() and not (got == hi).any()
    # rows that ARE a centre: distance exactly 0 to three centres
    Xd = torch.from_numpy(np.ascontiguousarray(C[[mid, hi, lo]])).cuda()
    labels = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    dist = torch.empty(3, dtype=torch.float32, device="cuda")
    eng.kmeans_assign(Xd, torch.from_numpy(C).cuda(), labels, dist)
    assert labels.cpu().tolist() == [min(lo, popular)] * 3 and dist.cpu().tolist() == [0.0] * 3


def test_kmeans_limits_are_refused(eng):
    X = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    lab = torch.zeros(4, dtype=torch.int32, device="cuda")
    dist = torch.zeros(4, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="160"):
        eng.kmeans_assign(X, torch.zeros((161, 3), dtype=torch.float32, device="cuda"), lab, dist)
    with pytest.raises(ValueError, match="8192"):
        eng.kmeans_center(torch.zeros((1, 8193), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="belong together"):
        eng.kmeans_assign(X, torch.zeros((2, 4), dtype=torch.float32, device="cuda"), lab, dist)
    with pytest.raises(ValueError, match="belong together"):
        eng.kmeans_update(X, lab, torch.zeros((2, 3), dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))
    # the widest and the most centres that are taken
    Xw = torch.ones((3, 8192), dtype=torch.float32, device="cuda")
    lab3, dist3 = torch.full((3,), -1, dtype=torch.int32, device="cuda"), torch.empty(3, dtype=torch.float32, device="cuda")
    assert eng.kmeans_assign(Xw, torch.zeros((160, 8192), dtype=torch.float32, device="cuda"), lab3, dist3) == 3
    assert lab3.cpu().tolist() == [0, 0, 0] and dist3.cpu().tolist() == [8192.0] * 3


# ------------------------------------------------------------------------------------------------ kmeans_update / kmeans_center
def within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()


# (20000, 7, 3): more than 64 x 256 rows, so slabs longer than one tile of labels
UPDATE_SHAPES = S.ASSIGN_SHAPES + ((20000, 7, 3),)


@pytest.mark.parametrize("N,D,k", UPDATE_SHAPES, ids=lambda v: str(v))
def test_kmeans_update_against_float64(eng, F, N, D, k):
    r = np.random.default_rng(N + D + k)
    X = (r.standard_normal((N, D)) * 30.0 + 5.0).astype(np.float32)
    C0 = (r.standard_normal((k, D)) * 30.0).astype(np.float32)
    labels = r.integers(0, k, N).astype(np.int32)
    empty = k - 1 if k > 2 else None
    if empty is not None:
        labels[labels == empty] = 0
    Xd, Ld = torch.from_numpy(X).cuda(), torch.from_numpy(labels).cuda()
    runs = []
    for _ in range(2):
        Cd = torch.from_numpy(C0).cuda()
        counts = torch.full((k + 1,), -1, dtype=torch.int32, device="cuda")
        eng.kmeans_update(Xd, Ld, Cd, counts)
        runs.append((Cd.cpu().numpy(), counts.cpu().numpy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(runs[0][1], runs[1][1])
    got, counts = runs[0]
    assert counts[k] == 0 and np.array_equal(counts[:k], np.bincount(labels, minlength=k))
    for c in range(k):
        if counts[c] == 0:
            assert c == empty and np.array_equal(bits(got[c]), bits(C0[c]))
        else:
            assert within_one_ulp(got[c], X[labels == c].astype(np.float64).mean(0)), c
    host_C, host_counts = F.update_host(X, labels, C0)
    assert np.array_equal(bits(host_C), bits(got)) and np.array_equal(host_counts, counts)


def test_kmeans_update_skips_and_reports_labels_out_of_range(eng):
    X = torch.from_numpy(np.arange(24, dtype=np.float32).reshape(6, 4)).cuda()
    C0 = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    labels = torch.tensor([0, 2, 1, -1, 0, 1 << 30], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="3 labels are outside"):
        eng.kmeans_update(X, labels, C0, counts)
    assert counts.cpu().tolist() == [2, 1, 3]
    assert C0.cpu().tolist() == [[8.0, 9.0, 10.0, 11.0], [8.0, 9.0, 10.0, 11.0]]       # rows 0 and 4; row 2


@pytest.mark.parametrize("N,D", [(1, 1), (67, 35), (300, 690), (1000, 7), (20000, 7)])
def test_kmeans_center_against_float64(eng, F, N, D):
    r = np.random.default_rng(N * 7 + D)
    X = r.integers(0, 256, (N, D)).astype(np.float32) + r.integers(0, 3, (N, D)).astype(np.float32) / 3
    runs = []
    for _ in range(2):
        Xd = torch.from_numpy(X).cuda()
        mean = eng.kmeans_center(Xd)
        runs.append((mean.cpu().numpy(), Xd.cpu().numpy()))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    mean, centred = runs[0]
    assert within_one_ulp(mean, X.astype(np.float64).mean(0))
    assert np.array_equal(bits(centred), bits(X - mean[None, :]))
    host_X, host_mean = F.center_host(X)
    assert np.array_equal(bits(host_mean), bits(mean)) and np.array_equal(bits(host_X), bits(centred))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("N,H,W,ow,k", S.PLANTED, ids=lambda v: str(v))
def test_kmeans_hip_equals_kmeans_host(eng, F, N, H, W, ow, k):
    X = S.planted_features(N, H, W, ow, k)
    host = F.kmeans_host(X, k, S.SEED)
    hip = F.kmeans_hip(np.array(X), k, S.SEED)
    assert S.same_partition(host[0], S.planted(N, H, W, k)[1])
    assert np.array_equal(hip[0], host[0]) and hip[2] == host[2]
    assert np.array_equal(bits(hip[1]), bits(host[1]))


def test_kmeans_select_hip_equals_host_on_an_array(eng, F):
    from deepgraphpose_amd.frames import ArraySource
    N, H, W, ow, k = S.PLANTED[1]
    src = ArraySource(S.planted(N, H, W, k)[0])
    for kw in (dict(), dict(color=True, crop=(3, 60, 2, 45), resizewidth=11), dict(start=0.1, stop=0.9, step=2, chunk=32)):
        host = F.kmeans_select(src, k, seed=S.SEED, backend="host", **kw)
        assert F.SELECT_STATS["backend"] == "host"
        hip = F.kmeans_select(src, k, seed=S.SEED, backend="hip", **kw)
        assert F.SELECT_STATS["backend"] == "hip" and F.SELECT_STATS["frames_read"] == F.SELECT_STATS["candidates"]
        assert hip == host and 1 <= len(hip) <= k, kw
    auto = F.kmeans_select(src, k, seed=S.SEED, backend="auto")
    assert F.SELECT_STATS["backend"] == "hip"         # a GPU is visible
    assert auto == F.kmeans_select(src, k, seed=S.SEED, backend="host")


def test_kmeans_select_hip_on_an_mjpeg_avi_and_a_sparse_index(eng, F, tmp_path):
    from deepgraphpose_amd.frames import open_frame_source, write_mjpeg_avi
    N, H, W, ow, k = S.PLANTED[1]
    path = str(tmp_path / "clip.avi")
    assert write_mjpeg_avi(path, S.planted(N, H, W, k)[0]) == N
    src = open_frame_source(path)
    try:
        assert hasattr(src, "jpeg_bytes")
        host = F.kmeans_select(src, k, seed=S.SEED, backend="host", chunk=64)
        hip = F.kmeans_select(src, k, seed=S.SEED, backend="hip", chunk=64)
        assert hip == host and 1 <= len(hip) <= k
        assert F.SELECT_STATS["frames_read"] == N
        index = [5, 6, 9, 40, 41, 77, 120, 121, 122, 200, 250, 251, 290, 299, 300, 0]       # 0 and 300 are not strictly inside (0, 300)
        read = []
        real = src.jpeg_bytes
        src.jpeg_bytes = lambda i: (read.append(int(i)), real(i))[1]
        hip = F.kmeans_select(src, 4, index=index, seed=3, backend="hip")
        src.jpeg_bytes = real
        assert F.SELECT_STATS["frames_read"] == F.SELECT_STATS["candidates"] == 14 and sorted(read) == sorted(index[:14])
        assert hip == F.kmeans_select(src, 4, index=index, seed=3, backend="host") and set(hip) <= set(index[:14])
    finally:
        src.close()
