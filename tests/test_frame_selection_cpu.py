"""Frame selection on the host (deepgraphpose_amd/frame_selection.py): the index contract of the selectors, the outlier rules, the numpy
statement of the thumbnails, the numpy executor of k-means, the extraction drivers end to end.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _selection_cases as S  # noqa: E402

from deepgraphpose_amd import frame_selection as F  # noqa: E402
from deepgraphpose_amd.frames import ArraySource  # noqa: E402


# ------------------------------------------------------------------------------------------------ the index contract
def test_candidate_indices_by_hand():
    assert F.candidate_indices(100).tolist() == list(range(100))
    assert F.candidate_indices(100, 0.25, 0.5, step=10).tolist() == [25, 35, 45]
    assert F.candidate_indices(10, 0.15, 0.85).tolist() == [1, 2, 3, 4, 5, 6, 7, 8]            # floor(1.5) = 1, ceil(8.5) = 9
    # a given index is cropped to the entries STRICTLY inside (startindex, stopindex); its order and repeats are kept
    assert F.candidate_indices(100, 0.2, 0.6, index=[70, 20, 21, 59, 60, 21, 5]).tolist() == [21, 59, 21]
    assert F.candidate_indices(100, index=[0, 1, 99, 100]).tolist() == [1, 99]


def test_kmeans_select_index_contract():
    N, H, W, ow, k = S.PLANTED[0]
    frames, member = S.planted(N, H, W, k)
    src = ArraySource(frames)
    # fewer than numframes2pick - 1 candidates: all of them, as they are, and nothing is clustered
    assert F.kmeans_select(src, 9, index=[10, 3, 66, 0, 67, 30, 31, 32, 33], backend="host") == [10, 3, 66, 30, 31, 32, 33]
    assert F.SELECT_STATS["frames_read"] == 0 and F.SELECT_STATS["candidates"] == 7
    assert F.kmeans_select(src, 5, start=0.5, stop=0.5, backend="host") == [33]          # floor(33.5) .. ceil(33.5)
    assert F.kmeans_select(src, 5, start=0.6, stop=0.4, backend="host") == []
    # exactly numframes2pick - 1 candidates are clustered: one pick per non-empty cluster, each a candidate
    cand = [10, 3, 66, 30, 31, 32, 33]
    picks = F.kmeans_select(src, 8, index=cand, resizewidth=ow, seed=0, backend="host")
    assert F.SELECT_STATS["frames_read"] == 7 and len(picks) == len(set(picks)) <= 7 and set(picks) <= set(cand)
    # the planted partition: one pick out of every planted cluster
    picks = F.kmeans_select(src, k, resizewidth=ow, seed=S.SEED, backend="host")
    assert sorted(member[picks].tolist()) == list(range(k))
    assert F.SELECT_STATS["backend"] == "host" and F.SELECT_STATS["iterations"] >= 1 and F.SELECT_STATS["total_s"] > 0
    assert picks == F.kmeans_select(src, k, resizewidth=ow, seed=S.SEED, backend="host")
    assert any(picks != F.kmeans_select(src, k, resizewidth=ow, seed=s, backend="host") for s in (7, 8, 9))
    # step and window: the picks are candidates
    picks = F.kmeans_select(src, k, start=0.2, stop=0.8, step=3, resizewidth=ow, seed=2, backend="host")
    assert set(picks) <= set(range(13, 54, 3)) and F.SELECT_STATS["candidates"] == len(range(13, 54, 3))
    with pytest.raises(ValueError, match="backend"):
        F.kmeans_select(src, k, backend="numpy")
    with pytest.raises(ValueError, match="upsamples"):
        F.kmeans_select(src, k, resizewidth=54, backend="host")
    with pytest.raises(ValueError, match="leaves the video"):
        F.kmeans_select(ArraySource(frames[:50]), 3, stop=2.0, index=[10, 20, 60], backend="host")


def test_kmeans_select_refuses_a_feature_matrix_above_the_limit(monkeypatch):
    N, H, W, ow, k = S.PLANTED[0]
    src = ArraySource(S.planted(N, H, W, k)[0])
    monkeypatch.setattr(F, "FEATURE_BYTES", 67 * 35 * 4 - 1)
    with pytest.raises(ValueError, match="step"):
        F.kmeans_select(src, k, resizewidth=ow, backend="host")
    assert len(F.kmeans_select(src, k, resizewidth=ow, step=2, seed=1, backend="host")) >= 1


def test_kmeans_select_sklearn_backend():
    pytest.importorskip("sklearn")
    N, H, W, ow, k = S.PLANTED[0]
    frames, member = S.planted(N, H, W, k)
    picks = F.kmeans_select(ArraySource(frames), k, resizewidth=ow, seed=4, backend="sklearn")
    assert F.SELECT_STATS["backend"] == "sklearn" and 1 <= len(picks) <= k and len(set(member[picks].tolist())) == len(picks)


def test_uniform_select_by_hand():
    picks = F.uniform_select(100, 10, 0.2, 0.5, seed=0)
    assert len(set(picks)) == 10 and all(20 <= p < 50 for p in picks)
    assert picks == F.uniform_select(100, 10, 0.2, 0.5, seed=0) != F.uniform_select(100, 10, 0.2, 0.5, seed=1)
    assert sorted(F.uniform_select(10, 10, 0., 1., seed=3)) == list(range(10))
    with pytest.raises(ValueError):
        F.uniform_select(10, 11, 0., 1.)                                                # more than there are, without replacement
    index = [5, 20, 21, 30, 49, 50, 80]
    assert F.uniform_select(100, 10, 0.2, 0.5, index=index) == [21, 30, 49]             # fewer than asked for: all, in order
    picks = F.uniform_select(100, 2, 0.2, 0.5, index=index, seed=5)
    assert len(picks) == 2 and set(picks) < {21, 30, 49}


# ------------------------------------------------------------------------------------------------ outlier_indices
def trajectory():
    n = 40
    x = np.tile(np.arange(n, dtype=float)[:, None], (1, 3))          # every body part walks one pixel a frame
    y = np.zeros((n, 3))
    p = np.full((n, 3), 0.9)
    x[10:, 0] += 30.0                                                # part 0 jumps between frames 9 and 10 ...
    y[25, 1] = 20.0                                                  # part 1 leaves at 25 and comes back at 26: exactly sqrt(1 + 400) each way
    x[31:, 2] += 19.0                                                # part 2 moves 20 pixels in x between 30 and 31: dx^2 = 400, not > 400
    x[10:, 2] += 25.0                                                # ... and jumps at frame 10 too
    p[4, 0], p[17, 2], p[18, 1], p[4, 1] = 0.001, 0.0, 0.01, 0.5
    return {"x": x, "y": y, "likelihoods": p}


def test_outlier_indices_on_a_hand_built_trajectory():
    lab = trajectory()
    got = F.outlier_indices(lab, "jump", epsilon=20)
    assert got.dtype == np.int64 and got.tolist() == [10, 25, 26]    # the LATER frame; 10 once although two parts jump there
    assert F.outlier_indices(lab, "jump", epsilon=20, bodyparts=[2]).tolist() == [10]          # dx = 20 at frame 31 is not > epsilon
    assert F.outlier_indices(lab, "jump", epsilon=19.9, bodyparts=[2]).tolist() == [10, 31]
    assert F.outlier_indices(lab, "jump", epsilon=20, bodyparts=[1, 0]).tolist() == [10, 25, 26]
    # the window [floor(40 * .5), ceil(40 * .9)) = [20, 36): the jump at 10 is outside, offsets are applied
    assert F.outlier_indices(lab, "jump", epsilon=20, start=0.5, stop=0.9).tolist() == [25, 26]
    # a window that STARTS at the jump does not see it: the difference to the frame before the window is never formed
    assert F.outlier_indices(lab, "jump", epsilon=20, start=0.25, stop=0.5).tolist() == []
    assert F.outlier_indices(lab, "jump", epsilon=20, start=0.225, stop=0.5).tolist() == [10]
    # uncertain: strictly below p_bound
    assert F.outlier_indices(lab, "uncertain", p_bound=0.01).tolist() == [4, 17]
    assert F.outlier_indices(lab, "uncertain", p_bound=0.0100001).tolist() == [4, 17, 18]
    assert F.outlier_indices(lab, "uncertain", p_bound=0.6, bodyparts=[1]).tolist() == [4, 18]
    assert F.outlier_indices(lab, "uncertain", p_bound=0.01, start=0.25).tolist() == [17]
    with pytest.raises(ValueError, match="statsmodels"):
        F.outlier_indices(lab, "fitting")
    with pytest.raises(ValueError, match="GUI"):
        F.outlier_indices(lab, "manual")
    with pytest.raises(ValueError, match="jump | uncertain".replace("|", r"\|")):
        F.outlier_indices(lab, "arima")
    with pytest.raises(ValueError, match="body part"):
        F.outlier_indices(lab, "jump", bodyparts=[3])


# ------------------------------------------------------------------------------------------------ features_host
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("H,W,ow,crop", [(37, 53, 7, None), (48, 64, 30, None), (33, 21, 4, (3, 20, 1, 30)), (5, 7, 7, None)])
def test_features_host_boxes_tile_the_window(H, W, ow, crop, color):
    frames = S.frames_for(3, H, W)
    x1, x2, y1, y2, oh, _, D = F.feature_geometry(H, W, ow, color, crop)
    X = F.features_host(frames, ow, color, crop)
    assert X.dtype == np.float32 and X.shape == (3, D)
    ye, xe = F.box_edges(y2 - y1, oh), F.box_edges(x2 - x1, ow)
    assert ye[0] == xe[0] == 0 and ye[-1] == y2 - y1 and xe[-1] == x2 - x1 and (np.diff(ye) >= 1).all() and (np.diff(xe) >= 1).all()
    count = np.diff(ye)[:, None] * np.diff(xe)[None, :]
    win = frames[:, y1:y2, x1:x2].astype(np.int64)
    if color:
        total = (np.rint(X.reshape(3, oh, 3, ow).astype(np.float64) * count[None, :, None, :])).sum(axis=(1, 3))
        assert np.array_equal(total, win.sum(axis=(1, 2)))
    else:
        total = np.rint(X.reshape(3, oh, ow).astype(np.float64) * (3 * count)[None]).sum(axis=(1, 2))
        assert np.array_equal(total, win.sum(axis=(1, 2, 3)))
    # every value is float32(float64(sum) / count) of its own box
    r, i = oh // 2, ow // 2
    box = win[:, ye[r]:ye[r + 1], xe[i]:xe[i + 1]]
    if color:
        assert np.array_equal(X.reshape(3, oh, 3, ow)[:, r, :, i], (box.sum(axis=(1, 2)).astype(np.float64) / (box.shape[1] * box.shape[2])).astype(np.float32))
    else:
        assert np.array_equal(X.reshape(3, oh, ow)[:, r, i], (box.sum(axis=(1, 2, 3)).astype(np.float64) / (box.shape[1] * box.shape[2] * 3)).astype(np.float32))


def test_feature_geometry_rules():
    g = F.feature_geometry
    assert g(48, 64, 30)[4:] == (22, 30, 660)              # 48 * 30 / 64 = 22.5: half to even is 22 ...
    assert g(47, 20, 4)[4:] == (9, 4, 36)                  # 9.4
    assert g(35, 20, 2)[4:] == (4, 2, 8)                   # 3.5 -> 4 (to even, upwards)
    assert g(25, 20, 2)[4:] == (2, 2, 4)                   # 2.5 -> 2
    assert g(480, 640, 30, True)[4:] == (22, 30, 1980)     # 22.5 again: a 640 x 480 video
    assert g(1, 64, 4)[4:] == (1, 4, 4)                    # never below one row
    assert g(48, 64, 30, False, (4, 44, 8, 48)) == (4, 44, 8, 48, 30, 30, 900)
    with pytest.raises(ValueError, match="upsamples"):
        g(48, 64, 65)
    with pytest.raises(ValueError, match="upsamples"):
        g(48, 64, 30, False, (0, 29, 0, 48))
    with pytest.raises(ValueError, match="crop"):
        g(48, 64, 30, False, (0, 65, 0, 48))
    with pytest.raises(ValueError, match="limits"):
        g(10, 20000, 30)
    with pytest.raises(ValueError, match="overflow"):
        g(2400, 2400, 1)                                   # 5.76 M pixels x 765 > 2^32 - 1
    assert g(2369, 2369, 1)[4:] == (1, 1, 1)               # 5 612 161 pixels: under the limit of 5 614 429


def test_features_host_values():
    frames = S.frames_for(2, 5, 7)
    # ow == Wc and oh == Hc: every box is one pixel, the grey value its channel mean
    X = F.features_host(frames, 7)
    assert np.array_equal(X.reshape(2, 5, 7), (frames.astype(np.int64).sum(-1).astype(np.float64) / 3).astype(np.float32))
    # colour: [oh, 3, ow], the three planes side by side in every row
    Xc = F.features_host(frames, 7, True).reshape(2, 5, 3, 7)
    for c in range(3):
        assert np.array_equal(Xc[:, :, c, :], frames[..., c].astype(np.float32))
    # crop = (x1, x2, y1, y2) selects frame[y1:y2, x1:x2] first
    big = S.frames_for(2, 33, 21)
    assert np.array_equal(F.features_host(big, 4, True, (3, 20, 1, 30)), F.features_host(np.ascontiguousarray(big[:, 1:30, 3:20]), 4, True))
    assert (F.features_host(np.full((1, 256, 256, 3), 255, np.uint8), 2) == 255.0).all()
    with pytest.raises(ValueError, match="uint8"):
        F.features_host(frames.astype(np.float32), 7)


# ------------------------------------------------------------------------------------------------ kmeans_host
@pytest.mark.parametrize("N,H,W,ow,k", S.PLANTED, ids=lambda v: str(v))
def test_kmeans_host_recovers_a_planted_partition(N, H, W, ow, k):
    X = S.planted_features(N, H, W, ow, k)
    labels, centres, iterations = F.kmeans_host(X, k, S.SEED)
    assert labels.dtype == np.int32 and centres.dtype == np.float32 and centres.shape == (k, X.shape[1]) and 1 <= iterations <= 50
    assert S.same_partition(labels, S.planted(N, H, W, k)[1])
    again = F.kmeans_host(X, k, S.SEED)
    assert np.array_equal(again[0], labels) and np.array_equal(again[1].view(np.uint32), centres.view(np.uint32)) and again[2] == iterations
    # converged: the centres are the means of their members (one fp32 ulp) and every row is nearest to its own
    for c in range(k):
        mean = X[labels == c].astype(np.float64).mean(0)
        assert np.abs(centres[c] - mean).max() <= np.spacing(np.abs(mean).max().astype(np.float32))
    assert np.array_equal(F.assign_host(X, centres)[0], labels)


def test_kmeans_host_empty_clusters_and_duplicate_rows():
    # three distinct rows, five centres: at least two clusters stay empty, and an empty cluster keeps the centre it started with
    rows = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    X = rows[np.arange(40) % 3]
    labels, centres, iterations = F.kmeans_host(X, 5, seed=0)
    assert S.same_partition(labels, np.arange(40) % 3) and iterations <= 3
    used = np.unique(labels)
    assert len(used) == 3
    for c in range(5):
        assert any(np.array_equal(centres[c], r) for r in rows)       # a member mean of identical rows, or the start row itself
    # one distinct row: everything goes to the lowest centre index
    labels, centres, _ = F.kmeans_host(np.ones((9, 4), np.float32), 3, seed=1)
    assert (labels == 0).all() and (centres == 1.0).all()
    # update_host: the empty-cluster rule and the out-of-range count on their own
    X = np.arange(24, dtype=np.float32).reshape(6, 4)
    C0 = np.full((3, 4), -5.0, np.float32)
    C, counts = F.update_host(X, np.array([0, 7, 2, -1, 0, 2], np.int32), C0)
    assert counts.tolist() == [2, 0, 2, 2] and (C[1] == -5.0).all() and C[0].tolist() == [8, 9, 10, 11] and C[2].tolist() == [14, 15, 16, 17]
    with pytest.raises(ValueError, match="160"):
        F.kmeans_host(np.zeros((200, 2), np.float32), 161)


def test_tie_exclusion_cap_of_the_gpu_assign_test():
    """tests/test_frame_selection_gpu.py compares labels only on rows whose float64 gap to the second nearest centre is at least twice
    the fp32 error bound; that this leaves out at most 1 % of the rows is a property of the inputs, shown here on the float64
    reference alone.  The numpy executor's own distances meet the same bound."""
    for N, D, k in S.ASSIGN_SHAPES:
        ref_labels, ref_dist, clear = S.assign_reference(N, D, k)
        assert (~clear).sum() <= 0.01 * N, (N, D, k, int((~clear).sum()))
        X, C = S.assign_case(N, D, k)
        labels, dist = F.assign_host(X, C)
        assert np.array_equal(labels[clear], ref_labels[clear])
        assert (np.abs(dist.astype(np.float64) - ref_dist)[clear] <= S.dist_bound(D) * ref_dist[clear]).all()


def test_center_host_is_the_column_mean():
    X = S.frames_for(1, 30, 23)[0].reshape(30, 69).astype(np.float32)
    centred, mean = F.center_host(X)
    want = X.astype(np.float64).mean(0).astype(np.float32)
    assert np.abs(mean - want).max() <= np.spacing(want).max() and np.array_equal(centred, X - mean[None, :])
    assert F.kmeans_slabs(1) == (1, 1) and F.kmeans_slabs(257) == (2, 129) and F.kmeans_slabs(20000) == (64, 313)
    assert [F.kmeans_chunk(k) for k in (1, 20, 21, 33, 100, 160)] == [512, 512, 448, 256, 64, 64]


# ------------------------------------------------------------------------------------------------ end to end
def make_project(tmp_path, n=120, cropping=False):
    from deepgraphpose_amd.models.eval import export_pose_like_dlc
    H, W = 24, 32
    frames = np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    proj = tmp_path / "proj"
    (proj / "videos").mkdir(parents=True)
    np.save(proj / "videos" / "clip.npy", frames)
    cfg = proj / "config.yaml"
    cfg.write_text("Task: reach\nproject_path: %s\nbodyparts: [hand, elbow]\nnumframes2pick: 4\nstart: 0\nstop: 1\niteration: 2\n"
                   "cropping: %s\nx1: 4\nx2: 30\ny1: 2\ny2: 20\n" % (proj, "true" if cropping else "false"))
    x = np.tile(np.arange(n, dtype=float)[:, None], (1, 2))
    for t in (7, 20, 21, 50, 64, 65, 90, 101, 110):                   # frames the model "got wrong": a jump there and back
        x[t, 0] += 40.0
    labels = {"x": x, "y": np.zeros((n, 2)), "likelihoods": np.full((n, 2), 0.95)}
    export_pose_like_dlc(labels, "snapshot-5", ["hand", "elbow"], str(proj / "videos" / "clip_labeled"))
    return proj, cfg, frames, labels


def test_extract_outlier_frames_end_to_end(tmp_path, capsys):
    import pandas as pd
    from PIL import Image
    proj, cfg, frames, labels = make_project(tmp_path)
    video = str(proj / "videos" / "clip.npy")
    picks = F.extract_outlier_frames(str(cfg), video, backend="host", seed=0, resizewidth=8)
    outliers = F.outlier_indices(labels, "jump", epsilon=20).tolist()
    assert outliers == [7, 8, 20, 22, 50, 51, 64, 66, 90, 91, 101, 102, 110, 111]
    assert 1 <= len(picks) <= 4 and set(picks) <= set(outliers)
    folder = proj / "labeled-data" / "clip"
    names = ["img%03d.png" % i for i in picks]                                          # ceil(log10(120)) = 3 digits
    assert sorted(f for f in os.listdir(folder) if f.endswith(".png")) == sorted(names)
    for i, name in zip(picks, names):
        assert np.array_equal(np.asarray(Image.open(folder / name)), frames[i])
    text = (folder / "machinelabels.csv").read_text().splitlines()
    assert text[0].startswith("scorer,snapshot-5") and text[1].startswith("bodyparts,hand,hand,hand,elbow") and text[2].startswith("coords,x,y,likelihood,x")
    df = pd.read_csv(folder / "machinelabels.csv", header=[0, 1, 2], index_col=0)
    assert list(df.index) == [os.path.join("labeled-data", "clip", n) for n in names]
    assert np.array_equal(df.values[:, 0], labels["x"][picks, 0]) and np.array_equal(df.values[:, 2], labels["likelihoods"][picks, 0])
    assert os.path.exists(folder / "machinelabels-iter2.h5") == _has_pytables()
    out = capsys.readouterr().out
    assert "config.yaml is not rewritten" in out and video in out
    assert cfg.read_text().count("clip") == 0                                           # config.yaml was not touched
    # a second call merges: the rows already there stay first and unchanged, a frame picked again appears once
    before = df.copy()
    tampered = before.copy()
    tampered.iloc[0, 0] = -1.0                                                          # "refined" by hand: must survive the merge
    tampered.to_csv(folder / "machinelabels.csv")
    picks2 = F.extract_outlier_frames(str(cfg), video, backend="host", seed=0, resizewidth=8, outlieralgorithm="jump", epsilon=20)
    assert picks2 == picks                                                              # same seed, same picks: every row is a duplicate
    df2 = pd.read_csv(folder / "machinelabels.csv", header=[0, 1, 2], index_col=0)
    assert list(df2.index) == list(before.index) and df2.iloc[0, 0] == -1.0
    picks3 = F.extract_outlier_frames(str(cfg), video, backend="host", seed=11, extractionalgorithm="uniform")
    df3 = pd.read_csv(folder / "machinelabels.csv", header=[0, 1, 2], index_col=0)
    new = [os.path.join("labeled-data", "clip", "img%03d.png" % i) for i in picks3 if i not in picks]
    assert list(df3.index) == list(before.index) + new and df3.iloc[0, 0] == -1.0 and not df3.index.duplicated().any()


def _has_pytables() -> bool:
    try:
        import tables  # noqa: F401
        return True
    except ImportError:
        return False


def test_extract_frames_with_the_config_crop(tmp_path):
    from PIL import Image
    proj, cfg, frames, _ = make_project(tmp_path, cropping=True)
    video = str(proj / "videos" / "clip.npy")
    picks = F.extract_frames(str(cfg), video, backend="host", seed=3, resizewidth=6)
    assert 1 <= len(picks) <= 4 and F.SELECT_STATS["candidates"] == 120
    folder = proj / "labeled-data" / "clip"
    assert sorted(os.listdir(folder)) == sorted("img%03d.png" % i for i in picks)
    for i in picks:
        assert np.array_equal(np.asarray(Image.open(folder / ("img%03d.png" % i))), frames[i, 2:20, 4:30])
    # the same seed picks the same frames; numframes2pick and the algorithm can be given; crop=False switches the file's crop off
    assert F.extract_frames(str(cfg), video, backend="host", seed=3, resizewidth=6) == picks
    more = F.extract_frames(str(cfg), video, numframes2pick=6, algo="uniform", crop=False, seed=1, start=0.5)
    assert len(more) == 6 and all(60 <= i < 120 for i in more)
    assert np.asarray(Image.open(folder / ("img%03d.png" % more[0]))).shape == (24, 32, 3)
    with pytest.raises(ValueError, match="kmeans | uniform".replace("|", r"\|")):
        F.extract_frames(str(cfg), video, algo="random")
    assert F.image_name(7, 1000) == "img007.png" and F.image_name(7, 1001) == "img0007.png" and F.image_name(123, 100) == "img123.png"


# ------------------------------------------------------------------------------------------------ ABI
def test_selection_symbols_are_declared_and_bound(lib_built):
    from deepgraphpose_amd import _lib, build
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dgp_hip.h")).read()
    for name in ("dgp_frame_features_u8", "dgp_kmeans_scratch_bytes", "dgp_kmeans_center", "dgp_kmeans_assign", "dgp_kmeans_update"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
    assert "dgp_select.hip" in build.SOURCES
    for text in ("DGP_KMEANS_MAX_K = %d" % F.KMEANS_MAX_K, "DGP_KMEANS_MAX_D = %d" % F.KMEANS_MAX_D, "DGP_KMEANS_MAX_SLABS = %d" % F.KMEANS_MAX_SLABS):
        assert text in hdr
    lib = _lib.load()
    assert lib.dgp_kmeans_scratch_bytes(300, 690, 0) == 2 * 690 * 8 and lib.dgp_kmeans_scratch_bytes(300, 690, 20) == 2 * 20 * 690 * 8 + 2 * 21 * 4
    assert lib.dgp_kmeans_scratch_bytes(300, 690, 161) == 0 and lib.dgp_kmeans_scratch_bytes(0, 690, 2) == 0 and lib.dgp_kmeans_scratch_bytes(1, 8193, 2) == 0
