"""dgp_target_maps (csrc/dgp_targets.hip, engine.target_maps) against the host function it replaces, compute_target_part_scoremap, cast to
fp32: bit for bit.  Every output is pre-filled with NaN, so a cell the kernel does not write shows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STDEV = 7.2801


def _host(entries, offsets, n, H, W, nj, thr, stride=8.0, scale=1.0, present_only=False):
    """the four fp32 maps the host path builds for n frames (dlc_dataset.PoseDataset.host_targets, frame by frame)"""
    from deepgraphpose_amd.dataset import compute_target_part_scoremap
    entries = np.asarray(entries, dtype=np.float64).reshape(-1, 3)
    out = [[], [], [], []]
    for f in range(n):
        e = entries[offsets[f]:offsets[f + 1]]
        ids = e[:, 0].astype(int)
        sc, lmap, lmask = compute_target_part_scoremap([ids], [e[:, 1:3]], (H, W), nj, thr, stride=stride, locref_stdev=STDEV, scale=scale)
        wts = np.ones(sc.shape)
        if present_only:
            wts = np.zeros(sc.shape)
            wts[:, :, ids] = 1.0
        for k, a in enumerate((sc, wts, lmap, lmask)):
            out[k].append(a.astype(np.float32))
    return [np.stack(a) for a in out]


def _device(entries, offsets, n, H, W, nj, thr, stride=8.0, scale=1.0, present_only=False, dgp=False):
    from deepgraphpose_amd import engine
    nan = lambda c: torch.full((n, H, W, c), float("nan"), dtype=torch.float32, device="cuda")
    outs = dict(scmap=None if dgp else nan(nj), weights=None if dgp else nan(nj), lmap=nan(2 * nj), lmask=nan(2 * nj))
    got = engine.target_maps(entries, offsets, n, H, W, nj, pos_dist_thresh=thr, stride=stride, scale=scale, locref_stdev=STDEV,
                             weigh_only_present_joints=present_only, **outs)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in got]


def _check(entries, offsets, n, H, W, nj, thr, hits=True, **kw):
    entries = np.asarray(entries, dtype=np.float64).reshape(-1, 3)
    ref = _host(entries, offsets, n, H, W, nj, thr, **kw)
    assert bool(ref[0].any()) == hits                       # (no case passes on all-zero maps, except the ones meant to)
    for dgp in (False, True):
        got = _device(entries, offsets, n, H, W, nj, thr, dgp=dgp, **kw)
        for k, name in enumerate(("scmap", "weights", "lmap", "lmask")):
            if dgp and k < 2:
                assert got[k] is None
                continue
            assert got[k].shape == ref[k].shape and not np.isnan(got[k]).any(), name
            assert np.array_equal(got[k], ref[k]), (name, int((got[k] != ref[k]).sum()))
    return ref


# 6 x 8 grid, nj = 3, stride 8: (entries, pos_dist_thresh, whether the scoremap has ones)
GRID_CASES = {
    "thr17_window_clamped_at_four_borders": ([(0, 30.0, 20.0), (2, 33.5, 27.25)], 17, True),
    "thr8_joints_in_corner_cells": ([(0, 4.0, 4.0), (1, 60.5, 43.0), (2, 3.0, 44.9)], 8, True),
    "joint_at_minus_200_is_skipped": ([(1, -200.0, 20.0)], 17, False),
    "half_even_2p5_and_3p5": ([(0, 24.0, 20.0), (1, 32.0, 28.0)], 8, True),          # (j_x - 4) / 8 = 2.5 -> 2, 3.5 -> 4
    "centre_exactly_thr_away": ([(0, 12.0, 20.0), (1, 28.0, 12.0)], 8, True),        # dx = 8, dy = 0 and dx = 0, dy = 8: inclusive <=
    "same_joint_twice_last_wins": ([(0, 20.0, 20.0), (1, 50.0, 10.0), (0, 26.0, 22.0)], 17, True),
}


@pytest.mark.parametrize("name", list(GRID_CASES))
@pytest.mark.parametrize("present_only", [False, True])
def test_grid_cases(lib_built, name, present_only):
    entries, thr, hits = GRID_CASES[name]
    ref = _check(entries, [0, len(entries)], 1, 6, 8, 3, thr, hits=hits, present_only=present_only)
    if name == "centre_exactly_thr_away":
        assert ref[0][0, 2, 0, 0] == 1 and ref[0][0, 2, 2, 0] == 1 and ref[0][0, 0, 3, 1] == 1 and ref[0][0, 2, 3, 1] == 1
    if name == "same_joint_twice_last_wins":
        first = _host(entries[:2], [0, 2], 1, 6, 8, 3, thr)
        assert (ref[2] != first[2]).any() and np.array_equal(ref[2][..., 2:4], first[2][..., 2:4])
    if present_only:                                        # 1 in the channels of the frame's entries, skipped or not
        present = sorted({int(e[0]) for e in entries})
        assert all(ref[1][..., j].all() == (j in present) and ref[1][..., j].any() == (j in present) for j in range(3))


@pytest.mark.parametrize("nj,H,W", [(3, 6, 8), (1, 7, 5), (4, 6, 8), (8, 7, 5)])      # nj % 4 == 0: the 16-byte store path
@pytest.mark.parametrize("scale", [1.0, 0.6137])
def test_three_frames_the_middle_one_empty(lib_built, nj, H, W, scale):
    rng = np.random.default_rng(nj * 100 + H)
    k0, k2 = nj, max(1, nj - 1)
    ent = np.column_stack([np.concatenate([rng.permutation(nj)[:k0], rng.permutation(nj)[:k2]]).astype(np.float64),
                           rng.uniform(2, W * 8 - 2, k0 + k2), rng.uniform(2, H * 8 - 2, k0 + k2)])
    off = [0, k0, k0, k0 + k2]
    for present_only in (False, True):
        ref = _check(ent, off, 3, H, W, nj, 17, scale=scale, present_only=present_only)
        assert ref[0][0].any() and ref[0][2].any() and not ref[0][1].any() and not ref[3][1].any()
        assert ref[1][1].any() == (not present_only)


def test_empty_frame_alone_is_all_zero(lib_built):
    ref = _check(np.zeros((0, 3)), [0, 0], 1, 6, 8, 3, 17, hits=False, present_only=True)
    assert not ref[1].any()


def test_every_item_of_the_reaching_mat(lib_built):
    import scipy.io as sio
    mlab = sio.loadmat(os.path.join(HERE, "golden", "Reaching_Mackenzie95shuffle1.mat"))["dataset"]
    ents, off = [], [0]
    for i in range(mlab.shape[1]):
        j = np.asarray(mlab[0, i][2][0][0], dtype=np.float64).reshape(-1, 3)
        ents.append(j)
        off.append(off[-1] + len(j))
    assert len(off) == 53
    ref = _check(np.concatenate(ents), off, 52, 94, 104, 5, 17)
    assert all(r.any() for r in ref[0])


def test_bad_inputs_are_refused_before_the_launch(lib_built):
    from deepgraphpose_amd import _lib, engine
    nan = lambda c: torch.full((2, 6, 8, c), float("nan"), dtype=torch.float32, device="cuda")
    outs = dict(scmap=nan(3), weights=nan(3), lmap=nan(6), lmask=nan(6))
    good = [(0, 20.0, 20.0), (2, 30.0, 30.0)]
    for entries, offsets, what in (([(0, 20.0, 20.0), (3, 30.0, 30.0)], [0, 1, 2], "joint id"),
                                   ([(0, 20.0, 20.0), (-1, 30.0, 30.0)], [0, 1, 2], "joint id"),
                                   (good, [0, 2, 1], "offsets"), (good, [0, 3, 2], "offsets decrease"),
                                   ([(0, float("nan"), 20.0), (1, 30.0, 30.0)], [0, 1, 2], "finite")):
        with pytest.raises(_lib.DgpError, match=what):
            engine.target_maps(entries, offsets, 2, 6, 8, 3, pos_dist_thresh=17, **outs)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all().item() for t in outs.values())              # nothing was launched
    engine.target_maps(good, [0, 1, 2], 2, 6, 8, 3, pos_dist_thresh=17, **outs)
    torch.cuda.synchronize()
    assert not any(torch.isnan(t).any().item() for t in outs.values())
