"""coord2map_entries (dataset.py): the entries and offsets handed to engine.target_maps are coord2map's own inputs to the host target
generator -- run through that generator they give coord2map's maps."""
import numpy as np
import pytest


def _through_host(entries, offsets, H, W, nj, thr, stdev):
    from deepgraphpose_amd.dataset import compute_target_part_scoremap
    t, m = [], []
    for f in range(len(offsets) - 1):
        e = entries[offsets[f]:offsets[f + 1]]
        _, lt, lm = compute_target_part_scoremap([e[:, 0].astype(int)], [e[:, 1:3]], (H, W), nj, thr, 8.0, stdev, 1.0)
        t.append(lt)
        m.append(lm)
    return np.array(t), np.array(m)


@pytest.mark.parametrize("nv", [1, 3])
def test_coord2map_entries_are_coord2maps_inputs(nv):
    from deepgraphpose_amd.dataset import coord2map, coord2map_entries
    nj, H, W = 4, 12, 16
    rng = np.random.default_rng(nv)
    jl = np.stack([rng.uniform(1, H - 2, (nv, nj)), rng.uniform(1, W - 2, (nv, nj))], -1)
    jl[0, 1] = np.nan                               # unlabeled
    jl[nv - 1, 2] = (-0.5, -0.5)                    # * 8 + 4 = (0, 0): dropped by the sum-is-zero rule
    ent, off = coord2map_entries(jl, nj)
    assert ent.dtype == np.float64 and ent.shape[1] == 3 and off.dtype == np.int32 and off.shape == (nv + 1,)
    assert off[0] == 0 and off[-1] == ent.shape[0] == nv * nj - 2
    first = ent[off[0]:off[1], 0].astype(int).tolist()
    assert 1 not in first and (2 not in ent[off[nv - 1]:off[nv], 0].astype(int).tolist())
    # (x, y) = flip(row, col) * 8 + 4
    assert np.array_equal(ent[0, 1:], np.flip(jl[0, 0] * 8 + 4))
    t, m = _through_host(ent, off, H, W, nj, 17, 7.2801)
    rt, rm = coord2map(jl, H, W, nj, 17, 7.2801)
    assert np.array_equal(t, rt) and np.array_equal(m, rm) and rm.any()


def test_coord2map_entries_checks_its_shape():
    from deepgraphpose_amd.dataset import coord2map_entries
    ent, off = coord2map_entries(np.zeros((0, 3, 2)), 3)
    assert ent.shape == (0, 3) and off.tolist() == [0]
    with pytest.raises(ValueError, match="joint_loc"):
        coord2map_entries(np.zeros((2, 4, 2)), 3)
