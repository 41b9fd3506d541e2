"""Host side of location refinement in video inference (no GPU): the coordinate composition of 7-lane read-out records
(models/eval.refined_pose), dist.unpack_offsets, and the frame-sharded all-gather of 7-lane records over gloo (world size 2)."""
import os
import socket

import numpy as np
import pytest
import torch

STRIDE, STDEV = 8.0, 7.2801


def _record(row, col, lik, iy, ix, dx, dy):
    r = np.zeros(7, dtype=np.float32)
    r[[0, 1, 2, 5, 6]] = row, col, lik, dx, dy
    r[3:5] = np.array([iy, ix], dtype=np.int32).view(np.float32)
    return r


def test_refined_pose_composes_dlc_geometry_in_both_modes():
    """x takes the column and channel 2j (dx), y the row and channel 2j + 1 (dy); "dgp" records carry the soft-argmax position and the
    window sigmoid, "dlc" records the arg-max cell as floats and its probability -- one composition serves both."""
    from deepgraphpose_amd.models import eval as E
    dgp = _record(2.25, 5.5, 0.75, 2, 6, 0.5, -0.25)
    dlc = _record(3.0, 4.0, 0.9, 3, 4, -1.0, 2.0)
    rec = np.stack([dgp, dlc])[None]                              # [1 frame, 2 joints, 7]
    x, y, lik = E.refined_pose(rec, STRIDE, STDEV)
    assert x.dtype == np.float64 and x.shape == (1, 2)
    np.testing.assert_allclose(x[0], [5.5 * 8 + 4 + 0.5 * STDEV, 4.0 * 8 + 4 - 1.0 * STDEV], rtol=0, atol=1e-12)
    np.testing.assert_allclose(y[0], [2.25 * 8 + 4 - 0.25 * STDEV, 3.0 * 8 + 4 + 2.0 * STDEV], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(lik[0], np.array([0.75, 0.9], dtype=np.float32).astype(np.float64))
    # without an offset the composition is estimate_pose's unrefined one (eval.py:352-353)
    rec0 = rec.copy()
    rec0[..., 5:] = 0
    x0, y0, _ = E.refined_pose(rec0, STRIDE, STDEV)
    np.testing.assert_array_equal(x0, rec[..., 1].astype(np.float64) * STRIDE + 0.5 * STRIDE)
    np.testing.assert_array_equal(y0, rec[..., 0].astype(np.float64) * STRIDE + 0.5 * STRIDE)


def test_refined_pose_applies_the_resize_scale_after_the_offset():
    from deepgraphpose_amd.models import eval as E
    rec = np.stack([_record(1.5, 2.5, 0.5, 1, 2, 0.25, 0.75)])[None]
    x1, y1, _ = E.refined_pose(rec, STRIDE, STDEV)
    x, y, _ = E.refined_pose(rec, STRIDE, STDEV, scale_x=2.0, scale_y=0.5)
    np.testing.assert_array_equal(x, x1 * 2.0)
    np.testing.assert_array_equal(y, y1 * 0.5)
    with pytest.raises(ValueError, match="7"):
        E.refined_pose(rec[..., :5], STRIDE, STDEV)


def test_unpack_offsets_and_keypoints_of_seven_lane_records():
    from deepgraphpose_amd import dist as dd
    rec = torch.from_numpy(np.stack([_record(1, 2, 0.5, 7, 9, 0.125, -3.5), _record(4, 5, 0.25, 1, 0, 2.0, 6.0)])[None])
    offs = dd.unpack_offsets(rec)
    assert offs.shape == (1, 2, 2) and offs.is_contiguous()
    assert offs.tolist() == [[[0.125, -3.5], [2.0, 6.0]]]
    mu, conf, idx = dd.unpack_keypoints(rec)                      # lanes 0..4 keep their meaning
    assert mu.tolist() == [[[1, 2], [4, 5]]] and conf.tolist() == [[0.5, 0.25]] and idx.tolist() == [[[7, 9], [1, 0]]]
    with pytest.raises(ValueError, match="7"):
        dd.unpack_offsets(rec[..., :5])


def test_record_lanes_and_modes():
    from deepgraphpose_amd import engine
    assert engine.record_lanes(None) == 5 and engine.record_lanes("dgp") == 7 and engine.record_lanes("dlc") == 7
    assert engine.LOC_REF_MODES == {"dgp": 1, "dlc": 2}
    with pytest.raises(ValueError):
        engine.record_lanes(True)


def test_estimate_pose_rejects_an_unknown_mode(tmp_path):
    from deepgraphpose_amd.models import eval as E
    with pytest.raises(ValueError, match="loc_ref"):
        E.estimate_pose("none.yaml", "none", "none.npy", str(tmp_path), loc_ref="soft")


# ------------------------------------------------------------------------ 7-lane records through the sharded gather (gloo, world 2)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _records_for(lo, hi, nj):
    fr = torch.arange(lo, hi, dtype=torch.float32)[:, None].expand(-1, nj)
    jj = torch.arange(nj, dtype=torch.float32)[None, :].expand(hi - lo, -1)
    idx = torch.stack([fr, jj], -1).to(torch.int32).contiguous().view(torch.float32)
    return torch.cat([torch.stack([fr + 0.25, fr * 2, fr / 100], -1), idx, torch.stack([fr / 8 - jj, -fr - 0.5], -1)], -1).contiguous()


def _worker(rank, world, port, T, q):
    import torch.distributed as dist
    from deepgraphpose_amd import dist as dd
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dd.init_from_env("gloo")
    lo, hi = dd.shard_range(T, rank, world)
    full = dd.gather_trajectory(_records_for(lo, hi, 3), T)
    q.put((rank, full.numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("T", [10, 7])
def test_seven_lane_records_allgather_gloo_world2(T):
    """gather_trajectory is width-generic: the refined records of two shards (T = 7: a short last shard) arrive frame-ordered and bit
    for bit on both ranks, the int32 lanes and the offsets included."""
    import torch.multiprocessing as mp
    from deepgraphpose_amd import dist as dd
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, T, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _records_for(0, T, 3)
    for rank, full in res:
        assert full.shape == (T, 3, 7)
        assert np.array_equal(full.view(np.int32), want.numpy().view(np.int32)), rank
        offs = dd.unpack_offsets(torch.from_numpy(full))
        np.testing.assert_array_equal(offs[:, 2, 0].numpy(), np.arange(T, dtype=np.float32) / 8 - 2)
        np.testing.assert_array_equal(dd.unpack_keypoints(torch.from_numpy(full))[2][:, 1, 0].numpy(), np.arange(T))
