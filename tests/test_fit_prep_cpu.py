"""The fit drivers' sample preparation without a GPU: PoseDataset.plan_batch (the draws apart from the pixels), plan_entries, and the
BOX / BILINEAR coefficient tables of dgp_resize_plan_f against Pillow."""
import numpy as np
import pytest

import _fit_prep as P
import _pil_resample_ref as R

SEED = 3          # 40 samples of this seed hold at least five cropped and five uncropped ones (asserted below)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """40 seeded samples of the Reaching project, once rendered by next_batch (make_batch) and once planned by plan_batch"""
    cfg = P.reaching_cfg(tmp_path_factory.mktemp("reaching"))
    ds = P.seeded_dataset(cfg, SEED)
    batches = [ds.next_batch() for _ in range(40)]
    end_render = P.rng_state()
    ds = P.seeded_dataset(cfg, SEED)
    plans = [ds.plan_batch() for _ in range(40)]
    end_plan = P.rng_state()
    ds = P.seeded_dataset(cfg, SEED)
    for _ in range(40):
        ds.skip_batch()
    return dict(cfg=cfg, ds=ds, batches=batches, plans=plans, states=(end_render, end_plan, P.rng_state()))


def test_plan_batch_draws_what_next_batch_draws(walk):
    from PIL import Image
    ncrop = 0
    for b, p in zip(walk["batches"], walk["plans"]):
        assert p.item.im_path == b["data_item"].im_path and p.mirror is False
        assert 0.75 * 0.8 <= p.scale <= 1.25 * 0.8
        assert tuple(b["inputs"].shape[1:3]) == tuple(p.out_hw)
        assert tuple(b["part_score_targets"].shape[1:3]) == tuple(int(v) for v in p.sm_size)
        rows, cols = int(p.item.im_size[1]), int(p.item.im_size[2])
        if p.crop is not None:
            ncrop += 1
            x0, y0, x1, y1 = p.crop
            assert 0 <= x0 <= x1 < cols and 0 <= y0 <= y1 < rows and p.in_hw == (y1 - y0 + 1, x1 - x0 + 1)
        else:
            assert p.in_hw == (rows, cols)
        # the window and the scale are the ones make_batch used: the same pixels come out of them
        with Image.open(walk["cfg"].project_path + "/" + p.item.im_path) as im:
            full = np.asarray(im.convert("RGB"))
        assert full.shape[:2] == (rows, cols)
        assert np.array_equal(walk["ds"].host_pixels(p, full)[None], b["inputs"])
    assert ncrop >= 5 and len(walk["plans"]) - ncrop >= 5


def test_plan_entries_reproduce_make_batchs_maps(walk):
    from deepgraphpose_amd.dataset import compute_target_part_scoremap
    from deepgraphpose_amd.dlc_dataset import plan_entries
    cfg = walk["cfg"]
    for b, p in zip(walk["batches"], walk["plans"]):
        ent = plan_entries(p)
        assert ent.dtype == np.float64 and ent.shape == (sum(len(i) for i in p.joint_ids), 3)
        assert np.array_equal(ent[:, 0], np.concatenate(p.joint_ids)) and np.array_equal(ent[:, 1:], np.concatenate(p.coords))
        sc, lmap, lmask = compute_target_part_scoremap([ent[:, 0].astype(int)], [ent[:, 1:3]], p.sm_size, cfg.num_joints, cfg.pos_dist_thresh,
                                                       stride=cfg.stride, locref_stdev=cfg.locref_stdev, scale=p.scale)
        assert np.array_equal(sc[None].astype(np.float32), b["part_score_targets"])
        assert np.array_equal(lmap[None].astype(np.float32), b["locref_targets"])
        assert np.array_equal(lmask[None].astype(np.float32), b["locref_mask"])
        assert np.array_equal(np.ones_like(b["part_score_targets"]), b["part_score_weights"])
        assert b["part_score_targets"].any()
        host = walk["ds"].host_targets(p)
        assert all(np.array_equal(host[k], b[k]) for k in P.MAP_KEYS)


def test_plan_and_skip_walks_leave_the_generators_where_next_batch_does(walk):
    rendered, planned, skipped = walk["states"]
    assert rendered == planned == skipped


def test_present_joint_weights_and_mirror_go_through_the_plan(tmp_path):
    """weigh_only_present_joints and mirror (symmetric pair 0 <-> 1): next_batch == render of the plan, entries carry the swapped ids"""
    from deepgraphpose_amd.dlc_dataset import plan_entries
    cfg = P.reaching_cfg(tmp_path, weigh_only_present_joints=True, mirror=True, all_joints=[[0, 1], [2], [3], [4]])
    ds = P.seeded_dataset(cfg, 1)
    batches = [ds.next_batch() for _ in range(6)]
    ds = P.seeded_dataset(cfg, 1)
    plans = [ds.plan_batch() for _ in range(6)]
    assert any(p.mirror for p in plans) and not all(p.mirror for p in plans)
    for b, p in zip(batches, plans):
        again = ds.render_batch(p)
        assert np.array_equal(again["inputs"], b["inputs"]) and all(np.array_equal(again[k], b[k]) for k in P.MAP_KEYS)
        present = np.zeros(5)
        present[plan_entries(p)[:, 0].astype(int)] = 1
        assert np.array_equal(b["part_score_weights"][0, 0, 0], present)


@pytest.mark.parametrize("n_in,n_out", [(53, 32), (53, 40), (37, 37), (5, 1), (40, 50), (7, 9)])
def test_box_and_bilinear_tables_give_pillows_bytes(lib_built, n_in, n_out):
    from PIL import Image
    from deepgraphpose_amd import engine
    img = R.test_image(n_in + 4, n_in, seed=n_out)              # rows n_in + 4 -> n_out + 3, columns n_in -> n_out
    oh = n_out + 3
    for name, pil in (("box", Image.BOX), ("bilinear", Image.BILINEAR)):
        got = P.resize_with(img, oh, n_out, lambda a, b: engine.resize_plan_f(a, b, name))
        ref = np.asarray(Image.fromarray(img).resize((n_out, oh), pil))
        assert np.array_equal(got, ref), name
    ks, b, c = engine.resize_plan_f(n_in, n_out, "box")
    assert ks == int(np.ceil(0.5 * max(n_in / n_out, 1.0))) * 2 + 1 and (c.sum(1) > 0).all() and (b[:, 0] + b[:, 1] <= n_in).all()


@pytest.mark.parametrize("n_in,n_out", [(53, 32), (37, 37), (5, 1), (40, 50), (131, 96)])
def test_bicubic_through_the_filter_entry_is_the_existing_plan(lib_built, n_in, n_out):
    from deepgraphpose_amd import _lib, engine
    old, new = engine.resize_plan(n_in, n_out), engine.resize_plan_f(n_in, n_out, "bicubic")
    assert old[0] == new[0] and np.array_equal(old[1], new[1]) and np.array_equal(old[2], new[2])
    with pytest.raises(_lib.DgpError, match="filter"):
        import ctypes as C
        ks = C.c_int32()
        _lib.check(_lib.load().dgp_resize_plan_size_f(n_in, n_out, 1, C.byref(ks)), "dgp_resize_plan_size_f")
