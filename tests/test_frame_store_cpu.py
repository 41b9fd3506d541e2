"""The torch-free part of the DGP drivers' frame store (models/staging.py: frame_slots, gather_table), the frame_store switch and the
Dataset's batch without pixels -- none of it needs a GPU."""
import contextlib
import io
import os

import numpy as np
import pytest

from deepgraphpose_amd.models import staging


def test_slot_stride_is_the_frame_rounded_up_to_16():
    assert [staging.slot_stride(n) for n in (1, 15, 16, 17, 105, 768, 2079, 2764800)] == [16, 16, 16, 32, 112, 768, 2080, 2764800]


def test_slots_under_a_budget():
    frames, fb = [9, 2, 5, 2, 7], 100                            # unsorted, one twice; a slot costs 112 bytes
    slots, refused = staging.frame_slots(frames, fb, 4 * 112)    # exact fit
    assert slots == {2: 0, 5: 1, 7: 2, 9: 3} and refused == []
    slots, refused = staging.frame_slots(frames, fb, 4 * 112 - 1)            # one frame over: the highest goes
    assert slots == {2: 0, 5: 1, 7: 2} and refused == [9]
    slots, refused = staging.frame_slots(frames, fb, 4 * 100)    # the budget counts the pitch, not the frame
    assert slots == {2: 0, 5: 1, 7: 2} and refused == [9]
    for budget in (0, 111, -5):
        assert staging.frame_slots(frames, fb, budget) == ({}, [2, 5, 7, 9])
    assert staging.frame_slots([], fb, 1000) == ({}, [])
    # the labeled frames give way first, the lower of them last; slots stay in ascending frame order
    slots, refused = staging.frame_slots(frames, fb, 3 * 112, last=[2, 5])
    assert slots == {2: 0, 7: 1, 9: 2} and refused == [5]
    slots, refused = staging.frame_slots(frames, fb, 1 * 112, last=[2, 5])
    assert slots == {7: 0} and refused == [2, 5, 9]
    slots, refused = staging.frame_slots(np.array(frames), fb, 1 << 20, last=np.array([2, 5]))
    assert slots == {2: 0, 5: 1, 7: 2, 9: 3} and refused == []


def test_src_tables():
    slots = {10: 0, 11: 1, 12: 2, 14: 3}
    src, order = staging.gather_table([10, 11, 12, 14], slots)                       # all stored
    assert src.dtype == np.int32 and src.tolist() == [0, 1, 2, 3] and order == []
    src, order = staging.gather_table([10, 11, 12, 14], slots, patched=[1, 3])       # augmented positions
    assert src.tolist() == [0, -1, 2, -2] and order == [1, 3]
    src, order = staging.gather_table([10, 13, 12, 15], slots)                       # frames without a slot
    assert src.tolist() == [0, -1, 2, -2] and order == [1, 3]
    src, order = staging.gather_table([13, 11, 13, 11], slots, patched={1: None})    # repeats: a slot twice, a patch frame each
    assert src.tolist() == [-1, -2, -3, 1] and order == [0, 1, 2]
    src, order = staging.gather_table(np.array([14, 12]), {}, patched=())            # no store
    assert src.tolist() == [-1, -2] and order == [0, 1]
    src, order = staging.gather_table([], slots)
    assert src.shape == (0,) and src.dtype == np.int32 and order == []


def test_resolve_frame_store_and_its_errors():
    from deepgraphpose_amd.models import fitdgp
    assert fitdgp.FRAME_STORES == ("off", "hip")
    assert fitdgp.resolve_frame_store() == "off" and fitdgp.resolve_frame_store("hip") == "hip"
    assert fitdgp.resolve_frame_store("hip", 50, "hip") == "hip" and fitdgp.resolve_frame_store("off", 50, "cv2") == "off"
    assert fitdgp.resolve_frame_store("hip", 0, None) == "hip"
    for bad in ("auto", "host", "on", None):
        with pytest.raises(ValueError, match="frame store"):
            fitdgp.resolve_frame_store(bad)
    with pytest.raises(ValueError, match="needs every frame"):
        fitdgp.resolve_frame_store("hip", 50, "cv2")
    # the drivers refuse before they open the project
    with pytest.raises(ValueError, match="frame store"):
        fitdgp.fit_dgp("snapshot-x", "/nonexistent", frame_store="gpu")
    with pytest.raises(ValueError, match="frame store"):
        fitdgp.fit_dgp_labeledonly("snapshot-x", "/nonexistent", frame_store="gpu")
    with pytest.raises(ValueError, match="needs every frame"):
        fitdgp.fit_dgp("snapshot-x", "/nonexistent", wt=50, flow_backend="cv2", frame_store="hip")
    assert fitdgp.PREP_STATS["frame_store"] is None or isinstance(fitdgp.PREP_STATS["frame_store"], dict)


def test_next_batch_without_pixels_gives_the_same_index_sets_and_labels(tmp_path):
    from scripts import fit_feed_digest as D
    from deepgraphpose_amd.models import fitdgp
    proj = D.bare_project(str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()):
        batcher, _ = fitdgp._setup("snapshot-step0-final--0", proj, 1, 0, None)
        batcher.create_batches_from_resnet_output(0, ns_jump=None, step=1, ns=3, nc=2048, n_max_frames=30)
    d = batcher.datasets[0]
    reads = []
    frame_at = d.video_clip.frame_at
    d.video_clip.frame_at = lambda i: (reads.append(int(i)), frame_at(i))[1]
    pv, ph = np.array([11, 3]), np.array([4, 5, 12])
    full, i0 = batcher.next_batch(0, 0, pv, ph)
    assert sorted(reads) == [3, 4, 5, 11, 12] and full[3].shape == (5, 64, 96, 3)
    del reads[:]
    bare, i1 = batcher.next_batch(0, 0, pv, ph, pixels=False)
    assert reads == [] and bare[3] is None and i0 == i1 == 0
    for k in (0, 1, 2, 4, 5, 6):
        assert np.array_equal(np.asarray(full[k]), np.asarray(bare[k]), equal_nan=True), k
    assert len(full[7]) == len(bare[7]) == 3 and all(np.array_equal(a, b) for a, b in zip(full[7], bare[7]))
    assert np.array_equal(d.load_data([3, 4], [3])[1], d.load_data([3, 4], [3], pixels=False)[1], equal_nan=True)
    assert d.load_data([3, 4], [3], pixels=False)[0] is None


def test_demo_forwards_frame_store_to_steps_1_and_2(monkeypatch, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "demo"))
    import run_dgp_demo as demo
    from deepgraphpose_amd.models import fitdgp, fitdgp_util
    calls = []

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(fitdgp, "fit_dgp_labeledonly", lambda *a, **k: calls.append(("step1", k.get("frame_store"))))
    monkeypatch.setattr(fitdgp, "fit_dgp", lambda *a, **k: calls.append(("step2", k.get("frame_store"))))
    monkeypatch.setattr(fitdgp_util, "get_snapshot_path", stop)               # step 3 is not this test's
    for argv, want in ((["--test"], "off"), (["--test", "--frame_store", "hip"], "hip"), (["--frame_store", "hip"], "hip")):
        del calls[:]
        with pytest.raises(Stop), contextlib.redirect_stdout(io.StringIO()):
            demo.main(["--dlcpath", str(tmp_path), "--dlcsnapshot", "snapshot-step0-final--0"] + argv)
        assert calls == [("step1", want), ("step2", want)]
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        demo.main(["--dlcpath", str(tmp_path), "--frame_store", "host"])
