"""Location refinement through the network-level entries: dgp_infer_packed_locref (engine.DGPNet.infer_packed(loc_ref=)), DGPPipeline and
estimate_pose(loc_ref=).  ResNet-50, 3 joints, 64 x 96 frames, batch 2, synthetic weights with the locref head.

Self-consistency (bit for bit, both tiers): the fused entry equals forward(want_locref=True) followed by the layer-level read-out.
Accuracy (parity tier): the project's float64-anchored criterion on the refined coordinate, against oracle.dgp_oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PX_TOL = 1e-3          # px
STRIDE, STDEV = 8.0, 7.2801
NJ, H, W, B = 3, 64, 96, 2


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


@pytest.fixture(scope="module")
def wts():
    from deepgraphpose_amd.synthetic import make_weights
    return make_weights(50, NJ, True, seed=41, head_std=0.05)


@pytest.fixture(scope="module")
def frames():
    from deepgraphpose_amd.synthetic import make_frames
    return make_frames(3 * B, H, W, NJ, seed=42)


def _net(eng, wts, tier=None, max_batch=B):
    net = eng.DGPNet(50, NJ, H, W, max_batch=max_batch, with_locref=True, tier=tier)
    net.load_weights(wts)
    return net


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _records(mu, conf, idx, offs):
    """the 7-lane record the read-out writes, assembled from the dense outputs"""
    return torch.cat([mu, conf.unsqueeze(-1), idx.contiguous().view(torch.float32), offs], dim=-1).contiguous()


@pytest.mark.parametrize("tier", ["parity", "f16"])
def test_infer_packed_locref_equals_forward_plus_readout(eng, wts, frames, tier):
    """Both modes, both tiers: the fused entry (heads into the workspace, one read-out launch into 7-lane records) equals the dense
    forward followed by soft_argmax_locref / hard_argmax, bit for bit; it also hands out the maps it read on request."""
    net = _net(eng, wts, tier)
    ft = torch.from_numpy(frames[:B]).cuda()
    scm, loc = net.forward(ft, want_locref=True)
    mu, conf, idx, offs = eng.soft_argmax_locref(scm, loc, 1.0, 1)
    got = net.infer_packed(ft, torch.zeros((B, NJ, 7), dtype=torch.float32, device="cuda"), 1.0, 1, loc_ref="dgp")
    assert torch.equal(_bits(got), _bits(_records(mu, conf, idx, offs)))
    hidx, prob, hoffs = eng.hard_argmax(scm, loc)
    scm_out, loc_out = torch.zeros_like(scm), torch.zeros_like(loc)
    got = net.infer_packed(ft, torch.zeros((B, NJ, 7), dtype=torch.float32, device="cuda"), 1.0, 1, scmap_out=scm_out, loc_ref="dlc",
                           locref_out=loc_out)
    assert torch.equal(_bits(got), _bits(_records(hidx.to(torch.float32), prob, hidx, hoffs)))
    assert torch.equal(_bits(scm_out), _bits(scm)) and torch.equal(_bits(loc_out), _bits(loc))
    assert net.range_status() == (False, 1)


def test_refined_record_keeps_the_plain_record_and_the_calibration(eng, wts, frames):
    """Lanes 0..4 of the "dgp" record are infer_packed's plain record, bit for bit; the heads own no activation scale, so a net
    calibrated through the plain entry is not calibrated again by the refined one.  Wrong record widths and modes are refused."""
    from deepgraphpose_amd import _lib, dist as dd
    net = _net(eng, wts)
    ft = torch.from_numpy(frames[:B]).cuda()
    plain = net.infer_packed(ft, torch.zeros((B, NJ, 5), dtype=torch.float32, device="cuda"), 1.0, 1)
    ref = net.infer_packed(ft, torch.zeros((B, NJ, 7), dtype=torch.float32, device="cuda"), 1.0, 1, loc_ref="dgp")
    assert net.range_status() == (False, 1)
    assert torch.equal(_bits(ref[..., :5]), _bits(plain))
    assert torch.isfinite(dd.unpack_offsets(ref)).all() and dd.unpack_offsets(ref).abs().max() > 0
    with pytest.raises(_lib.DgpError, match="traj must be"):
        net.infer_packed(ft, plain, 1.0, 1, loc_ref="dgp")
    with pytest.raises(_lib.DgpError, match="traj must be"):
        net.infer_packed(ft, ref, 1.0, 1)
    with pytest.raises(ValueError):
        net.infer_packed(ft, ref, 1.0, 1, loc_ref="hard")
    for gl in (0, 8):
        with pytest.raises(_lib.DgpError, match="gauss_len must be 1..7"):
            net.infer_packed(ft, ref, 1.0, gl, loc_ref="dgp")


def test_net_without_the_locref_head_is_refused(eng, frames):
    from deepgraphpose_amd import _lib
    from deepgraphpose_amd.synthetic import make_weights
    net = eng.DGPNet(50, NJ, H, W, max_batch=B)
    net.load_weights(make_weights(50, NJ, False, seed=41, head_std=0.05))
    ft = torch.from_numpy(frames[:B]).cuda()
    with pytest.raises(_lib.DgpError, match="net built without locref head"):
        net.infer_packed(ft, torch.zeros((B, NJ, 7), dtype=torch.float32, device="cuda"), 1.0, 1, loc_ref="dgp")


def _expected_offsets(pmap, locref, dtype=np.float64):
    b, h, w, c = pmap.shape
    return (pmap.astype(dtype)[..., None] * locref.reshape(b, h, w, c, 2).astype(dtype)).sum(axis=(1, 2), dtype=dtype)


def _refined_px(mu, offs):
    return np.asarray(mu, np.float64) * STRIDE + 0.5 * STRIDE + np.asarray(offs, np.float64) * STDEV


def test_refined_coordinate_against_the_float64_anchor(eng, wts, frames):
    """Parity tier, the float64-anchored criterion on the refined coordinate mu * 8 + 4 + offs * 7.2801:
    err(HIP) <= max(1e-3 px, 1.5 x err(fp32 oracle)), both against resnet_features -> pose_heads(with_locref) -> read-out in float64.
    Measured on an MI355X: HIP 2.13e-5 px, the fp32 oracle 2.97e-5 px from float64 (the line this test prints; EXPERIMENTS.md quotes it)."""
    from oracle import dgp_oracle as O
    fr = frames[:B]
    ref = {}
    for dt in (np.float32, np.float64):
        feats = O.resnet_features(fr, wts, 50, dtype=dt)
        scm, loc = O.pose_heads(feats, wts, True)
        mu, pm = O.argmax_2d_from_cm(scm, 1.0, 1, dtype=dt)
        ref[dt] = _refined_px(mu, _expected_offsets(pm, loc, dt))
    err_oracle = np.abs(ref[np.float32] - ref[np.float64]).max()
    net = _net(eng, wts, "parity")
    rec = net.infer_packed(torch.from_numpy(fr).cuda(), torch.zeros((B, NJ, 7), dtype=torch.float32, device="cuda"), 1.0, 1,
                           loc_ref="dgp").cpu().numpy()
    err = np.abs(_refined_px(rec[..., 0:2], rec[..., 5:7]) - ref[np.float64]).max()
    print("refined coordinate vs float64: HIP %.3g px, fp32 oracle %.3g px" % (err, err_oracle))
    assert err <= max(PX_TOL, 1.5 * err_oracle)


def test_pipeline_with_location_refinement_equals_one_engine(eng, wts, frames):
    """Two engines, three batches, loc_ref="dgp": which engine a batch lands on does not change a bit of its 7-lane records."""
    ft = torch.from_numpy(frames).cuda()
    one = _net(eng, wts)
    ref = torch.zeros((3 * B, NJ, 7), dtype=torch.float32, device="cuda")
    for s in range(0, 3 * B, B):
        one.infer_packed(ft[s:s + B].contiguous(), ref[s:s + B], 1.0, 1, loc_ref="dgp")
    assert one.range_status() == (False, 1)
    pipe = eng.DGPPipeline(50, NJ, H, W, max_batch=B, with_locref=True, n_streams=2)
    pipe.load_weights(wts)
    got = torch.zeros_like(ref)
    for s in range(0, 3 * B, B):
        pipe.submit(ft[s:s + B].contiguous(), got[s:s + B], 1.0, 1, loc_ref="dgp")
    pipe.join()
    torch.cuda.synchronize()
    assert pipe.range_status() == (False, 1) and [n.range_status()[1] for n in pipe.nets] == [1, 1]
    assert torch.equal(_bits(got), _bits(ref))


# ---------------------------------------------------------------------------- estimate_pose on a tiny project
def _tiny_project(tmp_path, with_locref, T=11):
    import yaml
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    parts = ["a", "b", "c"]
    proj = tmp_path / ("proj_locref" if with_locref else "proj_plain")
    train = proj / "dlc-models" / "iteration-0" / "DemoOct2-trainset95shuffle1" / "train"
    train.mkdir(parents=True)
    (proj / "config.yaml").write_text(yaml.safe_dump(dict(Task="Demo", date="Oct2", iteration=0, TrainingFraction=[0.95],
                                                          bodyparts=parts, skeleton=[], project_path=str(proj))))
    (train / "pose_cfg.yaml").write_text(yaml.safe_dump(dict(num_joints=NJ, all_joints_names=parts, net_type="resnet_50")))
    wts = make_weights(50, NJ, with_locref, seed=9, head_std=0.05)
    snap = weights_io.save_weights(str(train / "snapshot-step2-final--0"), wts)
    frames = make_frames(T, H, W, NJ, seed=5)
    clip = tmp_path / "clip.npy"
    if not clip.exists():
        np.save(clip, frames)
    return proj, snap, frames, wts


def test_estimate_pose_with_location_refinement(eng, tmp_path):
    """estimate_pose(loc_ref="dgp" | "dlc") on an 11-frame clip, batches of 4: x, y are refined_pose's composition of the engine-level
    records (same calibration batch: the video's first), the likelihood is the window sigmoid / the arg-max probability, the csv has
    the DLC header; loc_ref=None on the same project gives today's output."""
    from deepgraphpose_amd.models import eval as E
    proj, snap, frames, wts = _tiny_project(tmp_path, True)
    cfg, clip = str(proj / "config.yaml"), str(tmp_path / "clip.npy")
    T, bs = frames.shape[0], 4
    ft = torch.from_numpy(frames).cuda()
    net = _net(eng, wts, max_batch=bs)
    want = {}
    for mode in ("dgp", "dlc", None):
        lanes = 5 if mode is None else 7
        rec = torch.zeros((T, NJ, lanes), dtype=torch.float32, device="cuda")
        net.reset_scales()
        for s in range(0, T, bs):
            net.infer_packed(ft[s:s + bs].contiguous(), rec[s:s + bs], 1, 1, loc_ref=mode)
        assert not net.range_status()[0]
        want[mode] = rec.cpu().numpy()
    for mode in ("dgp", "dlc"):
        out = E.estimate_pose(cfg, snap, clip, str(tmp_path / ("pred_" + mode)), shuffle=1, batch_size=bs, loc_ref=mode)
        assert E.RUN_STATS["loc_ref"] == mode and E.RUN_STATS["chunk_reruns"] == 0
        x, y, lik = E.refined_pose(want[mode], STRIDE, STDEV)
        assert np.array_equal(out["x"], x) and np.array_equal(out["y"], y) and np.array_equal(out["likelihoods"], lik)
        r = want[mode].astype(np.float64)
        assert np.array_equal(out["x"], r[..., 1] * STRIDE + 0.5 * STRIDE + r[..., 5] * STDEV)      # x: column + dx
        assert np.array_equal(out["y"], r[..., 0] * STRIDE + 0.5 * STRIDE + r[..., 6] * STDEV)      # y: row + dy
        lines = (tmp_path / ("pred_" + mode) / "clip_labeled.csv").read_text().splitlines()
        assert lines[0].startswith("scorer,") and lines[1] == "bodyparts,a,a,a,b,b,b,c,c,c"
        assert lines[2] == "coords," + ",".join(["x", "y", "likelihood"] * NJ) and len(lines) == 3 + T
        back = E.load_pose_from_dlc_to_dict(str(tmp_path / ("pred_" + mode) / "clip_labeled.csv"))
        np.testing.assert_allclose(back["x"], out["x"], rtol=1e-12)
    # "dlc": cell coordinates are integers, the likelihood is the arg-max probability (not the window's)
    assert np.array_equal(want["dlc"][..., 0], np.round(want["dlc"][..., 0]))
    assert not np.array_equal(want["dlc"][..., 2], want["dgp"][..., 2])
    # the default path: the plain 5-lane records, composed as before
    out = E.estimate_pose(cfg, snap, clip, str(tmp_path / "pred_none"), shuffle=1, batch_size=bs)
    assert E.RUN_STATS["loc_ref"] is None
    m = want[None].astype(np.float64)
    assert np.array_equal(out["x"], m[..., 1] * STRIDE + 0.5 * STRIDE) and np.array_equal(out["y"], m[..., 0] * STRIDE + 0.5 * STRIDE)
    assert np.array_equal(out["likelihoods"], m[..., 2])
    assert np.array_equal(m[..., :5], want["dgp"].astype(np.float64)[..., :5])
    E.clear_session_cache()


def test_estimate_pose_names_the_missing_locref_variable(eng, tmp_path):
    """A snapshot trained without location refinement: KeyError naming pose/locref_pred, not a fall-through to ResNet-101 (whose
    KeyError would speak of resnet_v1_101 variables)."""
    from deepgraphpose_amd.models import eval as E
    proj, snap, frames, wts = _tiny_project(tmp_path, False)
    with pytest.raises(KeyError, match="pose/locref_pred/block4/weights"):
        E.estimate_pose(str(proj / "config.yaml"), snap, str(tmp_path / "clip.npy"), str(tmp_path / "pred"), shuffle=1, batch_size=4,
                        loc_ref="dgp")
    E.clear_session_cache()
