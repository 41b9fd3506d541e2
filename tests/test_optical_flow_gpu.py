"""HIP Farneback flow (csrc/dgp_flow.hip, engine.optical_flow) against the float64 restatement of its contract (tests/_farneback_ref.py),
its bit-exact properties, and the temporal clique fed from it end to end (dgp_loss_fwd_bwd, fit_dgp without OpenCV)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _farneback_ref as F  # noqa: E402
from test_optical_flow_cpu import REF_PARAMS, interior_epe, texture_pair  # noqa: E402

pytestmark = pytest.mark.gpu
SECOND_PARAMS = dict(pyr_scale=0.5, levels=2, winsize=9, iterations=2, poly_n=7, poly_sigma=1.5)


def _flow(frames, **kw):
    from deepgraphpose_amd import engine
    out = engine.optical_flow(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), output="flow", **kw)
    return out.cpu().numpy()


def _gate(got, ref, what):
    """|d| <= 2e-3 px + 1e-3 |ref| on >= 99.9 % of the components, max |d| <= 0.05 px, mean signed d <= 1e-4 px per component."""
    d = got.astype(np.float64) - ref
    ok = np.abs(d) <= 2e-3 + 1e-3 * np.abs(ref)
    bias = np.abs(d.reshape(-1, 2).mean(0))
    print("%s: within %.5f, max |d| %.3g px, bias (%.2g, %.2g) px, max |flow| %.3g" % (what, ok.mean(), np.abs(d).max(), bias[0],
                                                                                       bias[1], np.abs(ref).max()))
    assert ok.mean() >= 0.999, (what, ok.mean())
    assert np.abs(d).max() <= 0.05, (what, np.abs(d).max(), np.unravel_index(np.abs(d).argmax(), d.shape))
    assert np.all(bias <= 1e-4), (what, bias)


def _sequence(H, W, shifts, seed=0):
    """Frames of one smooth texture moved by the cumulative shifts (frame 0 unmoved)."""
    frames = [texture_pair(H, W, 0.0, 0.0, seed=seed)[0]]
    for dx, dy in np.cumsum(np.asarray(shifts, dtype=np.float64), 0):
        frames.append(texture_pair(H, W, dx, dy, seed=seed)[1])
    return np.stack(frames)


def _warp(img, dx, dy):
    """next(x) = img(x - d), bilinear, replicated borders, rounded back to uint8."""
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    sx, sy = np.clip(xx - dx, 0, W - 1), np.clip(yy - dy, 0, H - 1)
    x0, y0 = np.minimum(np.floor(sx).astype(int), W - 2), np.minimum(np.floor(sy).astype(int), H - 2)
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
    f = img.astype(np.float64)
    out = (f[y0, x0] * (1 - ax) * (1 - ay) + f[y0, x0 + 1] * ax * (1 - ay) + f[y0 + 1, x0] * (1 - ax) * ay
           + f[y0 + 1, x0 + 1] * ax * ay)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def _reaching(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(HERE, "golden", "reaching_frames", name)).convert("RGB"))[..., ::-1].copy()


@pytest.mark.parametrize("case,H,W,params", [
    ("no pyramid, one pass", 64, 96, dict(REF_PARAMS, levels=0, iterations=1)),
    ("one level", 128, 160, dict(REF_PARAMS, levels=1)),
    ("second parameter set", 128, 160, SECOND_PARAMS),
])
def test_flow_matches_restatement_small(lib_built, case, H, W, params):
    fr = _sequence(H, W, [(1.5, -1.0), (-2.0, 0.5)], seed=1)
    _gate(_flow(fr, **params), F.farneback(fr, **params), case)


def test_flow_matches_restatement_reference_parameters_640x480(lib_built):
    # (no zero component: at the last row / column a flow of ~0 px decides step 5's inside / outside branch by its sign alone, so fp32
    # and float64 may take different branches there: a (2, 0) shift measured max 0.0525 px, at row 479, column 98, with 99.93 % within)
    shifts = [(2.0, 0.5), (-1.5, 2.5), (3.5, -4.0)]
    fr = _sequence(480, 640, shifts, seed=2)
    got = _flow(fr, **REF_PARAMS)
    _gate(got, F.farneback(fr, **REF_PARAMS), "640x480 translations")
    for p, (dx, dy) in enumerate(shifts):                                # the translation gate holds on the GPU output too
        assert interior_epe(got[p], dx, dy) <= 0.1, (p, dx, dy)


def test_flow_matches_restatement_real_frames_odd_size(lib_built):
    a = _reaching("img005.png")
    assert a.shape == (747, 832, 3)
    fr = np.stack([a, _warp(a, 1.5, -2.0)])
    got = _flow(fr, **REF_PARAMS)
    _gate(got, F.farneback(fr, **REF_PARAMS), "832x747 warped by (1.5, -2)")
    b = _reaching("img020.png")                                          # two labelled frames, not consecutive: large motion
    fr = np.stack([a, b])
    _gate(_flow(fr, **REF_PARAMS), F.farneback(fr, **REF_PARAMS), "832x747 different frames")


def test_flow_batch_of_eleven_equals_pair_calls(lib_built):
    rng = np.random.default_rng(5)
    shifts = rng.uniform(-3, 3, (10, 2))
    fr = _sequence(64, 96, shifts, seed=4)
    from deepgraphpose_amd import engine
    dev = torch.from_numpy(fr).cuda()
    mag, flow = engine.optical_flow(dev, output="both")
    mag2, flow2 = engine.optical_flow(dev, output="both")
    torch.cuda.synchronize()
    assert mag.shape == (10, 64, 96) and flow.shape == (10, 64, 96, 2)
    assert torch.equal(flow, flow2) and torch.equal(mag, mag2)                       # run to run
    assert torch.equal(mag, flow.abs().sum(-1))                                       # magnitude == |flow|.sum(-1) in fp32
    for p in range(10):                                                                # one call on T frames == T-1 pair calls
        assert torch.equal(engine.optical_flow(dev[p:p + 2], output="flow")[0], flow[p]), p
    assert torch.equal(engine.optical_flow(dev), mag)
    _gate(flow.cpu().numpy(), F.farneback(fr, **REF_PARAMS), "64x96 x 11 frames")


def test_flow_identical_and_uniform_frames(lib_built):
    from deepgraphpose_amd import engine
    flat = torch.full((3, 48, 64, 3), 117, dtype=torch.uint8, device="cuda")
    mag, flow = engine.optical_flow(flat, output="both")
    assert torch.count_nonzero(mag) == 0 and torch.count_nonzero(flow) == 0
    # a textured frame against itself: zero wherever one pass of the box cannot reach the last row / column (see the CPU test)
    fr = texture_pair(64, 96, 0.0, 0.0, seed=3)[0]
    r = REF_PARAMS["winsize"] // 2
    got = _flow(np.stack([fr, fr, fr]), **dict(REF_PARAMS, levels=0, iterations=1))
    assert np.all(got[:, :64 - 1 - r, :96 - 1 - r] == 0.0)
    # with the pyramid the whole field is seeded by those last rows / columns, where a flow of ~0 px picks step 5's branch by its sign
    # (fp32 and float64 can disagree there): no gate against the restatement, only that the field stays a small fraction of a pixel
    got = _flow(np.stack([fr, fr]), **REF_PARAMS)
    assert np.abs(got).max() < 0.5 and np.abs(F.farneback(np.stack([fr, fr]), **REF_PARAMS)).max() < 0.5


def test_flow_edge_cases(lib_built):
    from deepgraphpose_amd import engine, _lib
    one = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device="cuda")
    assert engine.optical_flow(one).shape == (0, 32, 32)
    assert engine.optical_flow(one, output="flow").shape == (0, 32, 32, 2)
    two = torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DgpError):
        engine.optical_flow(two, poly_n=6)
    with pytest.raises(_lib.DgpError):
        engine.optical_flow(two.float())
    with pytest.raises(ValueError):
        engine.optical_flow(two, output="angle")


def test_loss_with_device_vector_field_equals_host_copy(lib_built):
    """dgp_loss_fwd_bwd with vector_field = the device magnitude tensor against the same call with its host copy: the loss kernels
    read bit-identical fields, and losses and gradients agree up to the loss kernels' own run-to-run spread (their gradient sums use
    float atomics, so two calls with the SAME host inputs may differ in the last bits too)."""
    import test_train_gpu as TT
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.loss import dgp_loss_fwd_bwd, dgp_loss_prepare, DGPHyper
    nt, H, W, nj = 6, 12, 16, 3
    rng = np.random.default_rng(7)
    batch, S0 = TT._make_loss_case(rng, nt, H, W, nj, 2, 0.0, 2)
    fr = _sequence(8 * H, 8 * W, rng.uniform(-3, 3, (nt - 1, 2)), seed=8)
    vf = engine.optical_flow(torch.from_numpy(fr).cuda())
    pred = torch.from_numpy((rng.standard_normal((nt, H, W, nj)) * 2).astype(np.float32)).cuda()
    loc = torch.from_numpy(rng.standard_normal((nt, H, W, 2 * nj)).astype(np.float32)).cuda()
    hy = DGPHyper(gm2=1, gm3=3, wt=50.0, wt_max=0.0)
    ws, ws_max = rng.uniform(5, 20, 2), rng.uniform(10, 40, 2)
    out, fields = [], []
    for v in (vf, vf.cpu().numpy(), vf.cpu().numpy()):
        b = dict(batch, vector_field=v, wt_batch_mask=np.array([1, 1, 0, 1, 1], dtype=np.float32))
        li = dgp_loss_prepare(nt, H, W, nj, b, hy, S0, ws, ws_max, 500.0, 37.0, pred.device)
        fields.append(li.vf.clone())
        assert (li.desc.use_wt, li.desc.Hin, li.desc.Win) == (1, 8 * H, 8 * W)
        out.append(dgp_loss_fwd_bwd(pred, loc, b, hy, S0, ws, ws_max, 500.0, 37.0))
    assert torch.equal(fields[0], fields[1]) and fields[0].data_ptr() != fields[1].data_ptr()
    assert fields[0].data_ptr() == vf.data_ptr() or torch.equal(fields[0], vf)
    (l0, dp0, dl0, mu0), (l1, dp1, dl1, mu1), (l2, dp2, dl2, mu2) = out
    assert l0["wt_loss"] > 0
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 1e-6 * max(abs(l1[k]), 1e-6), (k, l0[k], l1[k], l2[k])
    for a, b in ((dp0, dp1), (dl0, dl1), (mu0, mu1)):
        assert (a - b).abs().max() <= 1e-6 * max(float(b.abs().max()), 1e-6)


def test_fit_dgp_temporal_clique_runs_without_opencv(lib_built, tmp_path, monkeypatch):
    """fit_dgp(wt = 50) on a synthetic project with cv2 unavailable: the flow comes from the HIP kernels on the device."""
    import random
    from _project import make_project
    from deepgraphpose_amd.models import fitdgp_util as U
    from deepgraphpose_amd.models.fitdgp import fit_dgp
    from deepgraphpose_amd.models.fitdgp_util import get_snapshot_path
    from deepgraphpose_amd import weights_io
    import builtins
    real_import = builtins.__import__

    def no_cv2(name, *a, **k):
        if name == "cv2" or name.startswith("cv2."):
            raise ImportError("No module named 'cv2'")
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_cv2)
    assert U.resolve_flow_backend("auto") == "hip"
    proj, frames, wts = make_project(tmp_path)
    np.random.seed(0)
    random.seed(0)
    fit_dgp("snapshot-step0-final--0", proj, batch_size=4, shuffle=1, step=2, maxiters=3, displayiters=1, wt=50, aug=False,
            n_max_frames=30, ns=3)
    snap, _ = get_snapshot_path("snapshot-step2-final--0", proj, shuffle=1)
    assert os.path.isfile(snap + ".index")
    w = weights_io.load_weights(snap)
    assert all(np.isfinite(v).all() for v in w.values())
    assert any(np.abs(w[k] - wts[k]).max() > 0 for k in wts if k in w)
