"""GPU tests of the loss kernels at the edges typical random data never reaches: the DGP loss (loss_normalisers, loss_ce_backward,
loss_locref_backward through dgp_loss_fwd_bwd) and the DLC loss (dlc_loss_reduce / dlc_loss_backward through dgp_dlc_loss_fwd_bwd)
against the float64 autograd oracle (oracle/dgp_train_oracle.py) with the tolerances of tests/test_train_gpu.py, and TF's closed
forms (tests/_tf_kat.py) fed through the DLC kernels."""
import numpy as np
import pytest
import torch

from test_train_gpu import _make_loss_case

pytestmark = pytest.mark.gpu


def _cfg(hy, nj, S0, ws, ws_max, n_tot=500.0, n_vis=37.0):
    return dict(nj=nj, S0=S0, ws=ws, ws_max=ws_max, stride=8.0, gamma=hy.gamma, gauss_len=hy.gauss_len, lengthscale=hy.lengthscale,
                gm2=hy.gm2, gm3=hy.gm3, wn_visible=hy.wn_visible, wn_hidden=hy.wn_hidden, locref_loss_weight=hy.locref_loss_weight,
                locref_huber_loss=hy.locref_huber_loss, n_frames_total=n_tot, n_visible_frames_total=n_vis)


def _peaks(rng, nt, H, W, nj, amp=6.0):
    pred = (rng.standard_normal((nt, H, W, nj)) * 2).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for n in range(nt):
        for j in range(nj):
            cy, cx = rng.uniform(0, H - 1), rng.uniform(0, W - 1)
            pred[n, :, :, j] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 6.0)
    return pred


def _case(rng, nt, H, W, nj, nvf, nan_frac=0.2, gm2=0, gm3=0, huber=True):
    from deepgraphpose_amd.loss import DGPHyper
    nl = 2 if nj > 2 else (1 if nj == 2 else 0)
    batch, S0 = _make_loss_case(rng, nt, H, W, nj, nvf, nan_frac, nl)
    pred = _peaks(rng, nt, H, W, nj)
    loc = rng.standard_normal((nt, H, W, 2 * nj)).astype(np.float32)
    hy = DGPHyper(gm2=gm2, gm3=gm3, locref_huber_loss=huber)
    ws, ws_max = rng.uniform(5, 20, nl), rng.uniform(10, 40, nl)
    return batch, S0, pred, loc, hy, ws, ws_max


def _check_dgp(batch, S0, pred, loc, hy, ws, ws_max, oracle_dtype=torch.float64):
    """kernels vs the autograd oracle in oracle_dtype, with test_loss_forward_backward_matches_autograd's tolerances -> kernel outputs"""
    from deepgraphpose_amd.loss import dgp_loss_fwd_bwd
    from oracle import dgp_train_oracle as T
    nj = pred.shape[-1]
    pt = torch.tensor(pred, dtype=oracle_dtype, requires_grad=True)
    lt = torch.tensor(loc, dtype=oracle_dtype, requires_grad=True)
    L = T.dgp_loss(pt, lt, batch, _cfg(hy, nj, S0, ws, ws_max))
    L["total_loss"].backward()
    losses, dpred, dloc, mu = dgp_loss_fwd_bwd(torch.from_numpy(pred).cuda(), torch.from_numpy(loc).cuda(), batch, hy, S0, ws, ws_max,
                                               500.0, 37.0)
    dpred, dloc = dpred.cpu().numpy(), dloc.cpu().numpy()
    for k in ("visible_loss_pred", "hidden_loss_pred", "visible_loss_locref", "total_loss", "total_loss_visible"):
        ref = float(L[k].detach())
        assert np.isfinite(losses[k]) and abs(losses[k] - ref) <= 2e-5 * max(1.0, abs(ref)), (k, losses[k], ref)
    if S0.shape[0]:
        ref = float(L["ws_loss"].detach())
        assert abs(losses["ws_loss"] - ref) <= 2e-5 * max(1.0, abs(ref))
    np.testing.assert_allclose(mu.cpu().numpy(), L["_mu"].detach().numpy(), atol=2e-5)
    gp = pt.grad.numpy()
    gl = lt.grad.numpy() if lt.grad is not None else np.zeros_like(loc)
    assert np.isfinite(dpred).all() and np.isfinite(dloc).all()
    assert np.abs(dpred - gp).max() <= 2e-4 * (np.abs(gp).max() + 1e-12) + 1e-9
    assert np.abs(dloc - gl).max() <= 2e-5 * (np.abs(gl).max() + 1e-12) + 1e-10
    return losses, dpred, dloc, L


# ---------------------------------------------------------------------------------------------------------------------- DGP loss
@pytest.mark.parametrize("gm2,gm3", [(0, 0), (1, 3), (2, 3)])
@pytest.mark.parametrize("shape", [(5, 12, 16, 3, 2), (3, 136, 240, 4, 1)], ids=["lds", "streaming"])
def test_locref_squared_error_branch(lib_built, gm2, gm3, shape):
    """locref_huber_loss=False (pose_cfg): el = d^2, de = 2 d in loss_locref_backward, on a map the CE kernel keeps in LDS and on one
    it streams (136 x 240)."""
    nt, H, W, nj, nvf = shape
    rng = np.random.default_rng(H + 10 * gm2 + gm3)
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, nvf, gm2=gm2, gm3=gm3, huber=False)
    loc *= 2.0                          # residuals beyond 1 too: where Huber and squared error part
    _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)


@pytest.mark.parametrize("huber", [True, False])
def test_locref_residuals_on_the_huber_boundary(lib_built, huber):
    """Residuals at exactly |d| = 1, 1 -+ 1 ulp, 0 and a few beyond, with the target map 0 (so the kernel's fp32 pred - map is exactly
    the intended d) and the mask 1 everywhere: the value and the gradient of each branch where they meet."""
    rng = np.random.default_rng(21)
    nt, H, W, nj = 2, 12, 16, 3
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, nt, nan_frac=0.0, huber=huber)
    batch["locref_map"] = np.zeros((nt, H, W, 2 * nj))
    batch["locref_mask"] = np.ones((nt, H, W, 2 * nj))
    one = np.float32(1.0)
    vals = np.array([1.0, -1.0, np.nextafter(one, 0), np.nextafter(one, 2), -np.nextafter(one, 0), -np.nextafter(one, 2), 0.0, -0.0,
                     0.5, 2.0, -3.0], np.float32)
    loc = np.resize(vals, loc.shape).astype(np.float32)
    losses, _, dloc, _ = _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)
    # by hand: the mask is all ones, so every element weighs locref_loss_weight / (nt H W 2 nj)
    d = loc.astype(np.float64)
    el = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5) if huber else d * d
    assert abs(losses["visible_loss_locref"] - hy.locref_loss_weight * el.mean()) <= 1e-6 * hy.locref_loss_weight * el.mean()
    de = np.clip(d, -1, 1) if huber else 2 * d
    np.testing.assert_allclose(dloc, hy.locref_loss_weight * de / d.size, rtol=1e-6, atol=0)


def _saturate(rng, pred, batch, which, peak):
    """one cell of each hidden marker in `which` (indices into hidden_marker) set to `peak`: -> the markers"""
    nt, H, W, nj = pred.shape
    hm = np.asarray(batch["hidden_marker"])[which]
    for m in hm:
        pred[m // nj, rng.integers(H), rng.integers(W), m % nj] = peak
    return hm


@pytest.mark.parametrize("gm2", [1, 2])
@pytest.mark.parametrize("how", ["one", "all"])
def test_saturated_hidden_markers(lib_built, gm2, how):
    """gm3 = 3 with peaks of 45: sigmoid is exactly 1 there in fp32 AND fp64, so c = 1, the marker's weight 1 - c is 0 and
    loss_normalisers must not count it (1 - c != 0), and 1 / (1 - s + 1e-20) is 1e20 in fp32.  One of several hidden markers saturated,
    and all of them: then the normaliser's count is 0 and hidden_loss_pred is exactly 0.  Everything finite, against the fp64 oracle."""
    rng = np.random.default_rng(31 + gm2)
    nt, H, W, nj = 4, 12, 16, 3
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, 1, nan_frac=0.0, gm2=gm2, gm3=3)
    nh = len(batch["hidden_marker"])
    assert nh == 9
    _saturate(rng, pred, batch, [4] if how == "one" else np.arange(nh), 45.0)
    losses, dpred, _, L = _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)
    if how == "all":
        assert losses["hidden_loss_pred"] == 0.0
    else:
        assert losses["hidden_loss_pred"] > 0.0


@pytest.mark.parametrize("gm2", [1, 2])
def test_hidden_markers_saturated_in_fp32_only(lib_built, gm2):
    """Peaks between ~17 and ~37: fp32 sigmoid is exactly 1 (c = 1, the marker is not counted) but fp64's is not (it is, with a weight
    of 1e-11 -- which changes the normaliser's count).  TF ran this graph in fp32, so the kernel's fp32 count is the intended behaviour:
    the reference here is the same autograd oracle evaluated in float32, which rounds exactly like TF did.  (The fp64 oracle, shown
    below, disagrees by the one marker's H * W cells in the denominator.)"""
    rng = np.random.default_rng(41 + gm2)
    nt, H, W, nj = 4, 12, 16, 3
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, 1, nan_frac=0.0, gm2=gm2, gm3=3)
    _saturate(rng, pred, batch, [2, 6], 25.0)
    assert torch.sigmoid(torch.tensor(25.0)).item() == 1.0 and torch.sigmoid(torch.tensor(25.0, dtype=torch.float64)).item() < 1.0
    losses, _, _, _ = _check_dgp(batch, S0, pred, loc, hy, ws, ws_max, oracle_dtype=torch.float32)
    from oracle import dgp_train_oracle as T
    L64 = T.dgp_loss(torch.tensor(pred, dtype=torch.float64), torch.tensor(loc, dtype=torch.float64), batch, _cfg(hy, nj, S0, ws, ws_max))
    assert abs(losses["hidden_loss_pred"] - float(L64["hidden_loss_pred"])) > 1e-3 * abs(float(L64["hidden_loss_pred"]))


@pytest.mark.parametrize("gm2,gm3", [(1, 3), (2, 3), (1, 0)])
def test_reduce_max_ties_share_the_gradient(lib_built, gm2, gm3):
    """A plateau of three cells at exactly 5.0 as the maximum of every hidden marker (below saturation): d c / d x goes to the three
    cells in equal shares, as tf.reduce_max and torch.amax split it."""
    rng = np.random.default_rng(51 + gm2)
    nt, H, W, nj = 3, 12, 16, 3
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, 1, nan_frac=0.0, gm2=gm2, gm3=gm3)
    pred = np.clip(pred, -4.0, 4.0)
    for m in batch["hidden_marker"]:
        idx = rng.choice(H * W, 3, replace=False)
        pred[m // nj].reshape(H * W, nj)[idx, m % nj] = 5.0
    _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)


@pytest.mark.parametrize("gm2,gm3", [(0, 0), (1, 3), (2, 3), (1, 0)])
def test_no_hidden_markers(lib_built, gm2, gm3):
    """Every frame visible, no NaN: the hidden list is empty, hidden_loss_pred is 0 and the gm2 / gm3 machinery must stay out."""
    rng = np.random.default_rng(61 + 3 * gm2 + gm3)
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, 3, 12, 16, 3, 3, nan_frac=0.0, gm2=gm2, gm3=gm3)
    assert len(batch["hidden_marker"]) == 0
    losses, _, _, _ = _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)
    assert losses["hidden_loss_pred"] == 0.0


@pytest.mark.parametrize("gm2,gm3", [(0, 0), (1, 3)])
def test_visible_frame_with_every_joint_nan(lib_built, gm2, gm3):
    """A visible frame whose joints are all NaN: all its markers move to the hidden set and it contributes no locref entry."""
    from deepgraphpose_amd import dataset as D
    rng = np.random.default_rng(71 + gm2)
    nt, H, W, nj = 3, 12, 16, 3
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, nt, H, W, nj, 1, nan_frac=0.0, gm2=gm2, gm3=gm3)
    vis = np.array([0, 2])
    jl = np.stack([rng.uniform(1, H - 2, (2, nj)), rng.uniform(1, W - 2, (2, nj))], -1)
    jl[1] = np.nan
    vm, hm, vt = D.gen_idx_chunk(vis, np.array([1]), jl)
    lt, lm = D.coord2map(jl, H, W, nj, 8)
    lmap, lmask = np.zeros((nt, H, W, 2 * nj)), np.zeros((nt, H, W, 2 * nj))
    lmap[vis], lmask[vis] = lt, lm
    batch = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt, nt=nt)
    assert len(vm) == nj and len(hm) == 2 * nj and not lmask[2].any()
    _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)


def test_all_zero_locref_mask(lib_built):
    """No non-zero locref mask entry: the locref loss is 0 (not 0 / 0) and its gradient exactly 0 everywhere."""
    rng = np.random.default_rng(81)
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, 3, 12, 16, 3, 2, gm2=1, gm3=3)
    batch["locref_mask"] = np.zeros_like(batch["locref_mask"])
    losses, _, dloc, _ = _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)
    assert losses["visible_loss_locref"] == 0.0
    assert not dloc.any()


@pytest.mark.parametrize("huber", [True, False])
def test_many_visible_markers(lib_built, huber):
    """nt = 11, nj = 20 on 60 x 80, all visible: 220 visible markers, each loss_locref_backward workgroup recounting the whole mask."""
    rng = np.random.default_rng(91 + huber)
    batch, S0, pred, loc, hy, ws, ws_max = _case(rng, 11, 60, 80, 20, 11, nan_frac=0.0, gm2=1, gm3=3, huber=huber)
    assert len(batch["visible_marker"]) == 220
    _check_dgp(batch, S0, pred, loc, hy, ws, ws_max)


# ---------------------------------------------------------------------------------------------------------------------- DLC loss
def _dlc(pred, loc, pt, pw, lt, lm, huber=True, weight=0.05):
    """dgp_dlc_loss_fwd_bwd -> (losses [part, locref, total], dpred, dloc); loc None: no locref term"""
    from deepgraphpose_amd import _lib
    from deepgraphpose_amd.engine import _ptr
    lib = _lib.load()
    nt, H, W, nj = pred.shape
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    dp = torch.full(pred.shape, np.nan, device="cuda")
    dl = None if loc is None else torch.full(loc.shape, np.nan, device="cuda")
    losses, scratch = torch.full((4,), np.nan, device="cuda"), torch.empty(4, dtype=torch.float64, device="cuda")
    args = [d(pred), d(loc), d(pt), d(pw), d(lt), d(lm)]
    _lib.check(lib.dgp_dlc_loss_fwd_bwd(*[None if a is None else _ptr(a) for a in args], nt, H, W, nj, weight, int(huber), _ptr(dp),
                                        None if dl is None else _ptr(dl), _ptr(losses), _ptr(scratch), 32, None))
    torch.cuda.synchronize()
    return losses.cpu().numpy()[:3], dp.cpu().numpy(), None if dl is None else dl.cpu().numpy()


def _check_dlc(pred, loc, pt, pw, lt, lm, huber=True):
    """the kernels vs the fp64 autograd oracle, test_dlc_loss_kernel_matches_autograd's tolerances"""
    from oracle import dgp_train_oracle as T
    f = lambda a, g=False: None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=g)
    tp, tl = f(pred, True), f(loc, True)
    L = T.dlc_loss(tp, tl, f(pt), f(lt), f(lm), f(pw), 0.05, huber=huber)
    L["total_loss"].backward()
    L = {k: float(v.detach()) for k, v in L.items()}
    got, dp, dl = _dlc(pred, loc, pt, pw, lt, lm, huber)
    assert np.isfinite(got).all() and np.isfinite(dp).all() and np.isfinite(dl).all()
    assert abs(got[0] - L["part_loss"]) < 1e-5 * max(1, L["part_loss"])
    assert abs(got[1] - L["locref_loss"]) < 1e-5
    assert abs(got[2] - L["total_loss"]) < 1e-5 * max(1, L["total_loss"])
    gp, gl = tp.grad.numpy(), tl.grad.numpy()
    assert np.abs(dp - gp).max() < 1e-6 * max(1e-3, np.abs(gp).max()) + 1e-10
    assert np.abs(dl - gl).max() < 1e-6 * max(1e-3, np.abs(gl).max()) + 1e-10
    return got, dp, dl


def _dlc_inputs(rng, nt, H, W, nj, scale=3.0):
    pred = (rng.standard_normal((nt, H, W, nj)) * scale).astype(np.float32)
    loc = (rng.standard_normal((nt, H, W, 2 * nj)) * 1.5).astype(np.float32)
    pt = (rng.random((nt, H, W, nj)) < 0.1).astype(np.float32)
    lm = np.repeat(pt, 2, axis=3)
    lt = rng.standard_normal((nt, H, W, 2 * nj)).astype(np.float32) * lm
    return pred, loc, pt, lt, lm


@pytest.mark.parametrize("case", ["squared_error", "fractional_weights", "zero_weights", "logits_100", "large_grid"])
def test_dlc_loss_edges(lib_built, case):
    """huber = 0 (d^2, 2 d); part weights mixing 0, 0.25 and 1 (the denominator counts the non-zero ones); all weights 0 (part loss and
    its gradient exactly 0); logits of +-100 (expf(100) overflows in dlc_loss_backward's sigmoid); and 11 x 59 x 81 x 20 = 1 051 380
    cells -- more than the 256 x 1024 threads of either kernel and no multiple of 256, so both grid-stride loops wrap with a ragged end."""
    rng = np.random.default_rng(7)
    shape = (11, 59, 81, 20) if case == "large_grid" else (2, 23, 31, 3)
    pred, loc, pt, lt, lm = _dlc_inputs(rng, *shape)
    pw, huber = None, True
    if case == "squared_error":
        huber = False
    elif case == "fractional_weights":
        pw = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), pt.shape)
    elif case == "zero_weights":
        pw = np.zeros_like(pt)
    elif case == "logits_100":
        pred = np.where(rng.random(pred.shape) < 0.5, 100.0, -100.0).astype(np.float32)
        pred[0, :3, :3, 0] = [[100.0, -100.0, 99.5], [-99.5, 0.25, 1.0], [-1.0, 30.0, -30.0]]
    elif case == "large_grid":
        assert pt.size > 256 * 1024 and pt.size % 256 != 0
        pw = rng.choice(np.array([0.0, 1.0], np.float32), pt.shape, p=[0.3, 0.7])
    got, dp, dl = _check_dlc(pred, loc, pt, pw, lt, lm, huber)
    if case == "zero_weights":
        assert got[0] == 0.0 and not dp.any()


@pytest.mark.parametrize("case", __import__("_tf_kat").CE_KNOWN_ANSWERS, ids=lambda c: c[0])
def test_dlc_loss_sigmoid_ce_known_answers(lib_built, case):
    """TF's 3 x 3 sigmoid cross-entropy cases (tests/_tf_kat.py) as nt=1, H=3, W=3, nj=1 through dgp_dlc_loss_fwd_bwd (no locref term):
    the loss, and the gradient w (sigmoid(x) - z) / #non-zero weights (sigmoid(+-100) is 1 / 0 in fp32)."""
    import _tf_kat as K
    name, labels, weights, want = case
    x = K.CE_LOGITS.reshape(1, 3, 3, 1)
    z = labels.reshape(1, 3, 3, 1)
    w = None if weights is None else weights.reshape(1, 3, 3, 1)
    got, dp, _ = _dlc(x, None, z, w, None, None)
    assert abs(got[0] - want) <= 1e-6 * max(1.0, want), (got[0], want)
    wf = np.ones_like(z) if w is None else w
    nz = np.count_nonzero(wf)
    np.testing.assert_allclose(dp, wf * ((x > 0) - z) / max(nz, 1), rtol=1e-6, atol=0)


def test_dlc_loss_broadcast_marker_weights_known_answer(lib_built):
    """One weight per marker (3 and 0) written out over each 3 x 3 map: 3 * 600 / 9 = 200 -- the denominator counts the cells."""
    import _tf_kat as K
    x = np.stack([K.CE_LOGITS] * 2).reshape(2, 3, 3, 1)
    z = np.stack([K.CE_LABELS_WRONG] * 2).reshape(2, 3, 3, 1)
    w = np.broadcast_to(K.CE_MARKER_WEIGHTS.reshape(2, 1, 1, 1), x.shape)
    got, _, _ = _dlc(x, None, z, w, None, None)
    assert abs(got[0] - K.CE_MARKER_WEIGHTS_LOSS) <= 1e-6 * K.CE_MARKER_WEIGHTS_LOSS


@pytest.mark.parametrize("huber,want", [(True, "HUBER_MASKED"), (False, "MSE_MASKED")])
def test_dlc_locref_known_answers(lib_built, huber, want):
    """tf.losses.huber_loss / mean_squared_error with TF's mask (tests/_tf_kat.py) as the DLC locref term, weight 1: one marker, the five
    residuals in both channels of a 1 x 5 map."""
    import _tf_kat as K
    d = np.repeat(K.HUBER_D, 2).reshape(1, 1, 5, 2)
    m = np.repeat(K.HUBER_MASK, 2).reshape(1, 1, 5, 2)
    x = np.zeros((1, 1, 5, 1))
    got, _, dl = _dlc(x, d, x, None, np.zeros_like(d), m, huber=huber, weight=1.0)
    assert abs(got[1] - getattr(K, want)) <= 1e-6 * getattr(K, want)
    de = np.clip(d, -1, 1) if huber else 2 * d
    np.testing.assert_allclose(dl, m * de / m.sum(), rtol=1e-6, atol=0)
