"""The temporal clique's two kernels (loss_temporal_weights, loss_temporal in csrc/dgp_loss.hip) against the float32-coordinate mode of the
autograd oracle, at the boxes, kinks, ties and sizes where they branch.  Inputs and reference runs: _temporal_cases.py.  Every case
asserts, FROM THE REFERENCE, the branch it is named for; nothing is skipped or selected on a value the kernel computed.

Bounds (test_train_gpu.py::test_temporal_clique_matches_oracle's): 1e-4 relative on wt_loss and on the recovered weight, 3e-4 max|g|
on d total / d pred; 1e-6 relative between two runs of the kernels (test_loss_with_device_vector_field_equals_host_copy's)."""
import numpy as np
import pytest
import torch

import _temporal_cases as TC

pytestmark = pytest.mark.gpu
REL_LOSS, REL_GRAD, REL_RERUN = 1e-4, 3e-4, 1e-6


def _run(c, batch=None, **hyper):
    from deepgraphpose_amd.loss import dgp_loss_fwd_bwd
    z = np.zeros(0)
    losses, dpred, dloc, mu = dgp_loss_fwd_bwd(torch.from_numpy(c.pred).cuda(), torch.from_numpy(c.loc).cuda(), batch or c.batch,
                                               c.hyper(**hyper), np.zeros((0, c.nj)), z, z, TC.N_TOT, TC.N_VIS_TOT)
    torch.cuda.synchronize()
    return losses, dpred.cpu().numpy(), dloc.cpu().numpy(), mu.cpu().numpy()


def _check_one_pair(name, other_mode_differs=False):
    """one visible pair: wt_loss and the weight recovered from it against the float32-coordinate reference -> (reference info, weight)"""
    c, ref, r64 = TC.case(name), TC.reference(name), TC.reference(name, True, "float64")
    assert (c.nt, c.nj) == (2, 1) and len(c.batch["hidden_marker"]) == 0
    L, L64 = ref["loss"]["wt_loss"], r64["loss"]["wt_loss"]
    assert L > 0
    if other_mode_differs:
        assert abs(L64 - L) > 10 * REL_LOSS * L
    else:
        assert abs(L64 - L) < 0.1 * REL_LOSS * L
    losses, dpred, _, _ = _run(c)
    w_ref = ref["info"]["w"][0, 0]
    w_gpu = losses["wt_loss"] * w_ref / L            # wt_loss = (relu(D - wt_max) + wt_max) * w * C, D and C from the reference
    print("%s: wt_loss gpu %.9g ref %.9g rel %.3g (bound %.0e); f64-mode rel %.3g" % (name, losses["wt_loss"], L, abs(losses["wt_loss"] - L) / L,
                                                                                    REL_LOSS, abs(L64 - L) / L))
    assert abs(losses["wt_loss"] - L) <= REL_LOSS * L
    assert abs(w_gpu - w_ref) <= REL_LOSS * w_ref
    assert abs(losses["total_loss"] - ref["loss"]["total_loss"]) <= REL_LOSS * abs(ref["loss"]["total_loss"])
    assert np.isfinite(dpred).all()
    return ref["info"], losses


@pytest.mark.parametrize("name", sorted(TC.BOXES))
def test_weight_of_a_clamped_box(lib_built, name):
    """Each of the four clamps alone, all four (a position in each corner; the pair spanning the frame), none, r0 == r1 and c0 == c1."""
    p0, p1, clamps = TC.BOXES[name]
    info, _ = _check_one_pair("box_" + name)
    assert tuple(info["clamped"][0, 0].astype(int)) == clamps
    assert info["m"][0, 0] > 1
    assert tuple(info["P"].reshape(-1)) == (p0[0], p0[1], p1[0], p1[1])
    assert (info["P"][0, 0, 0] == info["P"][1, 0, 0]) == (name == "same_row") and (info["P"][0, 0, 1] == info["P"][1, 0, 1]) == (name == "same_col")


@pytest.mark.parametrize("name", ["outside_row", "outside_col", "outside_both_rows"])
def test_weight_with_a_position_outside_the_field(lib_built, name):
    """Hin, Win = 75, 83 under a 10 x 11 map (80 x 88 px): a field smaller than stride * H x stride * W, and a label beyond its edge."""
    info, _ = _check_one_pair(name)
    c = TC.case(name)
    assert c.batch["vector_field"].shape == (1, 75, 83) and (c.H * 8, c.W * 8) != (75, 83)
    P = info["P"]
    assert (P[:, 0, 0].max() > 75) if "row" in name else (P[:, 0, 1].max() > 83)
    assert info["clamped"][0, 0, 2 if "row" in name else 3] and info["m"][0, 0] > 1


@pytest.mark.parametrize("name", ["drop_bottom", "drop_right"])
def test_weight_where_float32_drops_the_last_sample(lib_built, name):
    """The two stored positions (test_temporal_clique_cpu.py's search): the kernel agrees with the float32 coordinates, which drop the last
    row / column, and is as far from the float64 mode as the reference's two modes are from each other."""
    info, losses = _check_one_pair(name, other_mode_differs=True)
    i64 = TC.reference(name, True, "float64")
    assert (info["rows"][0, 0], info["cols"][0, 0]) == ((TC.HIN - 1, TC.WIN) if name == "drop_bottom" else (TC.HIN, TC.WIN - 1))
    assert (i64["info"]["rows"][0, 0], i64["info"]["cols"][0, 0]) == (TC.HIN, TC.WIN)
    L, L64 = TC.reference(name)["loss"]["wt_loss"], i64["loss"]["wt_loss"]
    assert abs((losses["wt_loss"] - L64) - (L - L64)) <= REL_LOSS * L and abs(L - L64) > 0.01 * L


def test_weight_around_mean_flow_one(lib_built):
    """m just below 1 (w = wt / H / W, no dependence on m), just above (w = m^-3 wt / H / W), and an all-zero field."""
    below, _ = _check_one_pair("m_below_1")
    above, _ = _check_one_pair("m_above_1")
    zero, _ = _check_one_pair("zero_field")
    k = 50.0 / 12 / 16
    assert 0.998 < below["m"][0, 0] < 1 and below["w"][0, 0] == k
    assert 1 < above["m"][0, 0] < 1.002 and 0.99 * k < above["w"][0, 0] < 0.998 * k
    assert zero["m"][0, 0] == 0 and zero["w"][0, 0] == k


@pytest.mark.parametrize("name,shape", [("hin_1", (1, TC.WIN)), ("win_1", (TC.HIN, 1)), ("hin_win_1", (1, 1))])
def test_weight_on_a_one_row_or_one_column_field(lib_built, name, shape):
    info, _ = _check_one_pair(name)
    assert TC.case(name).batch["vector_field"].shape[1:] == shape
    assert (info["rows"][0, 0], info["cols"][0, 0]) == shape and info["m"][0, 0] > 1


@pytest.mark.parametrize("name", ["kink_below", "kink_at", "kink_above"])
def test_relu_kink(lib_built, name):
    """D = 40 px exactly (3-4-5 in map units times the stride) against wt_max = 50, 40, 30."""
    info, _ = _check_one_pair(name)
    D, wt_max = info["D"][0, 0], TC.case(name).wt_max
    assert D == 40.0 and {"kink_below": D < wt_max, "kink_at": D == wt_max, "kink_above": D > wt_max}[name]
    if name != "kink_above":
        assert abs(TC.reference(name)["loss"]["wt_loss"] / TC.reference("kink_above")["loss"]["wt_loss"] - wt_max / 40.0) < 1e-12


def _check_gradient(name, monkeypatch=None):
    c, on, off, f64 = TC.case(name), TC.reference(name), TC.reference(name, False), TC.reference(name, True, "float64")
    mask = np.asarray(c.batch.get("wt_batch_mask", np.ones(c.nt - 1))) != 0
    g = on["grad"]
    gmax = np.abs(g).max()
    assert (on["info"]["m"][mask] > 1).all() and np.isfinite(g).all()
    assert not TC.near_tie(on["info"], mask)
    share = np.abs(g - off["grad"]).max() / gmax
    assert share >= 100 * REL_GRAD, share
    assert np.abs(f64["grad"] - g).max() < 0.1 * REL_GRAD * gmax
    L = on["loss"]["wt_loss"]
    assert abs(f64["loss"]["wt_loss"] - L) < 0.1 * REL_LOSS * L
    losses, dpred, _, mu = _run(c)
    dev = np.abs(dpred - g).max() / gmax
    print("%s: wt_loss rel %.3g (bound %.0e); dpred dev %.3g max|g| (bound %.0e); weight-gradient share %.3g" % (
        name, abs(losses["wt_loss"] - L) / L, REL_LOSS, dev, REL_GRAD, share))
    assert abs(losses["wt_loss"] - L) <= REL_LOSS * L
    assert np.isfinite(dpred).all() and dev <= REL_GRAD
    return c, on, losses, dpred, mask


@pytest.mark.parametrize("kind", ["weight_only", "wtmax0", "wtmax_mid"])
@pytest.mark.parametrize("boxes", sorted(TC.GRAD_CELLS))
def test_gradient_through_weight_and_distance(lib_built, boxes, kind):
    """Hidden frames on sharp peaks, wt = 1e8 so that the temporal term is d total / d pred.  weight_only: wt_max above every D, the
    gradient flows through the flow weight alone; wtmax0: through D and w; wtmax_mid: wt_max between the pairs' distances.  Boxes with no
    clamp, top + bottom, left + right active, and a visible-hidden pair (only the hidden frame receives a gradient)."""
    name = "grad_%s_%s" % (boxes, kind)
    c, on, losses, dpred, mask = _check_gradient(name)
    D, cl = on["info"]["D"][mask], on["info"]["clamped"][mask]
    if kind == "weight_only":
        assert (D < c.wt_max).all()
    elif kind == "wtmax0":
        assert c.wt_max == 0 and (D > 0).all()
    else:
        assert D.min() < c.wt_max < D.max()
    want = TC.GRAD_CELLS[boxes][2]
    if want is not None:
        assert [tuple(x) for x in cl.reshape(-1, 4).astype(int)] == list(want)
    if boxes == "visible_hidden":
        assert len(c.batch["visible_marker"]) == c.nj and mask.tolist() == [True, False]
        # the visible frame's gradient is its cross-entropy's alone: the temporal term, which is all but 1e-3 of the hidden frame's, adds nothing
        assert np.abs(on["grad"][0]).max() < 1e-3 * np.abs(on["grad"]).max() and np.abs(dpred[0]).max() < 1e-3 * np.abs(on["grad"]).max()
        assert np.abs(on["grad"][1]).max() > 100 * np.abs(on["grad"][2]).max()


def test_gradient_of_a_tie(lib_built):
    """Two hidden frames with bitwise identical maps: r0 == r1, c0 == c1, D == 0.  The gradient is finite, equals the oracle's (min / max
    share a tie 0.5 / 0.5; no distance gradient at D == 0), and is the same for the two frames."""
    c, on, losses, dpred, mask = _check_gradient("grad_tie")
    assert np.array_equal(c.pred[1], c.pred[2])
    P = on["info"]["P"]
    assert np.array_equal(P[1], P[2]) and (on["info"]["D"][1] == 0).all() and c.wt_max > 0
    assert np.allclose(on["grad"][1], on["grad"][2], rtol=0, atol=1e-12 * np.abs(on["grad"]).max())
    assert np.abs(dpred[1] - dpred[2]).max() <= REL_RERUN * np.abs(dpred).max()


def test_more_than_256_pairs(lib_built):
    """nt = 14, nj = 20: 260 pairs, so loss_temporal's threads take a second pass; one frame pair masked out."""
    c, on, losses, dpred, mask = _check_gradient("grad_260_pairs")
    assert (c.nt - 1) * c.nj == 260 and c.batch["vector_field"].shape == (13, 48, 64)
    D = on["info"]["D"][mask]
    cl = on["info"]["clamped"]
    assert (D > c.wt_max).any() and (D < c.wt_max).any()
    assert cl[..., :2].any() and not cl[..., 2:].any()
    # the pairs beyond the 256th carry weight: without them the loss would be far outside the bound
    v = ((np.maximum(on["info"]["D"] - c.wt_max, 0) + c.wt_max) * on["info"]["w"]).reshape(-1)
    assert 1 - np.sqrt((v[:256] ** 2).sum() / (v ** 2).sum()) > 10 * REL_LOSS


def _cmp_runs(a, b):
    (la, dpa, dla, mua), (lb, dpb, dlb, mub) = a, b
    for k in la:
        if k != "wt_loss":
            assert abs(la[k] - lb[k]) <= REL_RERUN * max(abs(lb[k]), 1e-6), (k, la[k], lb[k])
    for x, y in ((dpa, dpb), (dla, dlb), (mua, mub)):
        assert np.abs(x - y).max() <= REL_RERUN * max(np.abs(y).max(), 1e-6)


@pytest.mark.parametrize("nt", [6, 2])
def test_all_pairs_masked_equals_no_temporal_term(lib_built, nt):
    """wt_batch_mask all zero: F == 0, wt_loss == 0.0 and loss_temporal adds nothing; everything else equals the wt = 0 call."""
    import test_train_gpu as TT
    from deepgraphpose_amd.loss import dgp_loss_fwd_bwd, DGPHyper
    H, W, nj = 12, 16, 3
    rng = np.random.default_rng(nt)
    batch, S0 = TT._make_loss_case(rng, nt, H, W, nj, 1, 0.0, 2)
    batch["vector_field"] = TC.wavy_field(nt - 1, 96, 128)
    batch["wt_batch_mask"] = np.zeros(nt - 1, dtype=np.float32)
    pred = torch.from_numpy((rng.standard_normal((nt, H, W, nj)) * 2).astype(np.float32)).cuda()
    loc = torch.from_numpy(rng.standard_normal((nt, H, W, 2 * nj)).astype(np.float32)).cuda()
    ws, ws_max = rng.uniform(5, 20, 2), rng.uniform(10, 40, 2)
    out = []
    for wt in (50.0, 0.0):
        l, dp, dl, mu = dgp_loss_fwd_bwd(pred, loc, batch, DGPHyper(gm2=1, gm3=3, wt=wt, wt_max=6.0), S0, ws, ws_max, 500.0, 37.0)
        out.append((l, dp.cpu().numpy(), dl.cpu().numpy(), mu.cpu().numpy()))
    assert out[0][0]["wt_loss"] == 0.0 and out[1][0]["wt_loss"] == 0.0
    assert np.abs(out[0][2]).max() > 0 and out[0][0]["total_loss"] > 0
    _cmp_runs(out[0], out[1])


def test_streaming_variant_feeds_the_temporal_kernels(lib_built, monkeypatch):
    """DGP_LOSS_STREAM=1 (loss_ce_backward<true>) on a gradient case against the LDS variant, and against the oracle."""
    name = "grad_top_bottom_wtmax_mid"
    c = TC.case(name)
    a = _run(c)
    monkeypatch.setenv("DGP_LOSS_STREAM", "1")
    b = _run(c)
    c2, on, losses, dpred, mask = _check_gradient(name)
    monkeypatch.delenv("DGP_LOSS_STREAM")
    assert a[0]["wt_loss"] > 0 and abs(a[0]["wt_loss"] - b[0]["wt_loss"]) <= REL_RERUN * a[0]["wt_loss"]
    _cmp_runs(b, a)


def test_temporal_term_on_maps_beyond_the_lds_limit(lib_built):
    """136 x 240 maps, nt = 3 (the streaming kernel by size) with wt > 0, against the oracle; the field is 272 x 480, not stride * H x
    stride * W, and the peaks lie inside it."""
    c, on, losses, dpred, mask = _check_gradient("grad_beyond_lds")
    assert 2 * c.H * c.W * 4 > 150 * 1024 and c.batch["vector_field"].shape == (2, 272, 480)
    P, cl = on["info"]["P"], on["info"]["clamped"]
    assert P[..., 0].max() < 272 and P[..., 1].max() < 480
    assert cl[0, 0, 0] and cl[1, 0, 2]
    D = on["info"]["D"]
    assert (D > c.wt_max).any() and (D < c.wt_max).any()


@pytest.mark.parametrize("bad", ["leading", "ndim", "mask"])
def test_prepare_rejects_a_wrong_field_or_mask(lib_built, bad):
    """A host vector_field that is not [nt-1, Hin, Win], or a wt_batch_mask of another length than 1 or nt-1, would make
    loss_temporal_weights read past a buffer: dgp_loss_prepare raises before anything is launched."""
    from deepgraphpose_amd.loss import dgp_loss_prepare
    c = TC.case("grad_inactive_wtmax0")
    b = dict(c.batch)
    if bad == "leading":
        b["vector_field"] = c.batch["vector_field"][:1]
    elif bad == "ndim":
        b["vector_field"] = c.batch["vector_field"][0]
    else:
        b["wt_batch_mask"] = np.ones(c.nt, dtype=np.float32)
    z = np.zeros(0)
    with pytest.raises(ValueError):
        dgp_loss_prepare(c.nt, c.H, c.W, c.nj, b, c.hyper(), np.zeros((0, c.nj)), z, z, TC.N_TOT, TC.N_VIS_TOT, torch.device("cuda", 0))
    for ok_mask in (np.ones(1, dtype=np.float32), np.ones(c.nt - 1, dtype=np.float32)):
        dgp_loss_prepare(c.nt, c.H, c.W, c.nj, dict(c.batch, wt_batch_mask=ok_mask), c.hyper(), np.zeros((0, c.nj)), z, z, TC.N_TOT,
                         TC.N_VIS_TOT, torch.device("cuda", 0))
