"""The temporal clique's reference (oracle/dgp_train_oracle.py): its float32-coordinate mode against its float64 mode, the search for the
boxes where the two decide differently, and the conditions the GPU cases (test_temporal_clique_gpu.py) rest on, checked on the reference
alone.  No GPU."""
import numpy as np
import pytest
import torch

import _temporal_cases as TC
from oracle import dgp_train_oracle as T

F32 = np.float32
HIN, WIN = TC.HIN, TC.WIN
# the comparison bounds of the GPU tests (test_train_gpu.py::test_temporal_clique_matches_oracle's)
REL_LOSS, REL_GRAD = 1e-4, 3e-4


def _both_modes(vf, p0, p1):
    Hin, Win = vf.shape
    out = []
    for dt in (np.float32, np.float64):
        box, cl = T.temporal_box(p0[0], p0[1], p1[0], p1[1], Hin, Win, coord_dtype=dt)
        kept = {}
        m = T.crop_and_resize_mean(vf, box, (Hin, Win), dt, kept)
        out.append((m, cl, kept["rows"], kept["cols"]))
    return out


@pytest.mark.parametrize("Hin,Win", [(96, 128), (75, 83), (48, 64)])
def test_float32_mode_equals_float64_mode_on_unclamped_boxes(Hin, Win):
    """A box inside the frame: the same clamps (none), the same samples kept (all), and a mean that differs only by the float32 rounding
    of the sample coordinates: at most 2 ulp(n - 1) per coordinate (one for a1 * (n - 1), one for the fused sum) times the field's
    largest slope (0.5 / 7 per row, 0.5 / 9 per column)."""
    rng = np.random.default_rng(Hin)
    vf = TC.wavy_field(1, Hin, Win)[0].astype(np.float64)
    bound = 2 * np.spacing(F32(Hin - 1)) * 0.5 / 7 + 2 * np.spacing(F32(Win - 1)) * 0.5 / 9
    for _ in range(40):
        p0 = (rng.uniform(10.5, Hin - 10.5), rng.uniform(10.5, Win - 10.5))
        p1 = (rng.uniform(10.5, Hin - 10.5), rng.uniform(10.5, Win - 10.5))
        (m32, cl32, r32, c32), (m64, cl64, r64, c64) = _both_modes(vf, p0, p1)
        assert cl32 == cl64 == (False, False, False, False)
        assert (r32, c32) == (r64, c64) == (Hin, Win)
        assert abs(m32 - m64) <= bound, (m32, m64, bound)
        assert abs(m32 - m64) < 0.01 * REL_LOSS * m64


def _search(axis):
    """first position in [n - 9, n - 1] (fixed seed; both markers on it, the other coordinate mid-frame) whose box ends on the bottom
    (axis 0) / right (axis 1) edge and keeps one sample fewer in the float32 mode than in the float64 mode"""
    n = (HIN, WIN)[axis]
    vf = TC.wavy_field(1, HIN, WIN)[0].astype(np.float64)
    rng = np.random.default_rng(2024 + axis)
    tried = 0
    for _ in range(2000):
        t, P = TC.px_to_label(rng.uniform(n - 9, n - 1))
        p0, p1 = ((P, 40.0), (P, 60.0)) if axis == 0 else ((40.0, P), (60.0, P))
        a, b = _both_modes(vf, p0, p1)
        assert a[1] == b[1] and a[1][2 + axis] and sum(a[1]) == 1          # clamped at that edge alone, in both modes
        tried += 1
        if (a[2], a[3]) != (b[2], b[3]):
            return float(t), p0, p1, a, b, vf, tried
    raise AssertionError("no box found")


@pytest.mark.parametrize("axis", [0, 1])
def test_search_finds_a_box_whose_last_sample_float32_drops(axis):
    """The stored positions of the GPU test are what this search yields.  float32 drops exactly the last row / column, float64 keeps it;
    the mean loses that row's share: (mean of the row's samples) / Hin, up to the coordinate rounding of the other rows (as above)."""
    t, p0, p1, a, b, vf, tried = _search(axis)
    assert t == (TC.DROP_BOTTOM_LABEL, TC.DROP_RIGHT_LABEL)[axis]
    n = (HIN, WIN)[axis]
    assert (a[2], a[3]) == ((HIN - 1, WIN) if axis == 0 else (HIN, WIN - 1)) and (b[2], b[3]) == (HIN, WIN)
    # the float64 samples of the last row / column
    box, _ = T.temporal_box(p0[0], p0[1], p1[0], p1[1], HIN, WIN)
    iy, _ = T._crop_axis(box[0], box[2], HIN, HIN, np.float64)
    ix, _ = T._crop_axis(box[1], box[3], WIN, WIN, np.float64)
    lerp = lambda img, y, x: np.array([[(img[int(np.floor(v)), int(np.floor(u))] * (1 - (u - np.floor(u))) + img[int(np.floor(v)), int(np.ceil(u))] * (u - np.floor(u))) * (1 - (v - np.floor(v)))
                                        + (img[int(np.ceil(v)), int(np.floor(u))] * (1 - (u - np.floor(u))) + img[int(np.ceil(v)), int(np.ceil(u))] * (u - np.floor(u))) * (v - np.floor(v))
                                        for u in x] for v in y])
    last = lerp(vf, iy[-1:], ix) if axis == 0 else lerp(vf, iy, ix[-1:])
    share = last.mean() / n
    bound = 2 * np.spacing(F32(HIN - 1)) * 0.5 / 7 + 2 * np.spacing(F32(WIN - 1)) * 0.5 / 9
    assert abs((b[0] - a[0]) - share) <= bound, (b[0] - a[0], share)
    assert 0.5 / n < (b[0] - a[0]) / b[0] < 1.5 / n           # about 1 / n of the mean: far above the 1e-4 the GPU test compares at
    assert tried <= 100                                       # such boxes are common: 1 to 2 % of the boxes that end on the edge


def test_separately_rounded_float32_keeps_the_last_sample():
    """The drop is the FUSED multiply-add's: with the product i * scale rounded to float32 first (the C++ expression as an x86 build
    without FMA evaluates it) the last sample of a box that ends on the edge is never above n - 1.  a1 (n - 1) and (1 - a1) (n - 1) sum
    to n - 1 exactly, so their two rounding errors cancel up to a tie, and the tie rounds to the even n - 1."""
    rng = np.random.default_rng(5)
    fused = 0
    for n in (75, 83, 96, 128):
        for _ in range(1500):
            _, P = TC.px_to_label(rng.uniform(n - 9, n - 1))
            box, cl = T.temporal_box(P, 40.0, P, 60.0, n, 200, coord_dtype=F32)
            assert cl[2] and box[2] == 1
            c, keep = T.crop_axis_unfused_float32(box[0], box[2], n)
            assert keep.all() and c[-1] <= n - 1
            fused += int(not T._crop_axis(box[0], box[2], n, n, F32)[1].all())
    assert 20 <= fused <= 200          # 0.3 to 3 % with the fused sum


@pytest.mark.parametrize("coord", [np.float32, np.float64])
def test_torch_weights_equal_numpy_weights_and_their_gradient_equals_differences(coord):
    """temporal_flow_weights_torch against temporal_flow_weights in both modes (clamped and unclamped boxes, a tie), and its gradient with
    respect to the positions against central differences of the numpy version in float64."""
    rng = np.random.default_rng(3)
    vf = TC.wavy_field(2, 48, 64).astype(np.float64)
    P = np.stack([rng.uniform(2, 46, (3, 4)), rng.uniform(2, 62, (3, 4))], -1)
    P[1, 0] = P[0, 0]                                    # a tie in both coordinates
    P[0, 1], P[1, 1] = (3.0, 5.0), (44.0, 61.0)          # all four clamps
    P = P.astype(F32).astype(np.float64)
    wtb = np.array([50.0, 20.0])
    Pt = torch.tensor(P, requires_grad=True)
    w = T.temporal_flow_weights_torch(Pt, vf, wtb, 6, 8, coord_dtype=coord)
    info = {}
    w_np = T.temporal_flow_weights(P, vf, wtb, 6, 8, coord_dtype=coord, info=info)
    assert info["clamped"][0, 1].all() and (info["m"] > 1).all()
    np.testing.assert_allclose(w.detach().numpy(), w_np, rtol=1e-12)
    if coord is np.float64:
        coef = torch.tensor(rng.standard_normal(w.shape))
        (w * coef).sum().backward()
        g = Pt.grad.numpy()
        h = 1e-5
        for idx in [(0, 2, 0), (1, 2, 1), (2, 3, 0), (1, 3, 1), (0, 1, 0), (1, 1, 1)]:
            Pp, Pm = P.copy(), P.copy()
            Pp[idx] += h
            Pm[idx] -= h
            fd = ((T.temporal_flow_weights(Pp, vf, wtb, 6, 8) - T.temporal_flow_weights(Pm, vf, wtb, 6, 8)) * coef.numpy()).sum() / (2 * h)
            assert abs(fd - g[idx]) <= 1e-5 * np.abs(g).max() + 1e-12, (idx, fd, g[idx])
        assert g[0, 1, 0] == 0 and g[1, 1, 1] == 0       # a clamped edge passes nothing to its position


def test_zero_distance_option_gives_a_finite_gradient():
    """D == 0: autograd's sqrt gives NaN (as TF's does); wt_zero_dist_grad gives the pair the zero distance gradient the kernel documents."""
    c = TC.case("grad_tie")
    for opt in (False, True):
        pt = torch.tensor(c.pred, dtype=torch.float64, requires_grad=True)
        L = T.dgp_loss(pt, torch.tensor(c.loc, dtype=torch.float64), c.batch, c.cfg(wt_zero_dist_grad=opt))
        L["total_loss"].backward()
        assert (L["_wt_info"]["D"][1] == 0).all()
        assert np.isfinite(pt.grad.numpy()).all() == opt


@pytest.mark.parametrize("name", TC.GRAD_CASES + ["grad_tie", "grad_260_pairs"])
def test_gradient_cases_see_the_weight_gradient(name):
    """What every GPU gradient case rests on, from the reference alone: all unmasked pairs have m > 1; the part of d total / d pred that
    flows through the flow weights (the oracle with wt_weight_grad minus the oracle without) is at least 100 times the comparison bound,
    so a kernel without it -- the wt_weight_grad = False run put in the reference's place -- fails the comparison; and the float32 and
    float64 coordinate modes agree far inside the bound."""
    on, off, f64 = TC.reference(name), TC.reference(name, False), TC.reference(name, True, "float64")
    c = TC.case(name)
    mask = np.asarray(c.batch.get("wt_batch_mask", np.ones(c.nt - 1))) != 0
    assert (on["info"]["m"][mask] > 1).all() and not TC.near_tie(on["info"], mask)
    g = on["grad"]
    assert np.isfinite(g).all() and np.isfinite(off["grad"]).all()
    share = np.abs(g - off["grad"]).max() / np.abs(g).max()
    assert share >= 100 * REL_GRAD, share
    assert not np.abs(off["grad"] - g).max() <= REL_GRAD * np.abs(g).max()          # the comparison, with the weight gradient switched off
    assert np.abs(f64["grad"] - g).max() < 0.1 * REL_GRAD * np.abs(g).max()
    assert abs(f64["loss"]["wt_loss"] - on["loss"]["wt_loss"]) < 0.1 * REL_LOSS * on["loss"]["wt_loss"]
    assert abs(off["loss"]["wt_loss"] - on["loss"]["wt_loss"]) <= 1e-12 * on["loss"]["wt_loss"]
