"""The read-out kernels at their numeric edges (dgp_ops.hip: soft_argmax_kernel<LARGE>, pmap_threshold_kernel, hard_argmax_kernel).

References: oracle.dgp_oracle -- argmax_2d_from_cm in float64 (the anchor) with the fp32 call beside it, likelihood_window evaluated
at the kernel's own mu, argmax_pose_predict on sigmoid_f32.  Gates: the suite's existing ones (test_parity_gpu.py) -- mu within
1e-3 px at stride 8, the normalised map within 1e-6, the likelihood within 2e-6, indices bit-exact.

Every soft-arg-max case runs on both instances of the kernel (the LDS one, and the streaming one through DGP_SOFTARGMAX_STREAM=1,
which the launcher reads per call); their outputs must be equal bit for bit, NaNs included.

The packed record layout (record stride 5) has no layer-level entry in the C-ABI -- only dgp_infer_packed writes it, behind a
whole network -- so it stays with test_boundary_gpu.py::test_infer_packed_equals_infer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PX_TOL = 1e-3          # px
STRIDE = 8.0
PMAP_TOL = 1e-6
LIK_TOL = 2e-6


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _soft_argmax_both(eng, monkeypatch, s, gamma, gl):
    """soft_argmax on the LDS instance and on the streaming one: asserts bit identity, returns (mu, conf, idx, pmap) as numpy"""
    t = torch.from_numpy(s).cuda()
    monkeypatch.delenv("DGP_SOFTARGMAX_STREAM", raising=False)
    lds = [x.clone() for x in eng.soft_argmax(t, gamma, gl, want_pmap=True)]
    monkeypatch.setenv("DGP_SOFTARGMAX_STREAM", "1")
    stream = eng.soft_argmax(t, gamma, gl, want_pmap=True)
    monkeypatch.delenv("DGP_SOFTARGMAX_STREAM")
    for a, b, name in zip(lds, stream, ("mu", "conf", "idx", "pmap")):
        assert torch.equal(_bits(a), _bits(b)), (name, s.shape, gl, gamma)
    return [x.cpu().numpy() for x in lds]


# ---------------------------------------------------------------------------- soft arg-max: wide blurs, maps smaller than the blur
WIDE_CASES = [((2, 3, 2, 3), 7, 1.0), ((1, 1, 9, 2), 5, 1.0), ((1, 9, 1, 2), 6, 3.0), ((2, 13, 11, 2), 7, 0.25), ((1, 60, 80, 2), 7, 1.0)]


@pytest.mark.parametrize("shape,gl,gamma", WIDE_CASES)
def test_soft_argmax_wide_blurs_and_maps_smaller_than_the_blur(eng, monkeypatch, shape, gl, gamma):
    """gauss_len 5-7 (7 fills the kernel's 16-float tap array: 15 taps) on maps down to one row or column, where most taps fall on
    the zero padding.  (On these inputs the fp32 oracle itself is within 1e-6 cells of float64, two orders inside the gate; asserted at a
    tenth of the gate.)"""
    from oracle import dgp_oracle as O
    s = (3.0 * np.random.default_rng(23).standard_normal(shape)).astype(np.float32)
    mu_ref, pm_ref = O.argmax_2d_from_cm(s, gamma, gl)
    mu64, pm64 = O.argmax_2d_from_cm(s, gamma, gl, dtype=np.float64)
    assert np.abs(mu_ref - mu64).max() * STRIDE < PX_TOL / 10            # the reference stands well inside the gate
    mu, conf, idx, pmap = _soft_argmax_both(eng, monkeypatch, s, gamma, gl)
    assert np.abs(mu - mu64).max() * STRIDE < PX_TOL
    assert np.abs(mu - mu_ref).max() * STRIDE < PX_TOL
    assert np.abs(pmap - pm_ref).max() < PMAP_TOL and np.abs(pmap - pm64).max() < PMAP_TOL
    assert (idx >= 0).all() and (idx[..., 0] < shape[1]).all() and (idx[..., 1] < shape[2]).all()
    for b in range(shape[0]):
        iref, lref = O.likelihood_window(s[b], mu[b])
        assert np.array_equal(idx[b], iref)
        assert np.abs(conf[b] - lref).max() < LIK_TOL


@pytest.mark.parametrize("gl", [0, 8, -1])
def test_soft_argmax_rejects_blur_lengths_outside_1_to_7(eng, gl):
    """gauss_len 8 would write 17 taps into gk[16]; gauss_len 0 gives 0/0 taps (the oracle's gaussian_taps(0) is NaN too) and every
    output silently NaN: both are refused, like dgp_loss_fwd_bwd refuses them."""
    from deepgraphpose_amd import _lib
    z = torch.zeros((1, 6, 6, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.DgpError, match="gauss_len must be 1..7"):
        eng.soft_argmax(z, 1.0, gl)


def test_infer_rejects_blur_lengths_outside_1_to_7(eng):
    """The same check at dgp_infer / dgp_infer_packed."""
    from deepgraphpose_amd import _lib
    from deepgraphpose_amd.synthetic import make_weights
    net = eng.DGPNet(50, 2, 64, 96, max_batch=1)
    net.load_weights(make_weights(50, 2, False, seed=1, head_std=0.05))
    frames = torch.zeros((1, 64, 96, 3), dtype=torch.uint8, device="cuda")
    traj = torch.zeros((1, 2, 5), dtype=torch.float32, device="cuda")
    for gl in (0, 8):
        with pytest.raises(_lib.DgpError, match="gauss_len must be 1..7"):
            net.infer(frames, 1.0, gl)
        with pytest.raises(_lib.DgpError, match="gauss_len must be 1..7"):
            net.infer_packed(frames, traj, 1.0, gl)


# ---------------------------------------------------------------------------- soft arg-max: saturated logits
def _saturated_map():
    s = np.full((1, 6, 7, 2), -1e4, dtype=np.float32)
    s[0, 2, 3, 0] = 1e4
    s[0, 5, 6, 1] = 3e4
    return s


def _check_saturated(eng, monkeypatch, s):
    from oracle import dgp_oracle as O
    with np.errstate(all="ignore"):
        mu64, pm64 = O.argmax_2d_from_cm(s, 1.0, 2, dtype=np.float64)
    np.testing.assert_allclose(mu64[0], [[2.0, 3.0], [4.158081, 5.158081]], atol=1e-6)      # the oracle's values, computed once on the CPU
    mu, conf, idx, pmap = _soft_argmax_both(eng, monkeypatch, s, 1.0, 2)
    assert np.abs(mu - mu64).max() * STRIDE < PX_TOL
    assert np.abs(pmap - pm64).max() < PMAP_TOL
    with np.errstate(all="ignore"):
        iref, lref = O.likelihood_window(s[0], mu[0])
    assert np.isnan(lref).all() and iref.tolist() == [[2, 3], [5, 6]]       # e^x / (e^x + 1) = inf / inf at both peaks
    assert np.array_equal(np.isnan(conf[0]), np.isnan(lref))
    assert np.array_equal(idx[0], iref)
    return mu, conf, idx, pmap


def test_soft_argmax_saturated_logits(eng, monkeypatch):
    """Logits of +-1e4 (and 3e4): the softmax is one-hot without overflow (the maximum is subtracted first), mu is the blur's
    expectation around the peak -- clipped at the corner -- and the likelihood is NaN exactly as the reference's numpy expression
    gives it, at the window's first NaN."""
    base = _check_saturated(eng, monkeypatch, _saturated_map())
    s = _saturated_map()
    s[0, 0, 0, 0] = s[0, 4, 1, 1] = -np.inf             # a -inf cell has softmax weight 0 like the -1e4 cells: nothing changes
    for a, b in zip(base, _check_saturated(eng, monkeypatch, s)):
        np.testing.assert_array_equal(a, b)


def test_soft_argmax_with_a_plus_inf_cell(eng, monkeypatch):
    """+inf in joint 0: s - max = inf - inf there, the map's softmax and mu are NaN (the oracle's too); the window index must still
    lie inside the map, and joint 1 of the same frame must not notice."""
    from oracle import dgp_oracle as O
    mu0, conf0, idx0, pmap0 = _soft_argmax_both(eng, monkeypatch, _saturated_map(), 1.0, 2)
    s = _saturated_map()
    s[0, 1, 5, 0] = np.inf
    with np.errstate(all="ignore"):
        mu64, _ = O.argmax_2d_from_cm(s, 1.0, 2, dtype=np.float64)
    assert np.isnan(mu64[0, 0]).all() and not np.isnan(mu64[0, 1]).any()
    mu, conf, idx, pmap = _soft_argmax_both(eng, monkeypatch, s, 1.0, 2)
    assert (idx >= 0).all() and (idx[..., 0] < 6).all() and (idx[..., 1] < 7).all()
    assert np.isnan(mu[0, 0]).all()
    np.testing.assert_array_equal(mu[0, 1], mu0[0, 1])
    np.testing.assert_array_equal(conf[0, 1], conf0[0, 1])
    np.testing.assert_array_equal(idx[0, 1], idx0[0, 1])
    np.testing.assert_array_equal(pmap[..., 1], pmap0[..., 1])


# ---------------------------------------------------------------------------- hard arg-max
def _hard_argmax_vs_oracle(eng, s, with_locref, seed=3):
    """dgp_hard_argmax on s [B,H,W,C] against argmax_pose_predict(sigmoid_f32(s)): idx, prob and the offsets bit for bit (NaN = NaN).
    The indices are range-checked on the host before anything else uses them.  Returns idx."""
    from oracle import dgp_oracle as O
    B, H, W, C = s.shape
    loc = np.random.default_rng(seed).standard_normal((B, H, W, 2 * C)).astype(np.float32) if with_locref else None
    idx, prob, offs = eng.hard_argmax(torch.from_numpy(s).cuda(), None if loc is None else torch.from_numpy(loc).cuda())
    idx, prob, offs = idx.cpu().numpy(), prob.cpu().numpy(), offs.cpu().numpy()
    assert (idx >= 0).all() and (idx[..., 0] < H).all() and (idx[..., 1] < W).all(), idx.tolist()
    for b in range(B):
        with np.errstate(all="ignore"):
            sig = O.sigmoid_f32(s[b])
        offmat = None if loc is None else loc[b].reshape(H, W, C, 2)
        pose_ref, loc_ref = O.argmax_pose_predict(sig, offmat, STRIDE)
        assert np.array_equal(idx[b], loc_ref), (idx[b].tolist(), loc_ref.tolist())
        # the oracle's pose in ITS float64 expression on the kernel's outputs: (index * stride + stride / 2) + offset, x first
        pos = idx[b][:, ::-1].astype("float") * STRIDE + 0.5 * STRIDE + offs[b].astype(np.float64)
        np.testing.assert_array_equal(np.hstack([pos, prob[b][:, None].astype(np.float64)]), pose_ref)
        if loc is None:
            assert not offs.any()
        else:
            for j in range(C):
                np.testing.assert_array_equal(offs[b, j], loc[b, loc_ref[j, 0], loc_ref[j, 1], 2 * j:2 * j + 2])
    return idx


def _tie_map(H, W, cells, peak):
    """Background strictly below the peak; `peak` at the flat indices `cells`.  The peaks are 0.0 or 40.0: their sigmoid is exactly
    0.5 or 1.0 in any fp32 exp, so a bit-exact probability says which cell was SELECTED, not how the last bit of expf rounds."""
    s = (-1.0 - np.abs(np.random.default_rng(H * W).standard_normal((1, H, W, 1)))).astype(np.float32)
    for f in cells:
        s[0, f // W, f % W, 0] = peak
    return s


# flat indices of the equal maxima.  256 threads scan i = t, t + 256, ...: thread t = i % 256, lane t % 64, wave t / 64
TIE_CASES = [(20, 26, (63, 64), 0.0),           # last lane of wave 0 and first lane of wave 1
             (20, 26, (5, 5 + 256), 40.0),      # the same thread on two strides
             (20, 26, (70, 130), 0.0),          # wave 1 then wave 2
             (20, 26, (200, 10), 40.0),         # wave 3 holds the LATER cell's rival: the earlier index (wave 0) must win the merge
             (20, 26, (130, 70 + 256), 0.0),    # a later wave with the lower index against an earlier wave on its second stride
             (3, 11, (31, 32), 40.0),           # 33 cells: lanes 31 | 32 meet in the first shuffle step (xor 32)
             (1, 37, (36,), 0.0), (37, 1, (0, 36), 40.0),       # fewer cells than threads: idle threads must never win
             (1, 1, (0,), 0.0)]


@pytest.mark.parametrize("with_locref", [False, True])
@pytest.mark.parametrize("H,W,cells,peak", TIE_CASES)
def test_hard_argmax_ties_across_reduction_boundaries(eng, H, W, cells, peak, with_locref):
    idx = _hard_argmax_vs_oracle(eng, _tie_map(H, W, cells, peak), with_locref)
    first = min(cells)
    assert idx[0, 0].tolist() == [first // W, first % W]


@pytest.mark.parametrize("with_locref", [False, True])
def test_hard_argmax_saturated_sigmoid(eng, with_locref):
    """All -inf: sigmoid is 0 everywhere, index (0, 0), probability 0.  +inf after 40.0: both sigmoids are exactly 1.0, the earlier
    cell wins.  Three joints in one launch (the strided column)."""
    s = _tie_map(5, 6, (), 0.0).repeat(3, axis=3)
    s[..., 0] = -np.inf
    s[0, 1, 2, 1] = 40.0
    s[0, 3, 3, 1] = np.inf
    s[0, 0, 4, 2] = np.inf
    s[0, 4, 5, 2] = 40.0
    idx = _hard_argmax_vs_oracle(eng, s, with_locref)
    assert idx[0].tolist() == [[0, 0], [1, 2], [0, 4]]


NAN_CASES = [((3, 2),), ((1, 4), (4, 1)), ((4, 5),), ((4, 5), (0, 0))]


@pytest.mark.parametrize("with_locref", [False, True])
@pytest.mark.parametrize("cells", NAN_CASES)
def test_hard_argmax_nan_is_the_maximum_first_one_wins(eng, cells, with_locref):
    """np.argmax treats NaN as the maximum and returns the first one (PET/nnet/predict.py:62-77 through the oracle).  A number is
    present in every map here, so even a kernel that skips NaNs returns an index inside the map."""
    s = _tie_map(5, 6, (7, 20), 40.0)
    for (r, c) in cells:
        s[0, r, c, 0] = np.nan
    idx = _hard_argmax_vs_oracle(eng, s, with_locref)
    assert idx[0, 0].tolist() == list(min(cells))


def test_hard_argmax_nan_across_waves(eng):
    """NaNs held by different threads, lanes and waves of the reduction, with larger numbers around: the lowest index wins each merge."""
    for cells in ((300, 70), (63, 64), (5 + 256, 6), (200, 130, 250)):
        s = _tie_map(20, 26, (1, 400), 40.0)
        for f in cells:
            s[0, f // 26, f % 26, 0] = np.nan
        idx = _hard_argmax_vs_oracle(eng, s, True)
        first = min(cells)
        assert idx[0, 0].tolist() == [first // 26, first % 26]


def test_hard_argmax_all_nan_map(eng):
    """What a 16-bit-tier pass leaves after an overflow and before the engine recovers: index (0, 0) and a NaN probability, as
    np.argmax gives.  (Without a locref tensor: an index outside the map is then only a wrong number, never a read.)"""
    s = np.full((2, 5, 6, 2), np.nan, dtype=np.float32)
    s[1, :, :, 1] = -3.0                       # one ordinary map beside them
    s[1, 2, 4, 1] = 0.0
    idx = _hard_argmax_vs_oracle(eng, s, False)
    assert idx.tolist() == [[[0, 0], [0, 0]], [[0, 0], [2, 4]]]


# ---------------------------------------------------------------------------- threshold branch
@pytest.mark.parametrize("shape,gl,th", [((2, 1, 1, 1), 1, 0.3), ((1, 1, 37, 1), 2, 0.3), ((1, 37, 1, 20), 1, 0.3), ((2, 6, 7, 20), 1, 0.3),
                                         ((1, 1, 37, 20), 1, 1.5), ((2, 6, 7, 1), 2, 1.5), ((1, 1, 1, 1), 1, 1.5)])
def test_threshold_branch_on_small_maps_and_strided_columns(eng, shape, gl, th):
    """pmap_threshold_kernel on maps of 1 and 37 cells (fewer than its 256 threads) and on C = 20 (a map is a strided column of the
    tensor).  th = 1.5 cuts everything: the fp32 reference divides 0 by 0, and where it gives NaN the kernel must too."""
    from oracle import dgp_oracle as O
    s = (3.0 * np.random.default_rng(29).standard_normal(shape)).astype(np.float32)
    with np.errstate(all="ignore"):
        mu_ref, pm_ref = O.argmax_2d_from_cm(s, 1.0, gl, th=th)
        mu64, pm64 = O.argmax_2d_from_cm(s, 1.0, gl, dtype=np.float64, th=th)
        _, pm_plain = O.argmax_2d_from_cm(s, 1.0, gl, dtype=np.float64)
    mu, conf, idx, pmap = eng.soft_argmax(torch.from_numpy(s).cuda(), 1.0, gl, want_pmap=True)
    mu_t = eng.pmap_threshold(pmap, th).cpu().numpy()
    pmap = pmap.cpu().numpy()
    if th > 1.0:
        assert np.isnan(mu_ref).all() and np.isnan(pm_ref).all()
        assert np.array_equal(np.isnan(mu_t), np.isnan(mu_ref)) and np.array_equal(np.isnan(pmap), np.isnan(pm_ref))
        np.testing.assert_allclose(mu_t, mu_ref, equal_nan=True)
        return
    cut = pm_plain.max(axis=(1, 2), keepdims=True) * th
    assert (np.abs(pm_plain - cut) / cut).min() > 1e-5              # no cell sits on the threshold: the kept set is well defined
    assert np.array_equal(pm_ref > 0, pm64 > 0) and np.array_equal(pmap > 0, pm64 > 0)
    assert np.abs(pmap - pm_ref).max() < PMAP_TOL and np.abs(pmap - pm64).max() < PMAP_TOL
    assert np.abs(mu_t - mu64).max() * STRIDE < PX_TOL and np.abs(mu_t - mu_ref).max() * STRIDE < PX_TOL


@pytest.mark.parametrize("th", [0.3, 1.0])
@pytest.mark.parametrize("H,W,C", [(1, 1, 1), (1, 37, 1), (37, 1, 20), (9, 8, 20)])
def test_threshold_branch_keeps_a_flat_map(eng, H, W, C, th):
    """A flat map: max * th <= every value up to th = 1 (the comparison is `<`), so nothing is cut, the map is unchanged and mu is
    the centre of the grid."""
    p = np.full((2, H, W, C), 1.0 / (H * W), dtype=np.float32)
    pmap = torch.from_numpy(p).cuda()
    mu = eng.pmap_threshold(pmap, th).cpu().numpy()
    assert np.abs(pmap.cpu().numpy().astype(np.float64) - 1.0 / (H * W)).max() < PMAP_TOL
    assert np.abs(mu - np.array([(H - 1) / 2.0, (W - 1) / 2.0])).max() * STRIDE < PX_TOL
