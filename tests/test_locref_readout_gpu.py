"""The fused locref read-out at layer level (dgp_ops.hip: soft_argmax_kernel<LARGE, LOCREF = true>; dgp_soft_argmax_locref).

Reference: oracle.dgp_oracle.argmax_2d_from_cm(..., dtype=float64)'s normalised map times the locref field, summed in float64 -- the
expectation of the raw field under the map mu is the expectation under.  Gate: the suite's 1e-3 px, on the refined coordinate
mu * 8 + 4 + offs * 7.2801 against float64 (on exactly these inputs the fp32 reference sits 5e-7 .. 1.2e-6 px from float64 in the
offset term; asserted, as in test_readout_edges_gpu.py, to stay within a tenth of the gate).

Every case also asserts that mu, conf, idx and pmap keep soft_argmax's bits, and that the LDS instance and the streaming one
(DGP_SOFTARGMAX_STREAM=1, read per call) agree bit for bit, offs included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PX_TOL = 1e-3          # px
STRIDE, STDEV = 8.0, 7.2801

# (B, H, W, C), gauss_len, gamma: odd C (a wrong 2C stride or pair index), B = 2 (the batch stride), maps smaller than the blur and of
# fewer than 64 cells, H W not a multiple of the 1024 threads
CASES = [((2, 3, 2, 3), 7, 1.0), ((1, 1, 9, 1), 5, 1.0), ((1, 9, 1, 2), 6, 3.0), ((2, 13, 11, 3), 1, 0.25), ((2, 13, 11, 3), 2, 1.0),
         ((1, 33, 37, 1), 3, 1.0), ((1, 60, 80, 2), 1, 1.0)]


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return engine


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _inputs(shape, seed=31):
    rng = np.random.default_rng(seed)
    B, H, W, C = shape
    s = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    l = (2.0 * rng.standard_normal((B, H, W, 2 * C))).astype(np.float32)
    return s, l


def _expected_offsets(pmap, locref, dtype=np.float64):
    """sum over the map of pmap [B,H,W,C] * locref [B,H,W,C,2] -> [B,C,2], in `dtype`"""
    B, H, W, C = pmap.shape
    lr = locref.reshape(B, H, W, C, 2).astype(dtype)
    return (pmap.astype(dtype)[..., None] * lr).sum(axis=(1, 2), dtype=dtype)


def _refined_px(mu, offs):
    return np.asarray(mu, np.float64) * STRIDE + 0.5 * STRIDE + np.asarray(offs, np.float64) * STDEV


def _locref_both(eng, monkeypatch, s, l, gamma, gl):
    """soft_argmax_locref on both kernel instances (bit identity asserted, offs included) and soft_argmax beside it (mu, conf, idx, pmap
    bit-identical); -> (mu, conf, idx, offs, pmap) as numpy"""
    st, lt = torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda()
    monkeypatch.delenv("DGP_SOFTARGMAX_STREAM", raising=False)
    lds = [x.clone() for x in eng.soft_argmax_locref(st, lt, gamma, gl, want_pmap=True)]
    plain = [x.clone() for x in eng.soft_argmax(st, gamma, gl, want_pmap=True)]
    monkeypatch.setenv("DGP_SOFTARGMAX_STREAM", "1")
    stream = eng.soft_argmax_locref(st, lt, gamma, gl, want_pmap=True)
    monkeypatch.delenv("DGP_SOFTARGMAX_STREAM")
    for a, b, name in zip(lds, stream, ("mu", "conf", "idx", "offs", "pmap")):
        assert torch.equal(_bits(a), _bits(b)), ("LDS vs streaming", name, s.shape, gl, gamma)
    for a, b, name in zip([lds[0], lds[1], lds[2], lds[4]], plain, ("mu", "conf", "idx", "pmap")):
        assert torch.equal(_bits(a), _bits(b)), ("locref vs plain instance", name, s.shape, gl, gamma)
    nop = eng.soft_argmax_locref(st, lt, gamma, gl)                # without the map: the same four outputs
    for a, b in zip(lds[:4], nop):
        assert torch.equal(_bits(a), _bits(b))
    return [x.cpu().numpy() for x in lds]


@pytest.mark.parametrize("shape,gl,gamma", CASES)
def test_expected_offset_against_float64(eng, monkeypatch, shape, gl, gamma):
    from oracle import dgp_oracle as O
    s, l = _inputs(shape)
    mu64, pm64 = O.argmax_2d_from_cm(s, gamma, gl, dtype=np.float64)
    mu32, pm32 = O.argmax_2d_from_cm(s, gamma, gl)
    off64 = _expected_offsets(pm64, l)
    off32 = _expected_offsets(pm32, l, np.float32)
    ref_err = np.abs(_refined_px(mu32, off32) - _refined_px(mu64, off64)).max()
    off_err = np.abs(off32.astype(np.float64) - off64).max() * STDEV
    print("fp32 reference vs float64: refined %.3g px (offset term %.3g px)" % (ref_err, off_err))
    assert ref_err < PX_TOL / 10                                   # the reference alone stands well inside the gate
    mu, conf, idx, offs, pmap = _locref_both(eng, monkeypatch, s, l, gamma, gl)
    err = np.abs(_refined_px(mu, offs) - _refined_px(mu64, off64)).max()
    print("HIP vs float64: refined %.3g px (offset term %.3g px)" % (err, np.abs(offs - off64).max() * STDEV))
    assert offs.shape == (shape[0], shape[3], 2) and offs.dtype == np.float32
    assert err < PX_TOL


@pytest.mark.parametrize("shape,gl,gamma", [CASES[0], CASES[4], CASES[6]])
def test_constant_field_comes_back(eng, monkeypatch, shape, gl, gamma):
    """A constant field's expectation is the constant, whatever the map: offs == c to 1e-6 relative (per channel: dx and dy differ)."""
    s, _ = _inputs(shape)
    B, H, W, C = shape
    c = np.linspace(-3.5, 4.25, 2 * C).astype(np.float32)
    l = np.broadcast_to(c, (B, H, W, 2 * C)).copy()
    offs = _locref_both(eng, monkeypatch, s, l, gamma, gl)[3]
    np.testing.assert_allclose(offs, np.broadcast_to(c.reshape(C, 2), (B, C, 2)), rtol=1e-6, atol=0)


def test_saturated_map_gives_the_stamp_weighted_mean(eng, monkeypatch):
    """Logits -1e4 with one cell at 1e4, gauss_len 1: the softmax is one-hot, the blurred map is the 3 x 3 stamp outer(g, g) around the
    cell (interior: 0.0751 / 0.1238 / 0.2042; at a corner the clipped stamp, renormalised), and offs its weighted mean of the field."""
    from oracle import dgp_oracle as O
    H, W, C = 6, 7, 2
    peaks = [(2, 3), (5, 6)]                                       # an interior cell and the corner
    s = np.full((1, H, W, C), -1e4, dtype=np.float32)
    for j, (h, w) in enumerate(peaks):
        s[0, h, w, j] = 1e4
    l = _inputs((1, H, W, C), seed=5)[1]
    g = O.gaussian_taps(1, dtype=np.float64)
    k2 = np.outer(g, g)
    np.testing.assert_allclose([k2[0, 0], k2[0, 1], k2[1, 1]], [0.0751, 0.1238, 0.2042], atol=5e-5)
    want = np.zeros((1, C, 2))
    for j, (h, w) in enumerate(peaks):
        tot = 0.0
        for a in range(-1, 2):
            for b in range(-1, 2):
                if 0 <= h + a < H and 0 <= w + b < W:
                    want[0, j] += k2[a + 1, b + 1] * l[0, h + a, w + b, 2 * j:2 * j + 2].astype(np.float64)
                    tot += k2[a + 1, b + 1]
        want[0, j] /= tot
    mu, conf, idx, offs, pmap = _locref_both(eng, monkeypatch, s, l, 1.0, 1)
    assert np.abs(offs - want).max() * STDEV < PX_TOL
    # tighter than the gate: the kernel's taps and map are fp32 (each weight within ~4 ulp = 2.4e-7 relative of the float64 stamp), the
    # field is below 8 in magnitude, and numerator and denominator each carry that error: 8 * 2 * 2.4e-7 < 5e-6
    np.testing.assert_allclose(offs, want, rtol=0, atol=5e-6)
    np.testing.assert_allclose(mu[0, 0], [2.0, 3.0], atol=1e-6)


def test_plus_inf_logit_gives_nan_offsets_without_a_fault(eng, monkeypatch):
    """+inf in joint 0: mu is NaN, the window index is (0, 0) inside the map, offs is NaN; joint 1 of the same frame does not notice."""
    s, l = _inputs((1, 6, 7, 2))
    base = _locref_both(eng, monkeypatch, s, l, 1.0, 2)
    s[0, 1, 5, 0] = np.inf
    mu, conf, idx, offs, pmap = _locref_both(eng, monkeypatch, s, l, 1.0, 2)
    assert np.isnan(mu[0, 0]).all() and np.isnan(offs[0, 0]).all()
    assert idx[0, 0].tolist() == [0, 0]
    for got, ref in zip((mu, conf, idx, offs), base[:4]):
        np.testing.assert_array_equal(got[0, 1], ref[0, 1])
    torch.cuda.synchronize()


def test_rejections(eng):
    from deepgraphpose_amd import _lib
    z = torch.zeros((1, 6, 6, 2), dtype=torch.float32, device="cuda")
    l = torch.zeros((1, 6, 6, 4), dtype=torch.float32, device="cuda")
    for gl in (0, 8):
        with pytest.raises(_lib.DgpError, match="gauss_len must be 1..7"):
            eng.soft_argmax_locref(z, l, 1.0, gl)
    with pytest.raises(_lib.DgpError, match="null argument"):
        eng.soft_argmax_locref(z, None, 1.0, 1)
    with pytest.raises(_lib.DgpError):
        eng.soft_argmax_locref(z, l[..., :3].contiguous(), 1.0, 1)      # not [B,H,W,2C]
    mu, conf, idx, offs = eng.soft_argmax_locref(z[:0], l[:0], 1.0, 1)  # no frames: empty outputs
    assert offs.shape == (0, 2, 2)
