"""The device augmenters (csrc/dgp_augment.hip, engine.aug_* and engine.augment_frames), each under a host-drawn plan: five stages byte
for byte against the host stage (augment.apply_<stage>), elastic and noise against their float64 restatements (tests/_aug_ref.py)."""
import numpy as np
import pytest
import torch

import _aug_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(5, 7), (37, 53), (64, 96)]       # a 2 x 3 elastic grid and a 1 x 1 mask; 159-byte rows; more than one workgroup
NO_KP = np.zeros((0, 2))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def reaching():
    return R.reaching_frame()


def _device(plan, img):
    """the plan applied to `img` by engine.augment_frames, as frame 1 of a 3-frame batch whose other frames must not change"""
    from deepgraphpose_amd import engine
    batch = np.stack([np.full_like(img, SENTINEL), img, np.full_like(img, SENTINEL)])
    dev = torch.from_numpy(batch).to(DEV)
    out = engine.augment_frames(dev, [plan], [1])
    assert out.data_ptr() == dev.data_ptr()
    host = out.cpu().numpy()
    assert (host[[0, 2]] == SENTINEL).all()
    return host[1]


def _host(stage, img, params):
    from deepgraphpose_amd import augment
    return np.ascontiguousarray(getattr(augment, "apply_" + stage)(img, NO_KP, params)[0])


def _exact(stage, img, params):
    got, want = _device([(stage, params)], img), _host(stage, img, params)
    assert got.shape == want.shape and np.array_equal(got, want), (stage, img.shape, int((got != want).sum()))
    return got


def _pipeline(seed, p=1.0):
    from deepgraphpose_amd.augment import NumpyAugPipeline
    return NumpyAugPipeline(p, seed=seed)


def _rotation(deg, H, W):
    from deepgraphpose_amd.augment import rotate_coefficients
    return {"deg": deg, "coef": rotate_coefficients(deg, H, W)[0]}


def _blur(deg):
    from deepgraphpose_amd.augment import motion_blur_kernel
    return {"kernel": motion_blur_kernel(deg)}


def _crop(fractions, H, W):
    from deepgraphpose_amd.augment import crop_amounts
    return {"amounts": crop_amounts(*fractions, H, W)}


CROPS = [(-0.3, -0.3, -0.3, -0.3), (0.1, 0.1, 0.1, 0.1), (-0.3, 0.1, 0.06, -0.12), (0.001, -0.002, 0.003, -0.001)]


# ---- byte-exact against the host stage -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SHAPES)
def test_fliplr_and_rotate_are_the_host_stages_bytes(lib_built, hw):
    H, W = hw
    img = R.pattern_frame(H, W)
    got = _exact("fliplr", img, {"flip": True})
    assert np.array_equal(got, img[:, ::-1])
    assert np.array_equal(_device([("fliplr", {"flip": False})], img), img)
    drawn = _pipeline(H).draw_rotate(H, W)
    assert -10 <= drawn["deg"] <= 10
    for params in (_rotation(10.0, H, W), _rotation(-10.0, H, W), _rotation(0.0, H, W), drawn):
        got = _exact("rotate", img, params)
        if abs(params["deg"]) == 10.0 and H > 5:
            assert (got[0, 0] == 0).all() or (got[0, -1] == 0).all()            # a corner left the image
    assert np.array_equal(_device([("rotate", _rotation(0.0, H, W))], img), img)


@pytest.mark.parametrize("hw", SHAPES)
def test_motion_blur_is_the_host_stages_bytes(lib_built, hw):
    H, W = hw
    img = R.pattern_frame(H, W)
    for params in (_blur(0.0), _blur(45.0), _blur(90.0), _blur(-90.0), _pipeline(W).draw_motion_blur(H, W)):
        assert params["kernel"].dtype == np.float32 and abs(float(params["kernel"].sum()) - 1) < 1e-6
        _exact("motion_blur", img, params)


@pytest.mark.parametrize("hw", SHAPES)
def test_coarse_dropout_is_the_host_stages_bytes(lib_built, hw):
    H, W = hw
    img = np.maximum(R.pattern_frame(H, W), 1)                  # (no zero byte of its own)
    assert np.array_equal(_exact("coarse_dropout", img, {"mask": np.zeros((1, 1), bool)}), img)
    assert not _exact("coarse_dropout", img, {"mask": np.ones((1, 1), bool)}).any()
    assert np.array_equal(_exact("coarse_dropout", img, {"mask": np.zeros((2, 3), bool)}), img)
    assert not _exact("coarse_dropout", img, {"mask": np.ones((2, 3), bool)}).any()
    mixed = np.array([[True, False, False], [False, True, True]])
    got = _exact("coarse_dropout", img, {"mask": mixed})
    assert 0 < (got == 0).all(-1).mean() < 1
    drawn = _pipeline(3).draw_coarse_dropout(H, W)
    assert drawn["mask"].dtype == bool and 1 <= drawn["mask"].shape[0] <= max(1, round(H * 0.05))
    _exact("coarse_dropout", img, drawn)


@pytest.mark.parametrize("hw", SHAPES)
def test_crop_and_pad_is_the_host_stages_bytes(lib_built, hw):
    H, W = hw
    img = R.pattern_frame(H, W)
    for fractions in CROPS:
        params = _crop(fractions, H, W)
        got = _exact("crop_and_pad", img, params)
        if fractions == CROPS[1] and min(params["amounts"]) > 0:
            assert (got[0] == 0).all() and (got[:, 0] == 0).all()              # the padding is there
    assert _crop(CROPS[3], H, W)["amounts"] == (0, 0, 0, 0)
    assert np.array_equal(_device([("crop_and_pad", _crop(CROPS[3], H, W))], img), img)


def test_exact_stages_on_a_reaching_frame(lib_built, reaching):
    H, W = reaching.shape[:2]
    p = _pipeline(11)
    _exact("fliplr", reaching, {"flip": True})
    _exact("rotate", reaching, p.draw_rotate(H, W))
    _exact("rotate", reaching, _rotation(10.0, H, W))
    _exact("motion_blur", reaching, p.draw_motion_blur(H, W))
    mask = p.draw_coarse_dropout(H, W)["mask"]
    mask[::3, ::4] = True                                        # (p <= 0.02 rarely sets a cell)
    _exact("coarse_dropout", reaching, {"mask": mask})
    _exact("crop_and_pad", reaching, _crop(CROPS[2], H, W))
    _exact("crop_and_pad", reaching, p.draw_crop_and_pad(H, W))


# ---- elastic: within rounding of float64, held to the host's fp32 stage ----------------------------------------------------------------

def _elastic_case(img, field, label):
    params = {"alpha": None, "field": np.ascontiguousarray(field, dtype=np.float32)}
    v64 = R.elastic_f64(img, params["field"])
    want = np.clip(np.rint(v64), 0, 255)
    got = _device([("elastic", params)], img).astype(np.float64)
    host = _host("elastic", img, params).astype(np.float64)
    err, host_err = np.abs(got - v64).max(), np.abs(host - v64).max()
    n, host_n = int((got != want).sum()), int((host != want).sum())
    print("elastic %s %s: max |byte - v64| %.4f (host %.4f), bytes off rint(v64) %d (host %d) of %d"
          % (label, img.shape, err, host_err, n, host_n, got.size))
    assert np.abs(got - want).max() <= 1, label
    assert err <= 2 * host_err, (label, err, host_err)
    assert n <= 2 * host_n + 8, (label, n, host_n)
    return got


@pytest.mark.parametrize("hw", SHAPES)
def test_elastic_is_within_rounding_of_float64(lib_built, hw):
    H, W = hw
    img = R.pattern_frame(H, W)
    p = _pipeline(H + W)
    drawn = p.draw_elastic(H, W)
    assert np.array_equal(_elastic_case(img, np.zeros_like(drawn["field"]), "alpha 0"), img)          # the identity
    got = _elastic_case(img, drawn["field"], "drawn")
    assert not np.array_equal(got, img)
    _elastic_case(img, drawn["field"] * np.float32(10.0 / drawn["alpha"]), "alpha 10")
    if hw == (5, 7):                                            # shifts of several pixels on a 5 x 7 frame: samples leave the image
        rng = np.random.default_rng(0)
        big = rng.uniform(-6, 6, drawn["field"].shape).astype(np.float32)
        got = _elastic_case(img, big, "leaving the image")
        assert (got == 0).all(-1).any()
        _elastic_case(img, np.full_like(big, -1e-7), "a hair left of every pixel")
        _elastic_case(img, np.full_like(big, 100.0), "all outside")


def test_elastic_on_a_reaching_frame(lib_built, reaching):
    H, W = reaching.shape[:2]
    _elastic_case(reaching, _pipeline(2).draw_elastic(H, W)["field"], "reaching")


# ---- noise: Philox4x32-10 + Box-Muller, addressed by the element ------------------------------------------------------------------------

def _noise_case(img, scale, per_channel, key):
    params = {"scale": scale, "per_channel": per_channel, "field": None, "key": key}
    got = _device([("gaussian_noise", params)], img)
    err = np.abs(got.astype(np.float64) - R.noise_f64(img, scale, per_channel, key)).max()
    print("noise %s per_channel %s: max |byte - f64| %.6f" % (img.shape, per_channel, err))
    # fp32 log, sqrt, sinpi / cospi at a few ulp on |z| <= 5.9: 2e-6; times scale <= 2.55 plus one fp32 add below 270: 2e-5; 1e-3 is 30 x that
    assert err <= 0.5 + 1e-3
    return got


@pytest.mark.parametrize("hw", SHAPES)
def test_noise_is_the_restated_stream(lib_built, hw):
    H, W = hw
    img = R.pattern_frame(H, W)
    key = 0x9E3779B97F4A7C15
    a = _noise_case(img, 2.55, True, key)
    b = _noise_case(img, 1.3, False, key)
    delta = b.astype(int) - img
    free = (img > 8).all(-1) & (img < 247).all(-1)              # (no clipping: the three channels move together)
    assert (delta[free][:, 0] == delta[free][:, 1]).all() and (delta[free][:, 0] == delta[free][:, 2]).all()
    assert np.array_equal(a, _noise_case(img, 2.55, True, key))                 # the same key: the same bytes
    assert not np.array_equal(a, _noise_case(img, 2.55, True, key + 1))         # another key: other bytes
    assert not np.array_equal(a, _noise_case(img, 2.55, True, key + (1 << 32)))  # (the high half is part of the key)
    drawn = _pipeline(5).draw_gaussian_noise(H, W, noise="key")
    _noise_case(img, drawn["scale"], drawn["per_channel"], drawn["key"])
    assert np.array_equal(_noise_case(img, 0.0, True, key), img)


def test_noise_on_a_reaching_frame(lib_built, reaching):
    got = _noise_case(reaching, 2.55, True, 12345678901234567890)
    d = got.astype(np.float64) - reaching
    free = (reaching > 16) & (reaching < 239)
    assert abs(d[free].mean()) < 0.02 and abs(d[free].std() / np.sqrt(2.55 ** 2 + 1 / 12.0) - 1) < 0.02
    _noise_case(reaching, 0.7, False, 3)


# ---- the chain -------------------------------------------------------------------------------------------------------------------------

def _exact_plan(seed, H, W):
    """a plan of the five exact stages, every one of them present"""
    p = _pipeline(seed)
    plan = [(s, params) for s, params in p.plan(H, W, noise="key") if s not in ("elastic", "gaussian_noise")]
    assert [s for s, _ in plan] == ["fliplr", "rotate", "motion_blur", "coarse_dropout", "crop_and_pad"][:len(plan)]
    plan[0] = ("fliplr", {"flip": True})
    plan[3][1]["mask"][0, 0] = True
    if len(plan) < 5:                                            # (crop_and_pad has a coin of its own, 0.4)
        plan.append(("crop_and_pad", p.draw_crop_and_pad(H, W)))
    return p, plan


def test_a_chain_of_the_exact_stages_is_apply_host(lib_built):
    from deepgraphpose_amd import engine
    H, W = 37, 53
    batch = np.stack([R.pattern_frame(H, W, s) for s in range(3)])
    (p2, plan2), (p0, plan0) = _exact_plan(1, H, W), _exact_plan(2, H, W)
    assert len(plan2) == len(plan0) == 5
    dev = torch.from_numpy(batch).to(DEV)
    out = engine.augment_frames(dev, [plan2, plan0], [2, 0])
    assert out.data_ptr() == dev.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(got[2], p2.apply_host(plan2, batch[2], NO_KP)[0])
    assert np.array_equal(got[0], p0.apply_host(plan0, batch[0], NO_KP)[0])
    assert np.array_equal(got[1], batch[1]) and not np.array_equal(got[0], batch[0]) and not np.array_equal(got[2], batch[2])
    for k in (2, 3, 4):                                          # shorter chains end in the frame too
        assert np.array_equal(_device(plan2[:k], batch[2]), p2.apply_host(plan2[:k], batch[2], NO_KP)[0]), k
    # all seven: the five exact stages around elastic and noise run, and twice alike
    full = _pipeline(4).plan(H, W, noise="key")
    assert len(full) >= 6
    assert np.array_equal(_device(full, batch[1]), _device(full, batch[1]))


def test_an_empty_plan_launches_nothing(lib_built):
    from deepgraphpose_amd import engine
    H, W = 6, 8                                                  # a shape no other test uses: its scratch frames would be new
    batch = np.stack([R.pattern_frame(H, W, s) for s in range(2)])
    dev = torch.from_numpy(batch).to(DEV)
    for plans, positions in (([[]], [1]), ([[], [("fliplr", {"flip": False})]], [0, 1]), ([], [])):
        assert engine.augment_frames(dev, plans, positions) is dev
    assert np.array_equal(dev.cpu().numpy(), batch)
    assert not any(k[1:] == (H, W) for k in engine._AUG_SCRATCH)


# ---- refusals: on the host, before any launch ------------------------------------------------------------------------------------------

def test_refusals_happen_on_the_host(lib_built):
    from deepgraphpose_amd import engine
    from deepgraphpose_amd._lib import DgpError
    H, W = 5, 7
    img = R.pattern_frame(H, W)
    src = torch.from_numpy(img).to(DEV)
    dst = torch.full((H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    mask = torch.zeros((1, 1), dtype=torch.uint8, device=DEV)
    field = torch.zeros((2, 2, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(DgpError, match="overlap"):
        engine.aug_affine(src, src, ident)                      # src == dst
    two = torch.full((2 * H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(DgpError, match="overlap"):
        engine.aug_blur3(two[1:H + 1], two[:H], np.eye(3, dtype=np.float32) / 3)          # overlapping views
    for bad in (torch.zeros((H + 1, 1), dtype=torch.uint8, device=DEV), torch.zeros((1, W + 1), dtype=torch.uint8, device=DEV)):
        with pytest.raises(DgpError, match="does not belong"):
            engine.aug_dropout(src, dst, bad)
    for bad in (torch.zeros((2, 3, 3), dtype=torch.float32, device=DEV), torch.zeros((2, 2, 2), dtype=torch.float32, device=DEV)):
        with pytest.raises(DgpError, match="does not belong"):
            engine.aug_elastic(src, dst, bad)
    with pytest.raises(DgpError):
        engine.aug_affine(src, dst, (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0))
    thin_s, thin_d = torch.zeros((1, 8, 3), dtype=torch.uint8, device=DEV), torch.full((1, 8, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    for call in (lambda: engine.aug_affine(thin_s, thin_d, ident), lambda: engine.aug_blur3(thin_s, thin_d, np.ones((3, 3), np.float32) / 9),
                 lambda: engine.aug_dropout(thin_s, thin_d, mask), lambda: engine.aug_elastic(thin_s, thin_d, field),
                 lambda: engine.aug_noise(thin_s, thin_d, 1.0, True, 1)):
        with pytest.raises(DgpError, match="at least 2"):       # H < 2
            call()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all() and (thin_d.cpu().numpy() == SENTINEL).all() and (two.cpu().numpy() == SENTINEL).all()
    # the same through augment_frames: a bad table anywhere in the plans stops the call before its first launch
    batch = torch.from_numpy(np.stack([img, img])).to(DEV)
    good = [("fliplr", {"flip": True})]
    p = _pipeline(0)
    for bad in ([("coarse_dropout", {"mask": np.ones((H + 1, 2), bool)})], [("elastic", {"alpha": 1.0, "field": np.zeros((2, 3, 3), np.float32)})]):
        with pytest.raises(DgpError, match="does not belong"):
            engine.augment_frames(batch, [good, bad], [0, 1])
    with pytest.raises(ValueError, match='noise="key"'):
        engine.augment_frames(batch, [good, [("gaussian_noise", p.draw_gaussian_noise(H, W, noise="field"))]], [0, 1])
    with pytest.raises(DgpError):
        engine.augment_frames(batch, [good, good], [0, 0])
    with pytest.raises(DgpError, match="at least 2"):
        engine.augment_frames(torch.zeros((1, 1, 8, 3), dtype=torch.uint8, device=DEV), [good], [0])
    assert np.array_equal(batch.cpu().numpy(), np.stack([img, img]))
