"""The augmentation pipeline as a plan drawn first and applied afterwards (deepgraphpose_amd/augment.py), and the float64 restatements
(tests/_aug_ref.py) the device kernels are held to.  No GPU."""
import numpy as np
import pytest

import _aug_ref as R

SHAPES = [(37, 53), (64, 96)]
SEEDS = list(range(8))


def _keypoints(H, W, seed):
    rng = np.random.default_rng(seed)
    kp = np.stack([rng.uniform(0, W - 1, 4), rng.uniform(0, H - 1, 4)], -1)
    kp[2] = np.nan                                              # an unlabeled joint
    return [tuple(v) for v in kp.tolist()]


def _same_rng(a, b):
    sa, sb = a.rng.get_state(), b.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def _same_params(a, b, skip=()):
    assert sorted(a) == sorted(b)
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


@pytest.mark.parametrize("hw", SHAPES)
def test_plan_then_apply_is_the_pipeline_before_the_split(hw):
    """8 seeds, two frames per call, keypoints with a NaN joint: apply_host(plan(...)) and __call__ both equal the monolithic pipeline
    (tests/_aug_parent.py) in images, keypoints and the RNG states left behind"""
    from _aug_parent import MonolithicAugPipeline
    from deepgraphpose_amd.augment import STAGES, NumpyAugPipeline
    H, W = hw
    fired = set()
    for seed in SEEDS:
        images = np.stack([R.pattern_frame(H, W, seed), R.pattern_frame(H, W, seed + 100)])
        kps = [_keypoints(H, W, seed), _keypoints(H, W, seed + 100)]
        old, called, split = MonolithicAugPipeline(0.8, seed=seed), NumpyAugPipeline(0.8, seed=seed), NumpyAugPipeline(0.8, seed=seed)
        want_img, want_kp = old(images=images, keypoints=kps)
        got_img, got_kp = called(images=images, keypoints=kps)
        assert got_img.dtype == np.uint8 and np.array_equal(got_img, want_img)
        assert np.array_equal(np.array(got_kp), np.array(want_kp), equal_nan=True)
        _same_rng(called, old)
        assert called.bulk.bit_generator.state == old.bulk.bit_generator.state
        for i in range(2):
            plan = split.plan(H, W, noise="field")
            fired.update(s for s, _ in plan)
            img, kp = split.apply_host(plan, images[i], kps[i])
            assert np.array_equal(img, want_img[i]), (seed, i, [s for s, _ in plan])
            assert np.array_equal(kp, np.array(want_kp[i]), equal_nan=True), (seed, i)
            assert np.isnan(kp[2]).all() and np.isfinite(kp[[0, 1, 3]]).all()
        _same_rng(split, old)
        assert len(called.last_plans) == 2
    assert fired == set(STAGES)                                 # every stage took part


@pytest.mark.parametrize("hw", SHAPES)
def test_key_and_field_plans_share_every_draw_but_the_noise_source(hw):
    from deepgraphpose_amd.augment import NumpyAugPipeline
    H, W = hw
    noisy = 0
    for seed in SEEDS:
        a, b = NumpyAugPipeline(0.8, seed=seed), NumpyAugPipeline(0.8, seed=seed)
        for _ in range(3):
            pf, pk = a.plan(H, W, noise="field"), b.plan(H, W, noise="key")
            assert [s for s, _ in pf] == [s for s, _ in pk]
            for (stage, x), (_, y) in zip(pf, pk):
                _same_params(x, y, skip=("field", "key") if stage == "gaussian_noise" else ())
                if stage == "gaussian_noise":
                    noisy += 1
                    assert x["key"] is None and x["field"].shape == (H, W, 3 if x["per_channel"] else 1) and x["field"].dtype == np.float32
                    assert y["field"] is None and isinstance(y["key"], int) and 0 <= y["key"] < 2 ** 64
            _same_rng(a, b)
    assert noisy > 0
    with pytest.raises(ValueError):
        a.plan(H, W, noise="device")


@pytest.mark.parametrize("hw", SHAPES)
def test_keypoints_of_is_apply_hosts_keypoint_half(hw):
    from deepgraphpose_amd.augment import NumpyAugPipeline, keypoints_of
    H, W = hw
    for seed in SEEDS:
        p = NumpyAugPipeline(0.8, seed=seed)
        plan = p.plan(H, W, noise="field")
        kps = _keypoints(H, W, seed)
        _, kp = p.apply_host(plan, R.pattern_frame(H, W, seed), kps)
        assert np.array_equal(keypoints_of(plan, kps, H, W), kp, equal_nan=True)
        q = NumpyAugPipeline(0.8, seed=seed)                     # the device's plan moves the labels alike
        assert np.array_equal(keypoints_of(q.plan(H, W, noise="key"), kps, H, W), kp, equal_nan=True)


def test_plan_aug_gives_data_augs_labels():
    """augment.plan_aug: data_aug's draws in data_aug's order, its labels bit for bit, no pixels"""
    from deepgraphpose_amd.augment import NumpyAugPipeline, data_aug, plan_aug, plan_stages

    class Cfg:
        stride = 8.0
    H, W = 64, 96
    batch = np.stack([R.pattern_frame(H, W, s) for s in range(5)])
    jl = np.array([[[3.0, 4.0], [5.0, 6.0], [np.nan, np.nan]], [[1.0, 9.0], [np.nan, np.nan], [6.5, 2.25]]])
    for seed in SEEDS:
        a, b = NumpyAugPipeline(0.8, seed=seed), NumpyAugPipeline(0.8, seed=seed)
        _, want = data_aug(batch, [1, 3], jl, a, Cfg)
        plans, got = plan_aug(2, H, W, jl, b, Cfg)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
        assert plan_stages(plans) == plan_stages(a.last_plans)
        _same_rng(a, b)


def _rotation(deg, H, W):
    from deepgraphpose_amd.augment import rotate_coefficients
    return rotate_coefficients(deg, H, W)[0]


def _pil_affine(img, coef):
    from PIL import Image
    H, W = img.shape[:2]
    return np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, coef, resample=Image.BILINEAR))


def test_affine_restatement_is_pillow_byte_for_byte():
    frame = R.reaching_frame()
    assert frame.shape == (747, 832, 3)
    crop = np.ascontiguousarray(frame[300:337, 400:453])
    cases = [(frame, d) for d in (-10.0, -3.3, 0.0, 7.77, 10.0)] + [(crop, d) for d in (-9.5, 4.2)]
    for img, deg in cases:
        H, W = img.shape[:2]
        coef = _rotation(deg, H, W)
        want = _pil_affine(img, coef)
        assert np.array_equal(R.pil_affine_bilinear(img, coef), want), (img.shape, deg)
    assert (want[0, 0] == 0).all() or (want[-1, 0] == 0).all()           # (a corner left the image)
    for img in (crop, R.pattern_frame(5, 7)):                   # fliplr as an affine map: an exact permutation
        H, W = img.shape[:2]
        flip = (-1.0, 0.0, float(W), 0.0, 1.0, 0.0)
        assert np.array_equal(_pil_affine(img, flip), img[:, ::-1]) and np.array_equal(R.pil_affine_bilinear(img, flip), img[:, ::-1])
    # a sample position exactly on the right / lower border is outside: Pillow fills it
    img = R.pattern_frame(6, 9)
    for coef in ((1, 0, 0.5, 0, 1, 0), (1, 0, 0, 0, 1, 0.5), (1, 0, -0.5, 0, 1, -0.5)):
        assert np.array_equal(R.pil_affine_bilinear(img, coef), _pil_affine(img, coef)), coef


def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10"""
    vectors = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
               ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in vectors:
        got = R.philox4x32_10(np.array(ctr, dtype=np.uint64), key)
        assert " ".join("%08x" % int(v) for v in got) == want
    both = R.philox4x32_10(np.array([vectors[0][0], vectors[0][0]], dtype=np.uint64), (0, 0))      # (vectorised over counters)
    assert both.shape == (2, 4) and np.array_equal(both[0], both[1])


def test_restated_noise_has_the_stages_distribution():
    """a 64 x 96 frame of 128 at scale 2.55, per channel: mean within 4 sigma / sqrt(n) = 0.08 (n = 18 432), standard deviation within
    3 % of sqrt(2.55^2 + 1/12) (the rounding to bytes adds a uniform's variance)"""
    img = np.full((64, 96, 3), 128, dtype=np.uint8)
    out = R.noise_u8(img, 2.55, True, 0x0123456789ABCDEF).astype(np.float64) - 128.0
    assert abs(out.mean()) <= 0.08
    assert abs(out.std() / np.sqrt(2.55 ** 2 + 1 / 12.0) - 1.0) <= 0.03
    z = R.noise_z64(64, 96, True, 0x0123456789ABCDEF)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.9      # u >= 2^-25: |z| <= sqrt(50 ln 2)
    one = R.noise_z64(64, 96, False, 7)
    assert one.shape == (64, 96, 1) and not np.array_equal(one[..., 0], z[..., 0])
    same = R.noise_u8(img, 2.55, False, 7)
    assert np.array_equal(same[..., 0], same[..., 1]) and np.array_equal(same[..., 0], same[..., 2])


def test_elastic_restatement_against_the_host_stage():
    """the host's fp32 stage (torch interpolate + grid_sample) against the float64 restatement under the same draws: no byte further
    than 1 from rint(v64), at most 1e-3 of the bytes differ"""
    from deepgraphpose_amd.augment import NumpyAugPipeline, apply_elastic
    frame = R.reaching_frame()
    noise = np.random.default_rng(5).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    for k, img in enumerate((frame, np.ascontiguousarray(frame[300:337, 400:453]), noise)):
        H, W = img.shape[:2]
        params = NumpyAugPipeline(1.0, seed=k).draw_elastic(H, W)
        assert params["field"].shape == (2, -(-(H - 1) // 4) + 1, -(-(W - 1) // 4) + 1) and params["field"].dtype == np.float32
        host, _ = apply_elastic(img, np.zeros((0, 2)), params)
        v64 = R.elastic_f64(img, params["field"])
        want = np.clip(np.rint(v64), 0, 255)
        diff = np.abs(host.astype(np.float64) - want)
        assert diff.max() <= 1, (img.shape, diff.max())
        assert (diff > 0).mean() <= 1e-3, (img.shape, (diff > 0).mean())
        assert not np.array_equal(host, img)


def test_the_drivers_refuse_hip_augmentation_off_the_gpu(tmp_path):
    """aug_backend is checked by name before a project is opened, and "hip" against the trainer's device before the first batch"""
    from scripts import fit_feed_digest as D
    from deepgraphpose_amd.models import fitdgp
    assert fitdgp.resolve_aug_backend() == "host" and fitdgp.resolve_aug_backend("hip") == "hip"
    assert fitdgp.resolve_aug_backend("hip", "cuda:0") == "hip" and fitdgp.resolve_aug_backend("host", "cpu") == "host"
    for call in (fitdgp.fit_dgp, fitdgp.fit_dgp_labeledonly):
        with pytest.raises(ValueError, match="aug backend"):
            call(D.START, str(tmp_path / "nowhere"), aug_backend="auto")
    with pytest.raises(ValueError, match="aug_backend='hip'"):
        D.run_case("dgp_aug", tmp_path, depth=0, call=lambda F, proj: F.fit_dgp(D.START, proj, batch_size=4, maxiters=6, gm2=1, gm3=3,
                                                                                 n_max_frames=30, ns=3, aug_backend="hip"))
    assert not D.RecordingSession.digests
    rec = D.run_case("labeledonly", tmp_path, depth=0)           # the default: the host path, with its statistics
    assert len(rec["digests"]) == 6 and fitdgp.PREP_STATS["aug"]["backend"] == "host" and fitdgp.PREP_STATS["aug"]["frames"] == 6
