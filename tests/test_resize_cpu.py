"""The resize contract on the host: the numpy restatement of Pillow's 8-bit bicubic resample (tests/_pil_resample_ref.py) gives Pillow's
bytes, and the C-ABI's coefficient tables (dgp_resize_plan, host only) are the restatement's integers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _pil_resample_ref as R  # noqa: E402

# every axis of the seven shapes, plus the sizes videos are run at
AXIS_PAIRS = sorted({(a, b) for (H, W), (oh, ow) in R.SHAPES for a, b in ((H, oh), (W, ow))} |
                    {(1280, 640), (720, 360), (832, 640), (747, 480)})


@pytest.mark.parametrize("src,dst", R.SHAPES, ids=lambda v: "%dx%d" % v)
def test_restatement_is_pillow_byte_for_byte(src, dst):
    """also pins the installed Pillow's default filter: Image.resize(size=...) without `resample` is BICUBIC"""
    from PIL import Image
    (H, W), (oh, ow) = src, dst
    x = R.test_image(H, W)
    want = np.asarray(Image.fromarray(x).resize(size=(ow, oh)))
    got = R.resize(x, oh, ow)
    assert got.shape == want.shape == (oh, ow, 3)
    assert np.array_equal(got, want), int((got != want).sum())


def test_restatement_crop_is_pillow_with_zeros_outside():
    from PIL import Image
    x = R.test_image(97, 131)
    for new_size, box in (((72, 96), (-4, -3, 50, 40)), (None, (8, 16, 136, 112)), ((72, 96), (90, 60, 110, 80))):
        im = Image.fromarray(x)
        if new_size is not None:
            im = im.resize(size=(new_size[1], new_size[0]))
        want = np.asarray(im.crop(box))
        assert np.array_equal(R.resize_crop(x, new_size, box), want), (new_size, box)


def _plan(lib, n_in, n_out):
    ks = C.c_int32(-1)
    rc = lib.dgp_resize_plan_size(n_in, n_out, C.byref(ks))
    if rc != 0:
        return rc, ks.value, None, None
    bounds = np.full((n_out, 2), -7, np.int32)
    coeffs = np.full((n_out, ks.value), -7, np.int32)
    rc = lib.dgp_resize_plan(n_in, n_out, bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p))
    return rc, ks.value, bounds, coeffs


@pytest.mark.parametrize("n_in,n_out", AXIS_PAIRS)
def test_plan_equals_restatement(lib_built, n_in, n_out):
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    rc, ks, bounds, coeffs = _plan(lib, n_in, n_out)
    assert rc == 0, lib.dgp_last_error()
    ks_ref, bounds_ref, coeffs_ref = R.plan(n_in, n_out)
    assert ks == ks_ref
    assert np.array_equal(bounds, bounds_ref)
    assert np.array_equal(coeffs, coeffs_ref)
    # Pillow's tables: every window inside the input, every row of weights sums to 1 within the rounding of its taps
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ks).all()
    assert np.abs(coeffs.sum(1, dtype=np.int64) - (1 << 22)).max() <= ks


def test_plan_of_equal_sizes_is_the_identity(lib_built):
    from deepgraphpose_amd import _lib
    rc, ks, bounds, coeffs = _plan(_lib.load(), 48, 48)
    assert rc == 0 and ks == 5
    for xx in range(48):
        x0, n = bounds[xx]
        taps = {int(x0 + i): int(coeffs[xx, i]) for i in range(n) if coeffs[xx, i]}
        assert taps == {xx: 1 << 22}, (xx, taps)


@pytest.mark.parametrize("n_in,n_out", [(0, 8), (8, 0), (-3, 8), (8, -1), (0, 0), ((1 << 24) + 1, 8)])
def test_plan_rejects_bad_sizes(lib_built, n_in, n_out):
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    ks = C.c_int32(-1)
    assert lib.dgp_resize_plan_size(n_in, n_out, C.byref(ks)) == -1 and lib.dgp_last_error()
    buf = np.zeros(64, np.int32)
    assert lib.dgp_resize_plan(n_in, n_out, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == -1
    assert lib.dgp_resize_plan(8, 4, None, None) == -1


def test_resize_symbols_are_declared_and_bound(lib_built):
    from deepgraphpose_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dgp_hip.h")).read()
    for name in ("dgp_resize_plan_size", "dgp_resize_plan", "dgp_resize_crop_u8"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)


def test_engine_resize_plan_and_output_shape(lib_built):
    from deepgraphpose_amd import engine
    ks, bounds, coeffs = engine.resize_plan(131, 96)
    ks_ref, bounds_ref, coeffs_ref = R.plan(131, 96)
    assert ks == ks_ref and np.array_equal(bounds, bounds_ref) and np.array_equal(coeffs, coeffs_ref)
    assert engine.resize_output_shape(120, 160) == (120, 160)
    assert engine.resize_output_shape(120, 160, new_size=(72, 96)) == (72, 96)
    assert engine.resize_output_shape(120, 160, crop_size=(8, 16, 136, 112)) == (96, 128)
    assert engine.resize_output_shape(97, 131, (72, 96), (-4, -3, 50, 40)) == (43, 54)


def test_estimate_pose_rejects_unknown_resize_backend(tmp_path):
    """checked before anything is opened: no project, snapshot or GPU is needed to get the error"""
    from deepgraphpose_amd.models.eval import estimate_pose
    with pytest.raises(ValueError, match="resize_backend"):
        estimate_pose(str(tmp_path / "cfg.yaml"), str(tmp_path / "snap"), str(tmp_path / "v.npy"), str(tmp_path), resize_backend="opencv")
