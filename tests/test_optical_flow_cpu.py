"""The Farneback flow contract on the host: the float64 restatement (tests/_farneback_ref.py) recovers known translations, the C-ABI's
level plan and parameter checks (dgp_optical_flow_scratch_bytes, host only) agree with it, and learn_wt's HIP backend fails loudly
without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _farneback_ref as F  # noqa: E402

REF_PARAMS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)


def texture_pair(H, W, dx, dy, seed=0, sigma=3.0):
    """Smooth random texture (Gaussian-filtered noise, periodic) and the same texture moved by (dx, dy): next(x) = prev(x - d).
    Sub-pixel moves are exact phase ramps of the band-limited field; both frames are then quantised to uint8 (B = G = R)."""
    rng = np.random.default_rng(seed)
    ky, kx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    spec = np.fft.fft2(rng.standard_normal((H, W))) * np.exp(-2 * (np.pi * sigma) ** 2 * (kx ** 2 + ky ** 2))
    base = np.real(np.fft.ifft2(spec))
    scale = 60.0 / base.std()

    def u8(img):
        return np.clip(np.rint(128 + scale * img), 0, 255).astype(np.uint8)[..., None].repeat(3, -1)
    moved = np.real(np.fft.ifft2(spec * np.exp(-2j * np.pi * (kx * dx + ky * dy))))
    return np.stack([u8(base), u8(moved)])


def interior_epe(flow, dx, dy, margin=20):
    e = flow[margin:-margin, margin:-margin] - np.array([dx, dy])
    return np.median(np.hypot(e[..., 0], e[..., 1]))


@pytest.mark.parametrize("dx,dy", [(2.0, 0.0), (0.0, -3.0), (1.5, -2.5), (-4.0, 3.5), (0.5, 0.5), (-1.0, 4.0)])
def test_restatement_recovers_translations(dx, dy):
    fr = texture_pair(128, 160, dx, dy)
    flow = F.farneback(fr, **REF_PARAMS)
    assert flow.shape == (1, 128, 160, 2)
    assert interior_epe(flow[0], dx, dy) <= 0.1
    m = flow[0, 20:-20, 20:-20].reshape(-1, 2).mean(0)
    assert np.all(np.abs(m - [dx, dy]) < 0.1), m          # right sign, right axis


def test_restatement_identical_frames_give_zero():
    """A uniform pair gives exactly zero flow.  A textured frame against itself does not, everywhere: step 5 sends the last row and
    column (floor(x + dx) = w - 1) to the "outside" branch, whose r2, r3 = R0 / 2 seed a small flow there that the box and the
    pyramid spread.  With one pass and no pyramid the flow is exactly zero wherever the box cannot reach that row or column."""
    flat = np.full((3, 48, 64, 3), 117, dtype=np.uint8)
    assert np.all(F.farneback(flat, **REF_PARAMS) == 0.0)
    fr = texture_pair(64, 96, 0.0, 0.0, seed=3)
    r = REF_PARAMS["winsize"] // 2
    flow = F.farneback(np.stack([fr[0], fr[0], fr[0]]), **dict(REF_PARAMS, levels=0, iterations=1))
    assert flow.shape == (2, 64, 96, 2)
    assert np.all(flow[:, :64 - 1 - r, :96 - 1 - r] == 0.0)
    assert np.abs(flow[:, -1, :]).max() > 0 and np.abs(flow[:, :, -1]).max() > 0
    full = F.farneback(np.stack([fr[0], fr[0]]), **REF_PARAMS)
    assert np.abs(full).max() < 0.1


def test_restatement_gray_is_opencv_fixed_point():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [10, 200, 77]]], dtype=np.uint8)
    assert F.gray(px).tolist() == [[29.0, 150.0, 76.0, 255.0, 0.0 + ((1868 * 10 + 9617 * 200 + 4899 * 77 + 8192) >> 14)]]


def _scratch(lib, T, H, W, **kw):
    from deepgraphpose_amd import _lib
    p = dict(REF_PARAMS, flags=0)
    p.update(kw)
    prm = _lib.DgpFlowParams(p["pyr_scale"], p["levels"], p["winsize"], p["iterations"], p["poly_n"], p["poly_sigma"], p["flags"])
    nb, used = C.c_size_t(0), C.c_int32(-1)
    rc = lib.dgp_optical_flow_scratch_bytes(T, H, W, C.byref(prm), C.byref(nb), C.byref(used))
    return rc, nb.value, used.value


@pytest.mark.parametrize("W,H,levels", [(640, 480, 3), (832, 747, 3), (96, 64, 1), (40, 36, 0)])
def test_scratch_bytes_level_plan_matches_restatement(lib_built, W, H, levels):
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    rc, nb, used = _scratch(lib, 11, H, W)
    assert rc == 0, lib.dgp_last_error()
    plan = F.plan(H, W, 0.5, 3)
    assert used == levels == len(plan) - 1
    assert nb >= 4 * 11 * H * W * (1 + 1 + 5) + 4 * 10 * H * W * (2 + 2 + 5 + 5)
    if (W, H) == (832, 747):
        assert [(w, h) for _, w, h, _, _ in plan[1:]] == [(416, 374), (208, 187), (104, 93)]


@pytest.mark.parametrize("bad", [dict(poly_n=6), dict(winsize=14), dict(winsize=33), dict(flags=1), dict(flags=256),
                                 dict(pyr_scale=1.0), dict(pyr_scale=0.0), dict(levels=-1), dict(iterations=0), dict(poly_sigma=0.0)])
def test_scratch_bytes_rejects_bad_parameters(lib_built, bad):
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    rc, _, _ = _scratch(lib, 4, 64, 96, **bad)
    assert rc == -1 and lib.dgp_last_error()


def test_scratch_bytes_rejects_small_frames(lib_built):
    from deepgraphpose_amd import _lib
    lib = _lib.load()
    assert _scratch(lib, 4, 15, 15)[0] == -1
    assert _scratch(lib, 4, 15, 64)[0] == -1
    assert _scratch(lib, 1, 64, 64)[0] == -1
    assert _scratch(lib, 2, 16, 16) == (0, _scratch(lib, 2, 16, 16)[1], 0)


def test_flow_symbols_are_declared_and_bound(lib_built):
    from deepgraphpose_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dgp_hip.h")).read()
    for name in ("dgp_optical_flow_scratch_bytes", "dgp_optical_flow"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)


def test_learn_wt_hip_fails_loudly_without_gpu(lib_built, monkeypatch):
    import torch
    from deepgraphpose_amd import _lib
    from deepgraphpose_amd.models import fitdgp_util as U
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    batch = np.zeros((3, 32, 32, 3), dtype=np.uint8)
    with pytest.raises(_lib.DgpError):
        U.learn_wt(batch, backend="hip")
    with pytest.raises(ValueError):
        U.learn_wt(batch, backend="numpy")
    monkeypatch.setattr(U, "_cv2_available", lambda: False)
    with pytest.raises(ImportError) as e:
        U.learn_wt(batch)                     # auto: neither cv2 nor a GPU
    assert "cv2" in str(e.value) and "HIP" in str(e.value)
