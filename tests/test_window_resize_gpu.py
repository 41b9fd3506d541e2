"""dgp_window_resize_u8 (engine.window_resize) against Pillow applied to the numpy window -- crop_image + imresize (+ np.fliplr) of the
step-0 loader -- byte for byte.  Every window is surrounded by bytes that differ from its border pixels and every case runs twice, the
second time with another surround: the results must be identical, so nothing outside the window reaches the result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pillow(win, scale, mirror):
    from PIL import Image
    from deepgraphpose_amd.dlc_dataset import resized_hw
    oh, ow = resized_hw(win.shape[0], win.shape[1], scale)
    out = np.asarray(Image.fromarray(win).resize((ow, oh), Image.BOX if scale < 1 else Image.BILINEAR))
    return np.fliplr(out) if mirror else out


def _source(H, W, window, flavour):
    """an H x W image: seeded bytes inside the window, and outside it a surround no byte of which equals the nearest window byte"""
    x0, y0, x1, y1 = window
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys, xs = np.clip(np.arange(H), y0, y1), np.clip(np.arange(W), x0, x1)
    nearest = img[ys][:, xs]
    other = (nearest.astype(np.int32) + (97 if flavour == 0 else 181)) % 256
    inside = np.zeros((H, W), bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    out = np.where(inside[..., None], img, other.astype(np.uint8))
    assert (out[~inside] != nearest[~inside]).all()
    return out


def _windows(H, W):
    """origins x0 = 0 .. 3 (every residue of 3 x0 mod 4), inner windows and windows that end on the last row and the last column"""
    for x0 in range(4):
        yield (x0, 1 + x0, W - 6 - x0, H - 4)
        yield (x0, 1 + (x0 * 5) % 7, W - 1, H - 1)


@pytest.mark.parametrize("H,W", [(37, 53), (64, 96)])
@pytest.mark.parametrize("scale", [0.6, 0.75, 0.97, 1.25])
def test_window_resize_is_pillow_on_the_window(lib_built, H, W, scale):
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.dlc_dataset import resized_hw
    filt = "box" if scale < 1 else "bilinear"
    for window in _windows(H, W):
        x0, y0, x1, y1 = window
        srcs = [_source(H, W, window, f) for f in (0, 1)]
        assert np.array_equal(srcs[0][y0:y1 + 1, x0:x1 + 1], srcs[1][y0:y1 + 1, x0:x1 + 1]) and (srcs[0] != srcs[1]).any()
        out_hw = resized_hw(y1 - y0 + 1, x1 - x0 + 1, scale)
        for mirror in (False, True):
            got = [engine.window_resize(torch.from_numpy(s).cuda(), window, out_hw, filt, mirror) for s in srcs]
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
            want = _pillow(np.ascontiguousarray(srcs[0][y0:y1 + 1, x0:x1 + 1]), scale, mirror)
            assert got[0].shape == want.shape == out_hw + (3,)
            assert np.array_equal(got[0], got[1]), (window, mirror, "the surround reached the result")
            assert np.array_equal(got[0], want), (window, mirror, int((got[0] != want).sum()))


def test_three_by_three_window_to_one_pixel(lib_built):
    from deepgraphpose_amd import engine
    for (H, W), window in (((37, 53), (1, 2, 3, 4)), ((37, 53), (50, 34, 52, 36)), ((64, 96), (3, 0, 5, 2))):
        x0, y0, x1, y1 = window
        srcs = [_source(H, W, window, f) for f in (0, 1)]
        for mirror in (False, True):
            got = [engine.window_resize(torch.from_numpy(s).cuda(), window, (1, 1), "box", mirror) for s in srcs]
            torch.cuda.synchronize()
            want = _pillow(np.ascontiguousarray(srcs[0][y0:y1 + 1, x0:x1 + 1]), 0.2, mirror)
            assert want.shape == (1, 1, 3)
            assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want)


def test_whole_image_and_refusals(lib_built):
    from deepgraphpose_amd import _lib, engine
    img = _source(37, 53, (0, 0, 52, 36), 0)
    dev = torch.from_numpy(img).cuda()
    got = engine.window_resize(dev, None, (22, 32), "box")
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), _pillow(img, 0.6, False))
    for window in ((0, 0, 53, 36), (5, 0, 4, 36), (-1, 0, 10, 10)):
        with pytest.raises(_lib.DgpError, match="window"):
            engine.window_resize(dev, window, (8, 8), "box")
    wide = torch.zeros((4, 4000, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DgpError, match="LDS budget"):                      # the horizontal bound stays a host-side refusal
        engine.window_resize(wide, None, (4, 64), "box")
