"""numpy restatement of Pillow's 8-bit antialiased resample (ImagingResample, BICUBIC: what `Image.resize(size=...)` runs by default) and
of `Image.crop` after it -- the contract of csrc/dgp_resize.hip, written from Pillow's documented algorithm (no Pillow call in here).

Per axis, inSize -> outSize: scale = inSize / outSize, filterscale = max(scale, 1), support = 2 * filterscale,
ksize = ceil(support) * 2 + 1; output xx takes inputs [xmin, xmin + n) around center = (xx + 0.5) * scale with the Keys bicubic
(a = -0.5) evaluated at (x + xmin - center + 0.5) / filterscale, normalised by the window's sum, all in double in this order, then rounded
half away from zero to 22-bit fixed point.  A pass is clip((2^21 + sum k * pixel) >> 22, 0, 255) on int32; horizontal first, its bytes
clipped before the vertical pass."""
import math

import numpy as np

PRECISION_BITS = 22

# the seven shapes Pillow was compared with byte for byte: (H, W) -> (oh, ow)
SHAPES = [((97, 131), (72, 96)), ((64, 80), (64, 40)), ((50, 70), (120, 70)), ((33, 47), (7, 5)), ((48, 64), (48, 64)),
          ((120, 160), (61, 83)), ((30, 40), (95, 133))]


def bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def plan(in_size: int, out_size: int):
    """(ksize, bounds int32 [out, 2] = (xmin, n), coeffs int32 [out, ksize], zero-padded)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) / filterscale) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return ksize, bounds, coeffs


def _pass_last_axis(img: np.ndarray, out_size: int) -> np.ndarray:
    """resample axis -2 of a [..., n, C] uint8 array"""
    _, bounds, coeffs = plan(img.shape[-2], out_size)
    out = np.empty(img.shape[:-2] + (out_size, img.shape[-1]), np.uint8)
    src = img.astype(np.int32)
    for xx in range(out_size):
        x0, n = bounds[xx]
        ss = (src[..., x0:x0 + n, :] * coeffs[xx, :n, None]).sum(-2, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        out[..., xx, :] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resize(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """[..., H, W, C] uint8 -> [..., oh, ow, C]: horizontal pass, clip to uint8, vertical pass"""
    hor = _pass_last_axis(img, ow)
    return np.swapaxes(_pass_last_axis(np.swapaxes(hor, -3, -2), oh), -3, -2)


def crop(img: np.ndarray, box) -> np.ndarray:
    """Image.crop: the box (left, upper, right, lower) of [..., H, W, C]; what lies outside the image is zero"""
    l, u, r, b = (int(v) for v in box)
    H, W = img.shape[-3:-1]
    out = np.zeros(img.shape[:-3] + (max(b - u, 0), max(r - l, 0), img.shape[-1]), img.dtype)
    y0, y1, x0, x1 = max(u, 0), min(b, H), max(l, 0), min(r, W)
    if y1 > y0 and x1 > x0:
        out[..., y0 - u:y1 - u, x0 - l:x1 - l, :] = img[..., y0:y1, x0:x1, :]
    return out


def resize_crop(img: np.ndarray, new_size=None, crop_size=None) -> np.ndarray:
    """what estimate_pose's host preparation gives: new_size = (rows, cols), crop_size = (left, upper, right, lower)"""
    if new_size is not None:
        img = resize(img, int(new_size[0]), int(new_size[1]))
    if crop_size is not None:
        img = crop(img, crop_size)
    return img


def test_image(H: int, W: int, seed: int = 0, batch=None) -> np.ndarray:
    """seeded random bytes with a saturated {0, 255} quadrant (bicubic over- and undershoots there: the clip between the passes shows)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    shape = ((batch,) if batch else ()) + (H, W, 3)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    x[..., :H // 2, :W // 2, :] = rng.integers(0, 2, shape[:-3] + (H // 2, W // 2, 3), dtype=np.uint8) * 255
    return x
