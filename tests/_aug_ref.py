"""float64 restatements in numpy of the augmentation stages that deepgraphpose_amd/csrc/dgp_augment.hip restates (no GPU, no project
code): Pillow's AFFINE + BILINEAR transform, the elastic stage, Philox4x32-10 and the noise stage built on it."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reaching_frame(name="img005.png"):
    """one 747 x 832 frame of the Reaching project, uint8 [H, W, 3]"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(HERE, "golden", "reaching_frames", name)).convert("RGB")))


def pattern_frame(H, W, seed=0):
    """a smooth pattern with noise on top, uint8 [H, W, 3]: every byte value, edges, no two rows or channels alike"""
    rng = np.random.default_rng(seed * 7919 + H * 1000 + W)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255.0 / max(W - 1, 1)), (y * 255.0 / max(H - 1, 1)), ((x + 2 * y) * 37 % 256)], -1)
    return np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)


def pil_affine_bilinear(img, coef):
    """Image.fromarray(img).transform((W, H), AFFINE, coef, BILINEAR) as Pillow computes it (Geometry.c: affine_transform +
    bilinear_filter32RGB), in float64: byte for byte"""
    H, W = img.shape[:2]
    a, b, c, d, e, f = (np.float64(v) for v in coef)
    y, x = np.mgrid[0:H, 0:W]
    xc, yc = x + 0.5, y + 0.5
    xin = a * xc + b * yc + c
    yin = d * xc + e * yc + f
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = xin - 0.5, yin - 0.5
    xi, yi = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - xi)[..., None], (yin - yi)[..., None]
    x0, x1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    y0 = np.clip(yi, 0, H - 1)
    below = (yi + 1 >= 0) & (yi + 1 < H)
    yb = np.where(below, np.clip(yi + 1, 0, H - 1), y0)
    src = img.astype(np.int64)
    p00, p01 = src[y0, x0], src[y0, x1]
    v1 = p00 + (p01 - p00) * dx
    p10, p11 = src[yb, x0], src[yb, x1]
    v2 = np.where(below[..., None], p10 + (p11 - p10) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], np.trunc(v), 0.0).astype(np.uint8)


def elastic_f64(img, field):
    """The elastic stage's value before rounding, float64 [H, W, 3]: d(y, x) = bilinear value of the fp32 coarse field [2, hc, wc] at
    (y / 4, x / 4), then the bilinear sample of img, zeros outside, at (x + dx, y + dy)"""
    H, W = img.shape[:2]
    g = np.asarray(field, dtype=np.float64)
    hc, wc = g.shape[1:]
    y, x = np.mgrid[0:H, 0:W]
    i0, j0 = y // 4, x // 4
    i1, j1 = np.minimum(i0 + 1, hc - 1), np.minimum(j0 + 1, wc - 1)
    fy, fx = (y - 4 * i0) / 4.0, (x - 4 * j0) / 4.0
    d = [(gc[i0, j0] * (1 - fx) + gc[i0, j1] * fx) * (1 - fy) + (gc[i1, j0] * (1 - fx) + gc[i1, j1] * fx) * fy for gc in g]
    sx, sy = x + d[0], y + d[1]
    xf, yf = np.floor(sx), np.floor(sy)
    tx, ty = (sx - xf)[..., None], (sy - yf)[..., None]
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    src = img.astype(np.float64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok[..., None], src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0)

    return (tap(yi, xi) * (1 - tx) + tap(yi, xi + 1) * tx) * (1 - ty) + (tap(yi + 1, xi) * (1 - tx) + tap(yi + 1, xi + 1) * tx) * ty


_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11).  counter: uint [..., 4], key:
    (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack(c, -1).astype(np.uint32)


def noise_z64(H, W, per_channel, key):
    """The noise stage's standard normals in float64, [H, W, 3] or [H, W, 1]: element e = (y W + x) 3 + c with per_channel and y W + x
    without takes lane e % 4 of Philox block e / 4 under key (low, high half); u = ((word >> 8) + 0.5) 2^-24; Box-Muller on the word
    pairs (0, 1) and (2, 3): sqrt(-2 ln u_a) cos(2 pi u_b) for the even lane, sin for the odd one"""
    n = H * W * (3 if per_channel else 1)
    e = np.arange(n, dtype=np.uint64)
    blk = e >> np.uint64(2)
    ctr = np.stack([blk & _MASK, blk >> np.uint64(32), np.zeros_like(blk), np.zeros_like(blk)], -1)
    w = philox4x32_10(ctr, (int(key) & 0xFFFFFFFF, int(key) >> 32))
    lane = (e & np.uint64(3)).astype(np.int64)
    rows = np.arange(n)
    wa, wb = w[rows, np.where(lane < 2, 0, 2)], w[rows, np.where(lane < 2, 1, 3)]
    ua = ((wa >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    ub = ((wb >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(ua))
    z = rad * np.where(lane & 1, np.sin(2 * np.pi * ub), np.cos(2 * np.pi * ub))
    return z.reshape(H, W, 3 if per_channel else 1)


def noise_f64(img, scale, per_channel, key):
    """The noise stage's value before rounding: clip(src + float32(scale) z64, 0, 255), float64 [H, W, 3]"""
    H, W = img.shape[:2]
    return np.clip(img.astype(np.float64) + np.float64(np.float32(scale)) * noise_z64(H, W, per_channel, key), 0.0, 255.0)


def noise_u8(img, scale, per_channel, key):
    return np.rint(noise_f64(img, scale, per_channel, key)).astype(np.uint8)
