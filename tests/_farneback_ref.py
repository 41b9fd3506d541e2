"""Float64 numpy restatement of the Farneback flow contract that csrc/dgp_flow.hip implements (the issue's steps 1-8), written from
the contract, not from OpenCV: every border rule is an explicit index array.  A checker only -- no cv2, no library filters."""
import numpy as np

MIN_SIZE = 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def gray(frame):
    """Step 1: uint8 [H, W, 3] with channel 0 = B -> OpenCV's fixed-point BGR2GRAY, as float64 (integer-valued)."""
    f = frame.astype(np.int64)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14).astype(np.float64)


def round_half_even(v):
    return int(np.rint(v))


def plan(H, W, pyr_scale=0.5, levels=3):
    """Step 2: [(k, w, h, sigma, ksize)] for k = 0..levels_used.  The pyramid stops before the first level narrower or lower than 32
    pixels: levels_used is the last k whose W * pyr_scale^k and H * pyr_scale^k are both >= 32 (at most `levels`)."""
    used, s = 0, 1.0
    while used < levels:
        s *= pyr_scale
        if W * s < MIN_SIZE or H * s < MIN_SIZE:
            break
        used += 1
    out = []
    for k in range(used + 1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1.0) * 0.5
        ksize = max(round_half_even(sigma * 5) | 1, 3)
        out.append((k, round_half_even(W * scale), round_half_even(H * scale), sigma, ksize))
    return out


def reflect101(i, n):
    i = np.asarray(i, dtype=np.int64).copy()
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i[lo] = -i[lo]
        i[hi] = 2 * (n - 1) - i[hi]


def blur_taps(ksize, sigma):
    if sigma <= 0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksize) - (ksize - 1) / 2.0
    t = np.exp(-(x * x) / (2 * sigma * sigma))
    return (t / t.sum()).astype(np.float32).astype(np.float64)


def lin_map(dst_size, src_size):
    """Half-pixel-centre bilinear source coordinates: (index0, index1, fraction) per destination index, clamped as the contract says."""
    s = (np.arange(dst_size) + 0.5) * (src_size / dst_size) - 0.5
    i0 = np.floor(s).astype(np.int64)
    fr = s - i0
    lo, hi = i0 < 0, i0 >= src_size - 1
    i0[lo], fr[lo] = 0, 0.0
    i0[hi], fr[hi] = src_size - 1, 0.0
    return i0, np.minimum(i0 + 1, src_size - 1), fr


def resize(img, w, h):
    """Bilinear resize of [H, W, ...] to [h, w, ...]: horizontal interpolation, then vertical."""
    H, W = img.shape[:2]
    x0, x1, fx = lin_map(w, W)
    y0, y1, fy = lin_map(h, H)
    ex = (slice(None),) + (None,) * (img.ndim - 2)
    fx, fy = fx[ex], fy[:, None][(slice(None), slice(None)) + (None,) * (img.ndim - 2)]
    rows = lambda r: img[r][:, x0] * (1 - fx) + img[r][:, x1] * fx
    return rows(y0) * (1 - fy) + rows(y1) * fy


def level_image(g, w, h, sigma, ksize):
    """Step 3: separable Gaussian (REFLECT_101, rows first) of the FULL-RESOLUTION gray, then bilinear resize to w x h."""
    H, W = g.shape
    taps = blur_taps(ksize, sigma)
    r = ksize // 2
    cols = reflect101(np.arange(W)[:, None] - r + np.arange(ksize)[None, :], W)      # [W, ksize]
    hb = (g[:, cols] * taps).sum(-1)
    rows = reflect101(np.arange(H)[:, None] - r + np.arange(ksize)[None, :], H)      # [H, ksize]
    v = (hb[rows] * taps[None, :, None]).sum(1)
    return resize(v, w, h)


def poly_coefficients(n, sigma):
    """Step 4's Gaussian (taps stored as float, as the kernels do) and the four entries of inv(G) it uses."""
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma)).astype(np.float32).astype(np.float64)
    g = (g / g.sum()).astype(np.float32).astype(np.float64)
    xg, xxg = x * g, x * x * g
    gy, gx = np.meshgrid(g, g, indexing="ij")
    yy, xx = np.meshgrid(x, x, indexing="ij")
    basis = [np.ones_like(xx), xx, yy, xx * xx, yy * yy, xx * yy]
    w = gy * gx
    G = np.array([[np.sum(w * a * b) for b in basis] for a in basis])
    iG = np.linalg.inv(G)
    return g, xg, xxg, iG[1, 1], iG[0, 3], iG[3, 3], iG[5, 5]


def poly_exp(img, n, sigma):
    """Step 4: R [5, h, w] = (y-linear, x-linear, y^2, x^2, xy) coefficients."""
    h, w = img.shape
    g, xg, xxg, ig11, ig03, ig33, ig55 = poly_coefficients(n, sigma)
    c = n                                          # tap k sits at index c + k
    s0, s1, s2 = img * g[c], np.zeros_like(img), np.zeros_like(img)
    ys = np.arange(h)
    for k in range(1, n + 1):
        up, dn = img[np.maximum(ys - k, 0)], img[np.minimum(ys + k, h - 1)]
        s0 = s0 + g[c + k] * (up + dn)
        s1 = s1 + xg[c + k] * (dn - up)
        s2 = s2 + xxg[c + k] * (up + dn)
    xs = np.arange(w)
    b1, b3, b5 = s0 * g[c], s1 * g[c], s2 * g[c]
    b2, b4, b6 = np.zeros_like(img), np.zeros_like(img), np.zeros_like(img)
    for k in range(1, n + 1):
        L, Rt = np.maximum(xs - k, 0), np.minimum(xs + k, w - 1)
        b1 = b1 + g[c + k] * (s0[:, Rt] + s0[:, L])
        b2 = b2 + xg[c + k] * (s0[:, Rt] - s0[:, L])
        b3 = b3 + g[c + k] * (s1[:, Rt] + s1[:, L])
        b4 = b4 + xxg[c + k] * (s0[:, Rt] + s0[:, L])
        b5 = b5 + g[c + k] * (s2[:, Rt] + s2[:, L])
        b6 = b6 + xg[c + k] * (s1[:, Rt] - s1[:, L])
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55])


def border_scale(h, w):
    def edge(size):
        s = np.ones(size)
        for d in range(min(5, size)):
            s[d] *= BORDER[d]
            s[size - 1 - d] *= BORDER[d]
        return s
    return edge(h)[:, None] * edge(w)[None, :]


def update_matrices(R0, R1, flow):
    """Step 5: M [5, h, w] of the pair (R0, R1) for flow [h, w, 2]."""
    _, h, w = R0.shape
    dx, dy = flow[..., 0], flow[..., 1]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fx, fy = xx + dx, yy + dy
    x1, y1 = np.floor(fx), np.floor(fy)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xi, yi = np.where(inside, x1, 0).astype(np.int64), np.where(inside, y1, 0).astype(np.int64)
    ax, ay = fx - x1, fy - y1
    interp = ((1 - ax) * (1 - ay) * R1[:, yi, xi] + ax * (1 - ay) * R1[:, yi, xi + 1] + (1 - ax) * ay * R1[:, yi + 1, xi]
              + ax * ay * R1[:, yi + 1, xi + 1])
    r2 = np.where(inside, interp[0], 0.0)
    r3 = np.where(inside, interp[1], 0.0)
    r4 = np.where(inside, (R0[2] + interp[2]) / 2, R0[2])
    r5 = np.where(inside, (R0[3] + interp[3]) / 2, R0[3])
    r6 = np.where(inside, (R0[4] + interp[4]) / 4, R0[4] / 2)
    r2 = (R0[0] - r2) / 2 + r4 * dy + r6 * dx
    r3 = (R0[1] - r3) / 2 + r6 * dy + r5 * dx
    s = border_scale(h, w)
    r2, r3, r4, r5, r6 = r2 * s, r3 * s, r4 * s, r5 * s, r6 * s
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3])


def box_mean(M, winsize):
    """winsize x winsize mean of each plane with replicated borders."""
    _, h, w = M.shape
    r = winsize // 2
    ry = np.clip(np.arange(-r, h + r), 0, h - 1)
    rx = np.clip(np.arange(-r, w + r), 0, w - 1)
    P = M[:, ry][:, :, rx]
    cs = np.cumsum(np.pad(P, ((0, 0), (1, 0), (0, 0))), axis=1)
    V = cs[:, winsize:] - cs[:, :-winsize]
    cs = np.cumsum(np.pad(V, ((0, 0), (0, 0), (1, 0))), axis=2)
    return (cs[:, :, winsize:] - cs[:, :, :-winsize]) / float(winsize * winsize)


def solve(B):
    g11, g12, g22, h1, h2 = B
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1)


def farneback(frames, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2):
    """Steps 1-8 on uint8 BGR frames [T, H, W, 3] -> flow [T-1, H, W, 2] float64 (dx, dy)."""
    frames = np.asarray(frames)
    T, H, W = frames.shape[:3]
    grays = [gray(f) for f in frames]
    lv = plan(H, W, pyr_scale, levels)
    prev = None
    for k, w, h, sigma, ksize in reversed(lv):
        R = [poly_exp(level_image(g, w, h, sigma if k > 0 else 0.0, ksize), poly_n, poly_sigma) for g in grays]
        cur = []
        for p in range(T - 1):
            f = np.zeros((h, w, 2)) if prev is None else resize(prev[p], w, h) * (1.0 / pyr_scale)
            M = update_matrices(R[p], R[p + 1], f)
            for it in range(iterations):
                f = solve(box_mean(M, winsize))
                if it < iterations - 1:
                    M = update_matrices(R[p], R[p + 1], f)
            cur.append(f)
        prev = cur
    return np.stack(prev) if prev else np.zeros((0, H, W, 2))


def magnitude(flow):
    return np.abs(flow).sum(-1)
