"""float64 reference of the 16-bit tier's backward kernels, written from their definitions (numpy / torch only, no project code).

The 16-bit pass keeps every tensor as fp16 cells ("H1") with a per-tensor power-of-two scale predicted from the range the same tensor had
one step earlier.  The reference computes in float64 on EXACTLY the values the cells hold, and rounds at the places the kernels round by
design -- there and nowhere else:

  1. H1 operands            h1(x, s) = float16(float32(x) * s); s is a power of two, so this is one rounding to nearest even (subnormals kept)
  2. the stem's frame patch float16(x_centred): the fused stem kernel keeps its 13 x 69 pixel patch as fp16 (no scale)
  3. the stem's dC1         the <= 4 pool windows that route to one conv1 pixel are summed in fp32 (window rows ascending, then columns)
                            and the sum is rounded to fp16 in dPool's scaled units; the column sums add the ROUNDED values
  4. the panel's cells      float16(float32(w * scale) * 2^(14 - E)) for max |w * scale| = m 2^E: high-only cells of the data-gradient panel
  5. the fp16 output cells  float16(float32 result * s_out): not applied here -- the tests bound |cell - reference * s_out| by half an ulp
The fused root block (root_forward) rounds at three more places:
  6. its pixels             float16(u8 - round(mean_c)): small integers, exact; the kernel's fourth input channel is 1 inside the frame and 0
                            in the padding
  7. the fourth weight      sum_c (round(mean_c) - mean_c) w_c carries the mean's fraction: the differences are fp32 values (of the fp32
                            mean), the sum is rounded to fp32 (the device's sum may differ from it by an fp32 ulp: 1e-9 of a conv1 value)
  8. the stem's cells       launch_pack_h3 of the row panel with the scale of rounding point 4 taken from max |w| over the three real
                            channels: high = float16(float32(w * s)), low = float16(w * s - high); the 16-bit tier multiplies by the
                            high cells, the parity tier by high + low
BN and ReLU are float64 there; the pool output's cells are rounding point 5 (the parity tier's H2 cells: 22 bits instead of 11).

Everything between two rounding points (products of two fp16 values, their sums) is exact or fp32-accumulated in the kernels and float64 here.
Tensors are NHWC torch tensors on any device; weights are HWIO.
"""
import math

import numpy as np
import torch


# ---- the predicted-scale rule ------------------------------------------------------------------------------------------------
def pred_scale(prev_max):
    """Scale predicted from last step's maximum (an fp32 value): max = m 2^E (1 <= m < 2) -> 2^(10 - E), so that the maximum lands in
    [2^10, 2^11).  0.0 (no scale, nothing is written) for a zero, subnormal or non-finite maximum, or a scale that is no normal fp32."""
    m = float(np.float32(prev_max))
    if not math.isfinite(m) or m < 2.0 ** -126:
        return 0.0
    E = math.frexp(m)[1] - 1
    if not (1 <= 127 + 10 - E <= 254):
        return 0.0
    return 2.0 ** (10 - E)


def usable(scale, cur_max):
    """A tensor written with `scale` is usable while this step's maximum stays inside [16, 65000) after scaling."""
    if not scale > 0.0:
        return False
    v = float(np.float32(np.float32(cur_max) * np.float32(scale)))
    return 16.0 <= v < 65000.0


def panel_scale(w_max):
    """Scale of a weight panel's fp16 cells: max = m 2^E -> 2^(14 - E); 1 for a zero or non-finite maximum."""
    m = float(np.float32(w_max))
    if not math.isfinite(m) or m < 2.0 ** -126:
        return 1.0
    return 2.0 ** (14 - (math.frexp(m)[1] - 1))


def h1(x, s):
    """The cells: float16(float32(x) * s)."""
    return (x.to(torch.float32) * float(s)).to(torch.float16)


def h1_values(x, s):
    """What the cells of h1(x, s) stand for, float64."""
    return h1(x, s).double() / float(s)


def panel_values(w_hwio, scale=None):
    """The data-gradient panel as its high-only cells hold it: fp32 product w * scale[co], then rounding point 4."""
    wf = w_hwio.to(torch.float32)
    if scale is not None:
        wf = wf * scale.to(torch.float32)
    s = panel_scale(float(wf.abs().max()))
    return h1_values(wf, s)


# ---- convolution geometry ----------------------------------------------------------------------------------------------------
def same_pads(n, k, stride, rate):
    """(pad_before, out): stride 1 TF SAME, stride > 1 the explicit padding of conv2d_same (total keff - 1, smaller half first)."""
    keff = (k - 1) * rate + 1
    tot = keff - 1
    if stride > 1:
        return tot // 2, (n + tot - keff) // stride + 1
    return tot // 2, n


def im2col(x, k, stride, rate, pad_t, pad_l, Ho, Wo):
    """x [N,H,W,C] float64 -> [N*Ho*Wo, k*k*C] with zero padding; tap-major, channel-minor (HWIO rows)."""
    N, H, W, C = x.shape
    keff = (k - 1) * rate + 1
    Hp = (Ho - 1) * stride + keff
    Wp = (Wo - 1) * stride + keff
    xp = torch.zeros((N, max(Hp, H + pad_t), max(Wp, W + pad_l), C), dtype=x.dtype, device=x.device)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    cols = []
    for kh in range(k):
        for kw in range(k):
            cols.append(xp[:, kh * rate: kh * rate + (Ho - 1) * stride + 1: stride,
                           kw * rate: kw * rate + (Wo - 1) * stride + 1: stride])
    return torch.stack(cols, 3).reshape(N * Ho * Wo, k * k * C)


def wgrad(x, dy, k, stride, rate, pad_t, pad_l):
    """dw [k,k,Cin,Cout] = sum over output pixels of x[pixel + tap] * dy[pixel]; colsum [Cout] = sum of dy.  float64 in, float64 out."""
    N, Ho, Wo, Cout = dy.shape
    Cin = x.shape[3]
    cols = im2col(x, k, stride, rate, pad_t, pad_l, Ho, Wo)
    d = dy.reshape(-1, Cout)
    return (cols.t() @ d).reshape(k, k, Cin, Cout), d.sum(0)


def dgrad(dy, w, H, W, stride, rate, pad_t, pad_l):
    """Transposed conv: dx[n, h, w, ci] = sum over taps / co of dy[n, ho, wo, co] * w[kh, kw, ci, co] with h = ho * stride + kh * rate - pad."""
    N, Ho, Wo, Cout = dy.shape
    k, _, Cin, _ = w.shape
    keff = (k - 1) * rate + 1
    Hp = max((Ho - 1) * stride + keff, H + pad_t)
    Wp = max((Wo - 1) * stride + keff, W + pad_l)
    dxp = torch.zeros((N, Hp, Wp, Cin), dtype=torch.float64, device=dy.device)
    dyf = dy.reshape(-1, Cout)
    for kh in range(k):
        for kw in range(k):
            t = (dyf @ w[kh, kw].t()).reshape(N, Ho, Wo, Cin)
            dxp[:, kh * rate: kh * rate + (Ho - 1) * stride + 1: stride,
                kw * rate: kw * rate + (Wo - 1) * stride + 1: stride] += t
    return dxp[:, pad_t:pad_t + H, pad_l:pad_l + W]


def zero_stuff(dy):
    """[N,Ho,Wo,C] -> [N,2Ho,2Wo,C], the data at the even positions."""
    N, Ho, Wo, C = dy.shape
    z = torch.zeros((N, 2 * Ho, 2 * Wo, C), dtype=dy.dtype, device=dy.device)
    z[:, ::2, ::2] = dy
    return z


def dgrad_stuffed(dy, w, H, W, rate, pad_t, pad_l):
    """The stride-2 data gradient in the form the 16-bit pass launches: a stride-1 correlation of the zero-stuffed gradient with the
    flipped taps on the 2 Ho x 2 Wo grid, padding keff - 1 - pad."""
    k, _, Cin, Cout = w.shape
    keff = (k - 1) * rate + 1
    z = zero_stuff(dy)
    cols = im2col(z, k, 1, rate, keff - 1 - pad_t, keff - 1 - pad_l, H, W)
    wf = torch.flip(w, (0, 1)).permute(0, 1, 3, 2).reshape(k * k * Cout, Cin)          # [(tap', co), ci]
    return (cols @ wf).reshape(dy.shape[0], H, W, Cin)


def add_residual(dx, add, add_mode):
    """add_mode 1: a gradient on dx's grid; -2: the subsample shortcut's gradient on the 2x coarser grid, added at the even positions."""
    dx = dx.clone()
    if add is None:
        return dx
    if add_mode == 1:
        dx += add
    elif add_mode == -2:
        dx[:, ::2, ::2] += add
    else:
        raise ValueError(add_mode)
    return dx


def gate(dx, g):
    """Zero wherever the gate value is not positive."""
    return dx if g is None else torch.where(g > 0, dx, torch.zeros_like(dx))


# ---- max-pool 3x3 / stride 2, TF SAME ----------------------------------------------------------------------------------------
def pool_geometry(n):
    """(windows, pad_before) of a 3 / 2 SAME pool over n positions."""
    out = (n + 1) // 2
    tot = max(0, (out - 1) * 2 + 3 - n)
    return out, tot // 2


def pool_windows(c1, fill=-float("inf")):
    """c1 [B,H1,W1,C] -> [9, B,HP,WP,C]: element a * 3 + b of every window (views of one padded copy); `fill` outside the map."""
    B, H1, W1, C = c1.shape
    HP, pt = pool_geometry(H1)
    WP, pl = pool_geometry(W1)
    pad = torch.full((B, 2 * HP + 1, 2 * WP + 1, C), fill, dtype=c1.dtype, device=c1.device)
    pad[:, pt:pt + H1, pl:pl + W1] = c1
    return [pad[:, a:a + 2 * HP - 1:2, b:b + 2 * WP - 1:2] for a in range(3) for b in range(3)]


def pool_valid(H1, W1, device="cpu"):
    """[9, HP, WP] bool: position a * 3 + b of window (qy, qx) lies inside the map."""
    ones = torch.ones((1, H1, W1, 1), dtype=torch.float32, device=device)
    return torch.stack([v[0, :, :, 0] > 0 for v in pool_windows(ones, 0.0)])


def pool_first_max(c1, first_valid=False):
    """c1 [B,H1,W1,C] -> (pool [B,HP,WP,C], record uint8 [B,HP,WP,C]): per window and channel the position a * 3 + b of its FIRST maximum
    in row-major window order (a, b from the window origin 2 q - pad; padding never wins).  first_valid: the first position inside the
    map is taken whatever it holds (maxpool_fwd_idx_kernel's rule: a window of -inf records its first valid position, not 0)."""
    B, H1, W1, C = c1.shape
    HP, WP = pool_geometry(H1)[0], pool_geometry(W1)[0]
    best = torch.full((B, HP, WP, C), -float("inf"), dtype=c1.dtype, device=c1.device)
    rec = torch.zeros((B, HP, WP, C), dtype=torch.uint8, device=c1.device)
    seen = torch.zeros((1, HP, WP, 1), dtype=torch.bool, device=c1.device)
    valid = pool_valid(H1, W1, c1.device)
    for k, v in enumerate(pool_windows(c1)):
        win = v > best                          # strictly greater: an equal later value does not replace the first maximum
        if first_valid:
            ok = valid[k][None, :, :, None]
            win = win | (ok & ~seen)
            seen = seen | ok
        best = torch.where(win, v, best)
        rec = torch.where(win, torch.full_like(rec, k), rec)
    return best, rec


def pool_backward(dpool, rec, H1, W1, dtype=torch.float64):
    """dC1 [B,H1,W1,C]: every window's gradient goes to the pixel its record names (a position outside the map: dropped).  Accumulated in
    `dtype` in the order window rows ascending, then window columns ascending per pixel (the stem kernel's order: float32 there)."""
    B, HP, WP, C = dpool.shape
    _, pt = pool_geometry(H1)
    _, pl = pool_geometry(W1)
    buf = torch.zeros((B, 2 * HP + 1, 2 * WP + 1, C), dtype=dtype, device=dpool.device)
    g = dpool.to(dtype)
    for a in (2, 1, 0):                         # a pixel's windows in ascending order = their in-window positions in descending order
        for b in (2, 1, 0):
            sel = torch.where(rec == a * 3 + b, g, torch.zeros_like(g))
            buf[:, a:a + 2 * HP - 1:2, b:b + 2 * WP - 1:2] += sel
    return buf[:, pt:pt + H1, pl:pl + W1].clone()


def stem_cells(w, mean):
    """w [7,7,3,64] -> (high, low) [7,7,4,64] float64 in scaled units and the scale: rounding points 7 and 8."""
    wf = w.to(torch.float32)
    m32 = np.asarray(mean, dtype=np.float32)
    d = torch.tensor((np.round(m32) - m32).astype(np.float64), dtype=torch.float64, device=w.device)
    w4 = (wf.double() * d[None, None, :, None]).sum(2, keepdim=True).to(torch.float32)
    s = panel_scale(float(wf.abs().max()))
    ws = torch.cat([wf, w4], 2) * float(s)                           # fp32, exact (a power of two)
    high = ws.to(torch.float16)
    low = (ws - high.float()).to(torch.float16)                      # the residual is exact in fp32
    return high.double(), low.double(), s


def root_forward(frames, w, bn_scale, bn_bias, mean, cells, scale=1.0):
    """The root block in float64 on the operands the kernel holds: frames [B,H,W,3] uint8, w [7,7,3,64] -> (conv1 map after BN + ReLU
    [B,H1,W1,64], pool maxima [B,HP,WP,64]), both times `scale` (the scaled units of the output cells).
    cells "h1": the 16-bit tier (high weight cells), "h2": the parity tier's fused kernel (high + low), "f32": the unfused layers (fp32
    pixels u8 - mean, fp32 weights, no cells).  The sum runs tap by tap and channel by channel with elementwise float64 operations, so
    that two conv1 pixels with identical patches get bitwise identical values (a library GEMM need not promise that)."""
    B, H, W, _ = frames.shape
    pad_t, H1 = same_pads(H, 7, 2, 1)
    pad_l, W1 = same_pads(W, 7, 2, 1)
    dev = frames.device
    if cells == "f32":
        m32 = torch.tensor(np.asarray(mean, dtype=np.float32), device=dev)
        x = (frames.to(torch.float32) - m32).double()                                     # one fp32 rounding, as preprocess_u8
        wq, s = w.to(torch.float32).double(), 1.0
    else:
        mr = torch.tensor(np.round(np.asarray(mean, dtype=np.float32)), device=dev)
        x = torch.cat([(frames.to(torch.float32) - mr).to(torch.float16).double(),          # rounding point 6
                       torch.ones((B, H, W, 1), dtype=torch.float64, device=dev)], 3)
        high, low, s = stem_cells(w, mean)
        wq = high if cells == "h1" else high + low
    C = x.shape[3]
    xp = torch.zeros((B, 2 * H1 + 5, 2 * W1 + 5, C), dtype=torch.float64, device=dev)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    acc = torch.zeros((B, H1, W1, 64), dtype=torch.float64, device=dev)
    for kh in range(7):
        for kw in range(7):
            v = xp[:, kh:kh + 2 * H1 - 1:2, kw:kw + 2 * W1 - 1:2]
            for c in range(C):
                acc += v[..., c:c + 1] * wq[kh, kw, c]
    c1 = torch.relu(acc / float(s) * bn_scale.double() + bn_bias.double()) * float(scale)
    return c1, torch.stack(pool_windows(c1)).amax(0)


def stem_wgrad(x_centred, dpool_cells, rec, s):
    """The fused stem weight gradient on dPool's cells (fp16, scaled by s): -> (dw [7,7,4,64], colsum [64], dC1 in scaled units), float64."""
    B, H, W, _ = x_centred.shape
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    xh = x_centred.to(torch.float32).to(torch.float16).double()                          # rounding point 2
    dc1 = pool_backward(dpool_cells, rec, H1, W1, dtype=torch.float32).to(torch.float16).double()      # rounding point 3
    dw, cs = wgrad(xh, dc1, 7, 2, 1, 3, 3)
    return dw / s, cs / s, dc1


# ---- heads: 3x3 / stride 2 transposed convs, both heads in one phase-major tensor --------------------------------------------------
def _pow2_at_least_4(x):
    p = 4
    while p < x:
        p *= 2
    return p


def heads_layout(nj):
    """(cpad0, cpad1, CT): the part head's 4 phases x nj columns padded to a power of two, the locref head's 4 x 2 nj likewise behind
    them, the row padded to a multiple of 64."""
    c0, c1 = _pow2_at_least_4(4 * nj), _pow2_at_least_4(8 * nj)
    return c0, c1, (c0 + c1 + 63) // 64 * 64


def heads_gather(dsc, dloc):
    """dsc [N,2h,2w,nj], dloc [N,2h,2w,2nj] -> [N,h,w,CT]: column ph * njt + c of a head = d out[n, 2i + (ph >> 1), 2j + (ph & 1), c]."""
    N, H2, W2, nj = dsc.shape
    c0, c1, CT = heads_layout(nj)
    out = torch.zeros((N, H2 // 2, W2 // 2, CT), dtype=dsc.dtype, device=dsc.device)
    for col0, t in ((0, dsc), (c0, dloc)):
        njt = t.shape[3]
        for ph in range(4):
            out[..., col0 + ph * njt: col0 + (ph + 1) * njt] = t[:, (ph >> 1)::2, (ph & 1)::2]
    return out


def heads_scatter(G, nj):
    """Inverse of heads_gather on the used columns: -> (dsc, dloc)."""
    N, h, w, _ = G.shape
    c0, _, _ = heads_layout(nj)
    res = []
    for col0, njt in ((0, nj), (c0, 2 * nj)):
        t = torch.zeros((N, 2 * h, 2 * w, njt), dtype=G.dtype, device=G.device)
        for ph in range(4):
            t[:, (ph >> 1)::2, (ph & 1)::2] = G[..., col0 + ph * njt: col0 + (ph + 1) * njt]
        res.append(t)
    return res


def head_backward(feat, dout, w):
    """One head, out[n, 2i + ka, 2j + kb, c] += feat[n, i, j, :] . w[ka, kb, c, :] (cropped to 2h x 2w): -> (dw [3,3,njt,Cin], db [njt],
    dfeat [N,h,w,Cin]) from d out, float64."""
    N, h, wd, Cin = feat.shape
    njt = dout.shape[3]
    dw = torch.zeros((3, 3, njt, Cin), dtype=torch.float64, device=feat.device)
    dfeat = torch.zeros((N, h, wd, Cin), dtype=torch.float64, device=feat.device)
    for ka in range(3):
        for kb in range(3):
            d = dout[:, ka::2, kb::2]
            hh, ww = d.shape[1], d.shape[2]
            f = feat[:, :hh, :ww]
            dw[ka, kb] = d.reshape(-1, njt).t() @ f.reshape(-1, Cin)
            dfeat[:, :hh, :ww] += d @ w[ka, kb]
    return dw, dout.sum((0, 1, 2)), dfeat
