"""A restatement of libjpeg's baseline ENCODER in numpy, the mirror image of _jpeg_ref.py: 16.16 fixed-point RGB -> YCbCr (jccolor),
chroma downsampling without smoothing (jcsample), the asymmetric edge replication, the "islow" forward DCT (jfdctint), quantisation by
8 q with a truncating divide, the dummy blocks of partial MCUs, and the stream Pillow writes around the Huffman-coded data (Annex K.3
tables, no restart markers).  It is the specification for dgp_jpeg_forward_u8 and dgp_jpeg_entropy_encode.

    quality_tables(q)                         -> uint16 [2, 64] natural order (luminance, chrominance)
    forward(rgb, sampling, qt)                -> int16 [total_blocks, 64] in the layout _jpeg_ref.entropy_decode writes
    entropy_encode(coef, H, W, sampling, qt)  -> bytes, SOI to EOI
    encode(rgb, quality, sampling)            -> entropy_encode(forward(...))"""
import numpy as np

import _jpeg_ref as R

S444, S422, S420 = R.S444, R.S422, R.S420
PILLOW_SUBSAMPLING = {S444: 0, S422: 1, S420: 2}

_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quality_tables(q):
    if not 1 <= q <= 100:
        raise ValueError("quality 1 .. 100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((np.array(t, np.int64) * scale + 50) // 100, 1, 255) for t in (_LUM, _CHR)]).astype(np.uint16)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(a, rows, cols):
    """replicate the last row / column up to rows x cols"""
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def real_blocks(H, W, sampling):
    """per component (rows, columns) of blocks that carry image samples"""
    g = R.geometry(W, H, sampling)
    ch, cw = -(-H // g["vs"]), -(-W // g["hs"])
    return [(-(-H // 8), -(-W // 8)), (-(-ch // 8), -(-cw // 8)), (-(-ch // 8), -(-cw // 8))]


def planes(rgb, sampling):
    """the three component planes, each real_blocks x 8 samples: int64"""
    H, W = rgb.shape[:2]
    g = R.geometry(W, H, sampling)
    hs, vs = g["hs"], g["vs"]
    rb = real_blocks(H, W, sampling)
    out = []
    for c, full in enumerate(ycc(rgb)):
        rby, rbx = rb[c]
        h, v = (1, 1) if c == 0 else (hs, vs)
        p = _pad(full, -(-H // vs) * vs, rbx * 8 * h)           # rows to a multiple of the vertical factor, columns to the real blocks
        if h == 2 and v == 1:
            bias = np.arange(p.shape[1] // 2) & 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif h == 2 and v == 2:
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_pad(p[:rby * 8], rby * 8, p.shape[1]))     # then the component's rows to its real blocks
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(x, first):
    """jfdctint's pass over the LAST axis of an int64 array [..., 8]"""
    d = [x[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(plane, q):
    """plane [8 by, 8 bx] -> quantised int64 [by, bx, 64]"""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128
    x = _fdct_1d(x, True)                                              # rows
    x = _fdct_1d(x.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # then columns
    x = x.reshape(by, bx, 64)
    d = q.astype(np.int64) * 8
    return np.sign(x) * ((np.abs(x) + (d >> 1)) // d)


def forward(rgb, sampling, qt):
    H, W = rgb.shape[:2]
    g = R.geometry(W, H, sampling)
    rb = real_blocks(H, W, sampling)
    out = []
    for c, p in enumerate(planes(rgb, sampling)):
        real = fdct_quant(p, qt[min(c, 1)])
        by, bx = g["blocks_y"][c], g["blocks_x"][c]
        ch, cv = (g["hs"], g["vs"]) if c == 0 else (1, 1)
        grid = np.zeros((by, bx, 64), np.int64)
        grid[:rb[c][0], :rb[c][1]] = real
        for my in range(g["mcus_y"]):                                  # dummy blocks: the DC of the block before, in MCU order
            for mx in range(g["mcus_x"]):
                prev = None
                for iy in range(cv):
                    for ix in range(ch):
                        y, x = my * cv + iy, mx * ch + ix
                        if y >= rb[c][0] or x >= rb[c][1]:
                            grid[y, x, 0] = prev
                        prev = grid[y, x, 0]
        out.append(grid.reshape(-1, 64))
    return np.concatenate(out).astype(np.int16)


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, size):
        self.acc = (self.acc << size) | code
        self.n += size
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _codes(key):
    """symbol -> (code, length) of an Annex K.3 table"""
    return {sym: (code, l) for (l, code), sym in R._huff(*R.STD_TABLES[key]).items()}


def header(H, W, sampling, qt):
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k in range(2):
        b += b"\xff\xdb\x00\x43" + bytes([k]) + bytes(int(qt[k][R.ZIGZAG[i]]) for i in range(64))
    hv = {S444: 0x11, S422: 0x21, S420: 0x22}[sampling]
    b += b"\xff\xc0\x00\x11\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = R.STD_TABLES[(tc, th)]
        b += b"\xff\xc4" + bytes([(19 + len(vals)) >> 8, (19 + len(vals)) & 255, (tc << 4) | th]) + bytes(bits) + bytes(vals)
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(b)


def entropy_encode(coef, H, W, sampling, qt):
    g = R.geometry(W, H, sampling)
    off = np.concatenate([[0], np.cumsum(g["blocks"])])
    dc, ac = [_codes((0, 0)), _codes((0, 1))], [_codes((1, 0)), _codes((1, 1))]
    w = _Writer()
    pred = [0, 0, 0]
    zz = coef.astype(np.int64)[:, R.ZIGZAG]

    def value(v, limit):
        n = int(abs(v)).bit_length()
        if n > limit:
            raise ValueError("coefficient %d needs category %d" % (v, n))
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    for my in range(g["mcus_y"]):
        for mx in range(g["mcus_x"]):
            for c in range(3):
                ch, cv = (g["hs"], g["vs"]) if c == 0 else (1, 1)
                t = min(c, 1)
                for by in range(cv):
                    for bx in range(ch):
                        blk = zz[off[c] + (my * cv + by) * g["blocks_x"][c] + mx * ch + bx]
                        n, bits = value(int(blk[0]) - pred[c], 11)
                        pred[c] = int(blk[0])
                        w.put(*dc[t][n])
                        if n:
                            w.put(bits, n)
                        run = 0
                        for k in range(1, 64):
                            v = int(blk[k])
                            if v == 0:
                                run += 1
                                continue
                            while run > 15:
                                w.put(*ac[t][0xF0])
                                run -= 16
                            n, bits = value(v, 10)
                            w.put(*ac[t][(run << 4) | n])
                            w.put(bits, n)
                            run = 0
                        if run:
                            w.put(*ac[t][0])
    w.flush()
    return header(H, W, sampling, qt) + bytes(w.out) + b"\xff\xd9"


def encode(rgb, quality, sampling):
    qt = quality_tables(quality)
    return entropy_encode(forward(rgb, sampling, qt), rgb.shape[0], rgb.shape[1], sampling, qt)
