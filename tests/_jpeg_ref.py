"""A restatement of baseline JPEG decoding, written from ITU-T T.81 and libjpeg's documented arithmetic: a pure-Python marker parser and
Huffman decoder, and the numpy reconstruction ("islow" inverse DCT, "fancy" chroma upsampling, 16.16 fixed-point YCbCr -> RGB).  It is the
oracle for the coefficients dgp_jpeg_entropy_decode writes and, beside Pillow itself, for the pixels of dgp_jpeg_reconstruct_u8.

    parse(b)            -> dict (width, height, ncomp, sampling, restart, scan_offset, tables)
    entropy_decode(b)   -> (coef int16 [total_blocks, 64] natural order, planar by component; qt uint16 [ncomp, 64]; info)
    reconstruct(coef, qt, H, W, sampling) -> uint8 [H, W, 3]
    decode(b)           -> reconstruct(entropy_decode(b))

Anything outside the accepted subset, and any malformed stream, raises JpegError."""
import numpy as np

GRAY, S444, S422, S420 = 0, 1, 2, 3


class JpegError(ValueError):
    pass


ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

# Annex K.3 (typical tables): (counts per length 1..16, symbols)
_AC_LUM = ("01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09 0a 16 17 18 "
           "19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 "
           "76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 "
           "c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa")
_AC_CHR = ("00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 34 e1 25 "
           "f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 "
           "75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba "
           "c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa")
STD_TABLES = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [int(v, 16) for v in _AC_LUM.split()]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [int(v, 16) for v in _AC_CHR.split()]),
}


def _huff(bits, vals):
    """Annex C: {(length, code): symbol}"""
    if sum(bits) != len(vals) or len(vals) > 256:
        raise JpegError("bad Huffman table")
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        if code + bits[l - 1] > (1 << l):
            raise JpegError("Huffman table is no prefix code")
        for _ in range(bits[l - 1]):
            table[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def geometry(W, H, sampling):
    hs = 2 if sampling in (S422, S420) else 1
    vs = 2 if sampling == S420 else 1
    ncomp = 1 if sampling == GRAY else 3
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    bx = [mx * hs, mx, mx][:ncomp]
    by = [my * vs, my, my][:ncomp]
    return dict(hs=hs, vs=vs, ncomp=ncomp, mcus_x=mx, mcus_y=my, blocks_x=bx, blocks_y=by, blocks=[a * b for a, b in zip(bx, by)],
                total_blocks=sum(a * b for a, b in zip(bx, by)))


def parse(b):
    try:
        return _parse(bytes(b))
    except IndexError:
        raise JpegError("truncated segment")


def _parse(b):
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise JpegError("no SOI")
    qt, huff, sof, restart, jfif, adobe = {}, {}, None, 0, False, None
    p = 2
    while True:
        if p + 2 > n or b[p] != 0xFF:
            raise JpegError("marker expected")
        while p + 1 < n and b[p + 1] == 0xFF:
            p += 1
        if p + 2 > n:
            raise JpegError("truncated")
        m = b[p + 1]
        p += 2
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegError("EOI before a scan")
        if p + 2 > n:
            raise JpegError("truncated")
        L = (b[p] << 8) | b[p + 1]
        if L < 2 or p + L > n:
            raise JpegError("truncated segment")
        seg = b[p + 2:p + L]
        p += L
        if m == 0xC0:
            if sof is not None or len(seg) < 6:
                raise JpegError("bad SOF0")
            if seg[0] != 8:
                raise JpegError("precision")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc not in (1, 3) or H == 0 or W == 0 or len(seg) != 6 + 3 * nc:
                raise JpegError("components / size")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(nc)]
            if any(c[2] > 3 for c in comps):
                raise JpegError("table id")
            if nc == 1:
                if not (1 <= comps[0][1] >> 4 <= 4 and 1 <= comps[0][1] & 15 <= 4):
                    raise JpegError("sampling")
                sampling = GRAY
            else:
                if comps[1][1] != 0x11 or comps[2][1] != 0x11 or comps[0][1] not in (0x11, 0x21, 0x22):
                    raise JpegError("sampling")
                sampling = {0x11: S444, 0x21: S422, 0x22: S420}[comps[0][1]]
                if len({c[0] for c in comps}) != 3:
                    raise JpegError("component ids")
            sof = (W, H, nc, sampling, comps)
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            raise JpegError("not baseline")
        elif m == 0xC4:
            t = 0
            while t < len(seg):
                if len(seg) - t < 17:
                    raise JpegError("DHT")
                tc, th = seg[t] >> 4, seg[t] & 15
                bits = list(seg[t + 1:t + 17])
                nv = sum(bits)
                if tc > 1 or th > 3 or nv > 256 or len(seg) - t < 17 + nv:
                    raise JpegError("DHT")
                huff[(tc, th)] = _huff(bits, list(seg[t + 17:t + 17 + nv]))
                t += 17 + nv
        elif m == 0xDB:
            t = 0
            while t < len(seg):
                if seg[t] >> 4 != 0 or seg[t] & 15 > 3 or len(seg) - t < 65:
                    raise JpegError("DQT")
                tab = np.zeros(64, np.uint16)
                tab[ZIGZAG] = list(seg[t + 1:t + 65])
                qt[seg[t] & 15] = tab
                t += 65
        elif m == 0xDD:
            if L != 4:
                raise JpegError("DRI")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDC:
            raise JpegError("DNL")
        elif m == 0xDA:
            if sof is None or len(seg) < 1:
                raise JpegError("SOS")
            W, H, nc, sampling, comps = sof
            if seg[0] != nc or len(seg) != 4 + 2 * nc:
                raise JpegError("several scans")
            sel = []
            for c in range(nc):
                if seg[1 + 2 * c] != comps[c][0]:
                    raise JpegError("scan order")
                sel.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
                if sel[-1][0] > 3 or sel[-1][1] > 3:
                    raise JpegError("table id")
            if tuple(seg[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
                raise JpegError("spectral selection")
            break
    if nc == 3:
        if adobe is not None and adobe != 1:
            raise JpegError("Adobe transform")
        if not jfif and adobe is None and bytes(c[0] for c in comps) == b"RGB":
            raise JpegError("RGB components")
    for key, (bits, vals) in STD_TABLES.items():
        if key not in huff:
            huff[key] = _huff(bits, vals)
    for c in range(nc):
        if comps[c][2] not in qt or (0, sel[c][0]) not in huff or (1, sel[c][1]) not in huff:
            raise JpegError("undefined table")
    return dict(width=W, height=H, ncomp=nc, sampling=sampling, restart=restart, scan_offset=p,
                qt=[qt[comps[c][2]] for c in range(nc)], dc=[huff[(0, sel[c][0])] for c in range(nc)],
                ac=[huff[(1, sel[c][1])] for c in range(nc)])


class _Bits:
    """the entropy-coded segment bit by bit: FF 00 is the byte FF, FF + anything else is a marker and ends the data"""

    def __init__(self, b, pos):
        self.b, self.pos, self.cur, self.left = b, pos, 0, 0

    def bit(self):
        if self.left == 0:
            b, p = self.b, self.pos
            if p >= len(b):
                raise JpegError("data ends early")
            if b[p] == 0xFF:
                if p + 1 >= len(b) or b[p + 1] != 0:
                    raise JpegError("data ends early")
                self.pos += 1
            self.pos += 1
            self.cur, self.left = b[p], 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in table:
                return table[(l, code)]
        raise JpegError("code past 16 bits")


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy_decode(b):
    b = bytes(b)
    info = parse(b)
    W, H, nc = info["width"], info["height"], info["ncomp"]
    g = geometry(W, H, info["sampling"])
    info.update(g)
    coef = np.zeros((g["total_blocks"], 64), np.int16)
    off = np.concatenate([[0], np.cumsum(g["blocks"])])
    bits = _Bits(b, info["scan_offset"])
    pred = [0] * nc
    ri, mcu = info["restart"], 0
    for my in range(g["mcus_y"]):
        for mx in range(g["mcus_x"]):
            if ri and mcu and mcu % ri == 0:
                bits.left = 0                       # the padding of the last byte
                p = bits.pos
                if p + 1 >= len(b) or b[p] != 0xFF:
                    raise JpegError("wrong restart marker")
                while p + 1 < len(b) and b[p + 1] == 0xFF:
                    p += 1
                if p + 1 >= len(b) or b[p + 1] != 0xD0 + ((mcu // ri - 1) & 7):
                    raise JpegError("wrong restart marker")
                bits.pos = p + 2
                pred = [0] * nc
            mcu += 1
            for c in range(nc):
                ch, cv = (g["hs"], g["vs"]) if c == 0 else (1, 1)
                q = info["qt"][c].astype(np.int64)
                for by in range(cv):
                    for bx in range(ch):
                        out = coef[off[c] + (my * cv + by) * g["blocks_x"][c] + mx * ch + bx]
                        s = bits.symbol(info["dc"][c])
                        if s > 11:
                            raise JpegError("DC category")
                        pred[c] += _extend(bits.bits(s), s) if s else 0
                        if abs(pred[c]) > 32767 or abs(pred[c] * q[0]) > 32767:
                            raise JpegError("coefficient range")
                        out[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(info["ac"][c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise JpegError("coefficient index past 63")
                            v = _extend(bits.bits(s), s)
                            if abs(v * q[ZIGZAG[k]]) > 32767:
                                raise JpegError("coefficient range")
                            out[ZIGZAG[k]] = v
                            k += 1
    return coef, np.stack(info["qt"]).astype(np.uint16), info


def _idct_1d(x, shift):
    """libjpeg's jidctint pass over the LAST axis of an int64 array [..., 8]"""
    i = [x[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, q):
    """coef int16 [n, 64], q [64] -> uint8 [n, 8, 8]"""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    x = _idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)        # columns first
    x = _idct_1d(x, 18)                                              # then rows
    return np.clip(x + 128, 0, 255).astype(np.uint8)


def _plane(blocks, by, bx):
    return blocks.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _up_h2v1(c):
    c = c.astype(np.int64)
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out


def _up_h2v2(c):
    c = c.astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    for v, other in ((0, up), (1, down)):
        cs = 3 * c + other
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + left + 8) >> 4
        out[v::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(coef, qt, H, W, sampling):
    g = geometry(W, H, sampling)
    off = np.concatenate([[0], np.cumsum(g["blocks"])])
    planes = [_plane(idct_blocks(coef[off[c]:off[c + 1]], qt[c]), g["blocks_y"][c], g["blocks_x"][c]) for c in range(g["ncomp"])]
    y = planes[0][:H, :W].astype(np.int64)
    if sampling == GRAY:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
    ch, cw = -(-H // g["vs"]), -(-W // g["hs"])
    cbcr = []
    for pl in planes[1:]:
        pl = pl[:ch, :cw]
        if sampling == S422:
            pl = _up_h2v1(pl)
        elif sampling == S420:
            pl = _up_h2v2(pl)
        cbcr.append(pl[:H, :W].astype(np.int64) - 128)
    cb, cr = cbcr
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    gch = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, gch, b], -1), 0, 255).astype(np.uint8)


def decode(b):
    coef, qt, info = entropy_decode(b)
    return reconstruct(coef, qt, info["height"], info["width"], info["sampling"])
