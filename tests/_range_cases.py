"""Case tables and float64 references of tests/test_range_tracking_gpu.py (numpy only; checked without a GPU by tests/test_range_cases_cpu.py).

The contract under test: the maximum of a tensor's ABSMAX_SLOTS floats is the maximum of |y| over every REAL element of the tensor and of
nothing else.  A dense random tensor has its maximum at one random element, so an epilogue that leaves a fraction f of its elements out
fails such a case with probability f.  Here every launch has ONE planted extreme that dominates everything else by a factor of four, and
the plant visits the places where ownership of elements changes hands: tile, wave and row-block seams, ragged last tiles, padded
columns, high row tiles of grids larger than the resident workgroups, tiles of a persistent workgroup's later rounds, the tiles a fix-up kernel owns, pixels whose X' is not stored.

How an extreme is planted so that it reaches ONE output element and the float64 reference needs no second product:

  residual   layers with a residual: the residual is zero but for V = 64 (-64 without ReLU, so that fabsf is needed) at the target,
             ref = base[m, c] +- V.
  wire       layers without one (stride-2 convs; R2, X' and R1' of the chain and unit kernels): one input channel is a "wire": it is
             zero at every pixel, its weight rows are zero but for a single 1.0 (the centre tap) into the target column, and the plant is
             V at one pixel of that channel.  In the fused kernels the wire runs on through X' into R1': the wire columns have scale 1,
             bias 0 and no other weight, so R2 = X' = R1' = V EXACTLY at the planted pixel (also through the fp16 cells of the 16-bit
             tier), and one launch checks all its slot sets.

Operands are exact in both cell formats by construction (activations on a grid of 1/16 below 16, weights on a grid of 2^-10, V a power
of two; the 16-bit tier's weight rounding, fp16 on the panel's power-of-two scale as in tests/test_h1_gpu.py, is applied all the same
and changes nothing), so `base` is float64 on what the kernels hold.  The base recipe is the suite's: x = relu(randn) * 3, w ~ N(0, 1 / K), scale 1 +- 0.1, bias +- 0.1, integer seeds."""
import math

import numpy as np

TOL = 1e-4           # the project's bound for a range tracked in fp32 before the cell rounding (tests/test_h2_gpu.py)
V = 64.0             # the planted extreme
DOMINANCE = 4.0      # ref_max >= DOMINANCE * runner-up: an omitted plant shows as an error of at least 75 %
BM = BN = 128        # rows / columns of every split-family and fp32 tile the cases land on (asserted through mtiles / ntiles)
COUT = 136           # one full column tile and a ragged one of 8 real channels
N_CU_CPU = 256       # the CPU checks plan for an MI355X


def grid16(a):
    return (np.round(np.asarray(a, np.float64) * 16.0) / 16.0).astype(np.float32)


def grid1024(a):
    """weights on a grid of 2^-10: below 1 they have at most 10 significant bits, so the 16-bit tier's fp16 panel holds them exactly"""
    return (np.round(np.asarray(a, np.float64) * 1024.0) / 1024.0).astype(np.float32)


def w_exp(w_max):
    """exponent of an H1 weight panel's power-of-two scale (tests/test_h1_gpu.py)"""
    return 14 - (math.frexp(float(w_max))[1] - 1)


def h1_weights(w, w_max):
    e = w_exp(w_max)
    return (w.astype(np.float64) * 2.0 ** e).astype(np.float16).astype(np.float64) * 2.0 ** -e


def out_hw(H, W, k, stride, d):
    pad = d * (k - 1) // 2
    return (H + 2 * pad - (k - 1) * d - 1) // stride + 1, (W + 2 * pad - (k - 1) * d - 1) // stride + 1


def conv_f64(x, w, stride=1, d=1):
    """float64 conv, padding d (k - 1) / 2: x [N,H,W,Cin], w [k,k,Cin,Cout] -> [N Ho Wo, Cout], tap by tap"""
    N, H, W, Cin = x.shape
    k = w.shape[0]
    pad = d * (k - 1) // 2
    Ho, Wo = out_hw(H, W, k, stride, d)
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, Cin), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    acc = np.zeros((N * Ho * Wo, w.shape[3]), np.float64)
    for a in range(k):
        for b in range(k):
            cols = xp[:, a * d:a * d + (Ho - 1) * stride + 1:stride, b * d:b * d + (Wo - 1) * stride + 1:stride]
            acc += cols.reshape(N * Ho * Wo, Cin) @ w[a, b].astype(np.float64)
    return acc


class Top2:
    """the two largest values of a non-negative array and where the largest is: the runner-up of a plant at any element"""

    def __init__(self, a):
        flat = a.reshape(-1)
        self.arg = int(flat.argmax())
        self.top = float(flat[self.arg])
        rest = np.delete(flat, self.arg) if flat.size > 1 else np.zeros(1)
        self.second = float(rest.max())

    def without(self, flat_index):
        return self.second if flat_index == self.arg else self.top


# ------------------------------------------------------------------------------------------------------------------ conv layers
# name -> entry: "f32" (engine.conv2d) / "cells" (conv2d_h2 and conv2d_h1, one case per tier); shape: (N, H, W) or a key of conv_shape();
# res: how the plant travels ("f32" / "cells": residual of that kind on the output grid, "cells2": cell residual on the 2x finer grid,
# None: the wire); ycells: cell output; want: plan fields (a callable of n_cu, or per tier); env: switches the case needs (a child process)
CONV_CASES = {
    "f32_unranged_big": dict(entry="f32", ranged=False, shape="rounds", cin=64, k=1, relu=True, res="f32",
                             want=lambda n: dict(family=2, tile=10, mode=2, tail_ksplit=0)),
    "f32_unranged_cin16": dict(entry="f32", ranged=False, shape=(2, 17, 23), cin=16, k=3, relu=False, res="f32", want=lambda n: dict(family=0)),
    "f32_unranged_s2_wire": dict(entry="f32", ranged=False, shape=(2, 17, 23), cin=64, k=3, stride=2, relu=True, res=None,
                                 want=lambda n: dict(family=2, tile=10, mode=1)),
    "f32_ranged_big": dict(entry="f32", ranged=True, shape="rounds", cin=64, k=1, relu=True, res="f32",
                           want=lambda n: dict(family=2, tile=16, cs=0, mode=2, tail_ksplit=0)),
    "f32_ranged_3x3": dict(entry="f32", ranged=True, shape=(2, 17, 23), cin=64, k=3, relu=False, res="f32",
                           want=lambda n: dict(family=2, tile=16, cs=0, mode=1)),
    "f32_ranged_tail": dict(entry="f32", ranged=True, shape="rounds", cin=256, k=1, relu=True, res="f32", slab=True,
                            want=lambda n: dict(family=2, tile=16, cs=0, tail_ksplit=2, n_main=2 * n)),
    "pw_big": dict(entry="cells", shape="rounds", cin=64, k=1, relu=True, res="cells", ycells=True, want=lambda n: dict(mode=2, deep=0, tail_ksplit=0)),
    "pw_f32out": dict(entry="cells", shape=(1, 1, 700), cin=64, k=1, relu=False, res={"h2": "f32", "h1": None}, ycells=False,
                      want=lambda n: dict(mode=2, deep=0, oh2=0)),
    "pw_res_s2": dict(entry="cells", shape=(2, 17, 23), cin=64, k=1, relu=True, res="cells2", ycells=True, want=lambda n: dict(mode=2, deep=0)),
    "pw_deep_ring": dict(entry="cells", tiers=("h2",), shape=(1, 1, 700), cin=256, k=1, relu=True, res="cells", ycells=True,
                         want=lambda n: dict(mode=2, deep=1)),
    "tap_3x3": dict(entry="cells", shape=(2, 5, 116), cin=64, k=3, relu=True, res="cells", ycells=True,
                    want={"h2": lambda n: dict(mode=1, deep=1), "h1": lambda n: dict(mode=1, deep=0)}),
    "tap_s2_wire": dict(entry="cells", shape=(2, 17, 23), cin=64, k=3, stride=2, relu=True, res=None, ycells=True,
                        want={"h2": lambda n: dict(mode=1, deep=1), "h1": lambda n: dict(mode=1, deep=0)}),
    "halo_walk": dict(entry="cells", shape="walk", cin=64, k=3, relu=True, res="cells", ycells=True, want=lambda n: dict(mode=3, deep=0, tail_ksplit=0)),
    "tail_h2": dict(entry="cells", tiers=("h2",), shape="rounds", cin=256, k=1, relu=True, res="cells", ycells=True, slab=True,
                    env={"DGP_TAIL_SPLIT": "2"}, want=lambda n: dict(mode=2, deep=0, tail_ksplit=2, n_main=2 * n)),
}
SLAB_FLOATS = (64 << 20) // 4


def conv_shape(shape, n_cu):
    """"rounds": 2 n_cu tiles (two column tiles each), as many as the CUs hold at once, and three more row tiles, the last one ragged --
    more tiles than resident workgroups, and with a slab the K-split tail; "walk": 46 x 47 frames on more than one tile per CU (the halo walk's domain)"""
    if shape == "rounds":
        return 1, 1, BM * (n_cu + 3) - 50
    if shape == "walk":
        return -(-(BM // 2) * (n_cu + 8) // (46 * 47)), 46, 47
    return tuple(shape)


def conv_case_ids():
    out = []
    for name, c in CONV_CASES.items():
        for tier in (("f32",) if c["entry"] == "f32" else c.get("tiers", ("h2", "h1"))):
            out.append((name, tier))
    return out


def conv_want(name, tier, n_cu):
    c = CONV_CASES[name]
    w = c["want"][tier] if isinstance(c["want"], dict) else c["want"]
    want = dict(w(n_cu))
    if c["entry"] == "cells":
        want.update(tile=16, ah2=1, h1=int(tier == "h1"), cs=1, dma=1)
        want.setdefault("oh2", int(c["ycells"]))
    return want


def conv_plan_args(name, tier, n_cu, with_res=True):
    """keyword arguments of engine.conv2d_plan for the case (with_res=False: launched without its residual)"""
    c = CONV_CASES[name]
    N, H, W = conv_shape(c["shape"], n_cu)
    k, stride = c["k"], c.get("stride", 1)
    Ho, Wo = out_hw(H, W, k, stride, 1)
    res = c["res"][tier] if isinstance(c["res"], dict) else c["res"]
    fmt = {"f32": 0, "h2": 1, "h1": 2}[tier]
    kw = dict(x_shape=(N, H, W, c["cin"]), w_shape=(k, k, c["cin"], COUT), stride=stride, pad_t=(k - 1) // 2, pad_l=(k - 1) // 2, out_hw=(Ho, Wo),
              in_fmt=fmt, out_fmt=fmt if c.get("ycells") else 0, slab_bytes=4 * SLAB_FLOATS if c.get("slab") else 0)
    if res and with_res:
        kw.update(res_stride=2 if res == "cells2" else 1, res_hw=(2 * Ho - 1, 2 * Wo) if res == "cells2" else (Ho, Wo), res_fmt=fmt if res.startswith("cells") else 0)
    if c["entry"] == "f32":
        kw.update(ranged=c["ranged"])
    return kw


def conv_rows(M, pl):
    """name -> output row, from the plan: the seams of the first tile, tile borders, the ragged last tile, a second-round tile, the tail"""
    mt, nt = pl["mtiles"], pl["ntiles"]
    assert mt == -(-M // BM) and nt == -(-COUT // BN), (pl, M)
    rows = {"first": 0, "last": M - 1}
    for r in (31, 32, 63, 64, 95, 96, 127):
        rows["seam_%d" % r] = r
    rows["tile1_first"] = BM
    if M % BM:
        rows["last_full_tile_last"] = (M // BM) * BM - 1
        rows["ragged_first"] = (M // BM) * BM
    slots = 2 * pl["n_cu"]
    if mt * nt > slots:
        # A row tile past the first 2 n_cu / ntiles: more tiles than the 2 n_cu workgroups the CUs hold at once.  The kernels take one tile
        # per workgroup and permute block ids per XCD (and, on pointwise launches with two column tiles, walk groups of 32 row tiles
        # column-major), so this is a HIGH ROW TILE inside its interior, not a statement about which round the hardware dispatches it in.
        rows["high_row_tile"] = -(-slots // nt) * BM + 37
    if pl["tail_ksplit"] > 1:
        t0 = pl["n_main"] // nt * BM
        rows.update(tail_first=t0, tail_middle=(t0 + M) // 2, tail_last=M - 1)
    return {k: r for k, r in rows.items() if 0 <= r < M}


def conv_cols():
    return [0, 7, 8, 63, 64, 127, 128, COUT - 8, COUT - 1]


def conv_cross(M, pl):
    """[(label, row, column)]: every row at two columns, every column at two rows -- not the product"""
    rows, cols = conv_rows(M, pl), conv_cols()
    out = [(n, r, c) for n, r in rows.items() for c in (5, COUT - 1)]
    out += [("col_%d" % c, r, c) for c in cols for r in (64, M - 1)]
    return sorted(set(out), key=lambda t: (t[1], t[2]))


class ConvLayer:
    """operands (numpy, what the cells hold exactly) and the float64 base output [M, COUT] of one conv case"""

    def __init__(self, name, tier, n_cu, mode="plant"):
        c = CONV_CASES[name]
        self.name, self.tier, self.c = name, tier, c
        N, H, W = conv_shape(c["shape"], n_cu)
        self.k, self.stride, self.cin, self.relu = c["k"], c.get("stride", 1), c["cin"], c["relu"]
        self.N, self.H, self.W = N, H, W
        self.Ho, self.Wo = out_hw(H, W, self.k, self.stride, 1)
        self.M = N * self.Ho * self.Wo
        self.res = c["res"][tier] if isinstance(c["res"], dict) else c["res"]
        self.wire = self.cin - 3 if self.res is None else None
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name + tier))
        rng = np.random.default_rng(seed)
        K = self.k * self.k * self.cin
        x = rng.standard_normal((N, H, W, self.cin))
        w = rng.standard_normal((self.k, self.k, self.cin, COUT)) / np.sqrt(K)
        self.scale = (1 + 0.1 * rng.standard_normal(COUT)).astype(np.float32)
        self.bias = (0.1 * rng.standard_normal(COUT)).astype(np.float32)
        if mode == "plant":
            self.x = np.minimum(grid16(np.maximum(x, 0) * 3.0), 15.0)
            self.w = grid1024(w)
        else:
            # padding must not count: x > 0, w < 0, bias B on every channel, ReLU -- a padded row (x = 0) would give relu(B) = B, above every
            # real output; mode "zero": B < 0, every output is 0
            self.x = np.minimum(grid16(np.abs(x) * 3.0) + 1.0 / 16, 15.0)
            self.w = grid1024(-np.abs(w))
            self.relu, self.res, self.wire = True, None, None
            self.B = 16.0 * math.sqrt(K / 64.0) * (1 if mode == "padding" else -1)
            self.scale = np.abs(self.scale)
            self.bias = np.full(COUT, self.B, np.float32)
        if self.wire is not None:
            self.x[..., self.wire] = 0.0
            self.w[:, :, self.wire, :] = 0.0
        self._base = None

    def w_for(self, col=None):
        """the launch's weights: the wire's 1.0 (centre tap) into column `col`"""
        if self.wire is None:
            return self.w
        w = self.w.copy()
        w[self.k // 2, self.k // 2, self.wire, col] = 1.0
        return w

    @property
    def base(self):
        if self._base is None:
            w_max = 1.0 if self.wire is not None else float(np.abs(self.w).max())
            wq = h1_weights(self.w, w_max) if self.tier == "h1" else self.w.astype(np.float64)
            self._base = conv_f64(self.x.astype(np.float64), wq, self.stride) * self.scale.astype(np.float64) + self.bias.astype(np.float64)
            self._mag = np.maximum(self._base, 0.0) if self.relu else np.abs(self._base)
            self._top = Top2(self._mag)
        return self._base

    def ref_max(self):
        """max |y| of the layer as it stands (no plant)"""
        self.base
        return self._top.top

    def sign(self):
        return 1.0 if self.relu else -1.0

    def wire_pixel(self, m):
        """(n, h, w) of the input pixel under the centre tap of output row m"""
        n, r = divmod(m, self.Ho * self.Wo)
        ho, wo = divmod(r, self.Wo)
        return n, ho * self.stride, wo * self.stride

    def res_pixel(self, m):
        """(n, h, w) of the residual pixel output row m reads"""
        n, r = divmod(m, self.Ho * self.Wo)
        ho, wo = divmod(r, self.Wo)
        return (n, 2 * ho, 2 * wo) if self.res == "cells2" else (n, ho, wo)

    def planted(self, m, c):
        """-> (ref_max, runner_up) of the layer with the plant at output element (m, c)"""
        b = float(self.base[m, c])
        delta = self.sign() * V * (float(self.scale[c]) if self.wire is not None else 1.0)
        val = b + delta
        return (max(val, 0.0) if self.relu else abs(val)), self._top.without(m * COUT + c)


# ------------------------------------------------------------------------------------------------------------------ chain and unit kernels
# (C, C1, CIN2, res_mode) -> N, Ho, Wo of the small case; the frame seam (Ho Wo = 391 / 99 pixels) falls inside a 16-pixel row block
CHAIN_INSTANCES = {(64, 64, 0, 1): (2, 17, 23), (64, 64, 64, 0): (2, 17, 23), (64, 128, 0, 2): (2, 17, 23), (256, 256, 0, 1): (2, 9, 11)}
CHAIN_BIG = [(64, 64, 0, 1), (64, 64, 64, 0)]         # the instances that also run on more tiles than workgroups
CHAIN_TILES = (80, 96, 128)                            # pixels per tile of the chain kernels' instances (16 RB NCW, csrc/dgp_chain.hip)
# The fused kernels are persistent: a grid of n_cu x (resident workgroups per CU, from the occupancy query) walks the tiles, and a tile past
# the grid is one of a workgroup's SECOND round.  There is no plan query for them, so the big cases are sized from a hardware bound: a
# workgroup of these kernels has 9 to 12 waves (576 to 768 threads), a CU has 32 wave slots (2048 threads), so at most 3 workgroups are
# resident whatever their LDS and registers allow.  The cases take 8 n_cu tiles, more than twice that bound.
MAX_WGS_PER_CU = 3
BIG_TILES_PER_CU = 8
UNIT_INSTANCES = {(0, 1): "identity", (64, 0): "K-concatenated"}       # (CIN2, res_mode); C = C1 = 64
UNIT_TH, UNIT_TW = 8, 16                               # the unit kernel's tile: one wave per row (NCW = 8), 16 columns
UNIT_MAPS = {"ragged": (2, 13, 21), "narrow": (2, 3, 5)}
BLOCK_PIXELS = 2048                                    # the big cases repeat a block of this many pixels / of 4 frames


def chain_big_pixels(n_cu):
    return 128 * (BIG_TILES_PER_CU * n_cu + 2) - 50


def chain_pixels(N, Ho, Wo, big=False, n_cu=0):
    """name -> pixel of the flattened [N Ho Wo] list"""
    M, F = N * Ho * Wo, Ho * Wo
    px = {"first": 0, "last": M - 1, "row_block_15": 15, "row_block_16": 16, "frame_seam_a": F - 1, "frame_seam_b": F}
    for t in CHAIN_TILES:
        px["tile_%d_a" % t], px["tile_%d_b" % t] = t - 1, t
    if big:                                              # every workgroup of a grid of at most 3 n_cu has had its first tile by here
        px = {"first": 0, "last": M - 1, "second_round": max(CHAIN_TILES) * MAX_WGS_PER_CU * n_cu + 21,
              "later_round": max(CHAIN_TILES) * (BIG_TILES_PER_CU - 1) * n_cu + 77}
    return {k: p for k, p in px.items() if 0 <= p < M}


def unit_pixels(N, H, W):
    """name -> (frame, y, x): rows 0, TH - 1, TH, H - 1 at the first and last column, columns 0, 15, 16, W - 1 at the first and last row"""
    rows = sorted({r for r in (0, UNIT_TH - 1, UNIT_TH, H - 1) if r < H})
    cols = sorted({c for c in (0, UNIT_TW - 1, UNIT_TW, W - 1) if c < W})
    px = {(0, r, c) for r in rows for c in (0, W - 1)} | {(0, r, c) for c in cols for r in (0, H - 1)}
    px |= {(N - 1, H - 1, W - 1), (N - 1, 0, 0)}
    return {"f%d_y%d_x%d" % p: p for p in sorted(px)}


def unit_big_frames(n_cu, H=13, W=21):
    tiles = -(-H // UNIT_TH) * -(-W // UNIT_TW)
    return -(-(BIG_TILES_PER_CU * n_cu + 1) // tiles) + 1


class FusedLayer:
    """Operands and float64 base outputs of a chain (unit=False) or unit (unit=True) case.  Wires: channel K0 of R2 -> channel J0 of X' ->
    channel C0 of R1'; the unit's conv2 takes channel K00 of R1 to K0 (centre tap); the K-concatenated source's channel K1 goes to J0.
    Every wire column has scale 1, bias 0, no other weight, and the wire channels are zero in every input, so a plant of V arrives as
    exactly V.  mode "padding" / "zero": no wires; x > 0, w < 0, bias +-B everywhere (see ConvLayer)."""

    def __init__(self, C, C1, CIN2, res_mode, nhw, unit=False, repeat=None, mode="plant"):
        self.C, self.C1, self.CIN2, self.res_mode, self.unit, self.mode = C, C1, CIN2, res_mode, unit, mode
        N, H, W = nhw
        self.N, self.H, self.W = N, H, W
        self.M = N * H * W
        C4 = 4 * C
        self.K00, self.K0, self.J0, self.C0, self.K1 = 5, C - 9, C4 - 20, C1 - 1, 11
        rng = np.random.default_rng(C * 1000 + C1 * 10 + CIN2 + res_mode + 17 * unit + (mode != "plant") * 5)
        plant = mode == "plant"
        act = (lambda shape, s: np.minimum(grid16(np.maximum(rng.standard_normal(shape), 0) * s), 15.0)) if plant else \
            (lambda shape, s: np.minimum(grid16(np.abs(rng.standard_normal(shape)) * s) + 1.0 / 16, 15.0))
        wgt = (lambda shape, K: grid1024(rng.standard_normal(shape) / np.sqrt(K))) if plant else \
            (lambda shape, K: grid1024(-np.abs(rng.standard_normal(shape)) / np.sqrt(K)))
        sc = lambda n: (1 + 0.1 * rng.standard_normal(n)).astype(np.float32) if plant else np.abs(1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
        bi = lambda n, K: (0.1 * rng.standard_normal(n)).astype(np.float32) if plant else \
            np.full(n, 16.0 * math.sqrt(K / 64.0) * (1 if mode == "padding" else -1), np.float32)
        # the distinct pixels (a block that the big cases repeat: frames for the unit kernel, pixels for the chain)
        self.repeat = repeat
        if repeat is None:
            bshape = (N, H, W)
        else:
            bshape = (4, H, W) if unit else (1, 1, BLOCK_PIXELS)
        self.bshape = bshape
        s2shape = bshape if res_mode != 2 else (bshape[0], 2 * bshape[1] - 1, 2 * bshape[2])
        self.a_in = act(bshape + (C,), 3.0)                                   # R1 (unit) or R2 (chain)
        self.src2 = act(s2shape + (CIN2 if res_mode == 0 else C4,), 2.0)
        if not plant and res_mode != 0:
            self.src2[:] = 0.0                  # (a positive residual would lift real outputs above B)
        if unit:
            self.w2, self.s2, self.b2 = wgt((3, 3, C, C), 9 * C), sc(C), bi(C, 9 * C)
        self.w3 = wgt((C + CIN2, C4), C + CIN2)
        self.s3 = None if res_mode == 0 else sc(C4)
        self.b3 = bi(C4, C + CIN2)
        self.w1, self.s1, self.b1 = wgt((C4, C1), C4), sc(C1), bi(C1, C4)
        if plant:
            self._wires()
        self._out = None

    def _wires(self):
        K00, K0, J0, C0, K1, C = self.K00, self.K0, self.J0, self.C0, self.K1, self.C
        if self.unit:
            self.a_in[..., K00] = 0.0
            self.w2[:, :, K00, :] = 0.0
            self.w2[:, :, :, K0] = 0.0
            self.w2[1, 1, K00, K0] = 1.0
            self.s2[K0], self.b2[K0] = 1.0, 0.0
        else:
            self.a_in[..., K0] = 0.0
        self.w3[K0, :] = 0.0
        self.w3[:, J0] = 0.0
        self.w3[K0, J0] = 1.0
        if self.res_mode == 0:
            self.src2[..., K1] = 0.0
            self.w3[C + K1, :] = 0.0
            self.w3[C + K1, J0] = 1.0
        else:
            self.src2[..., J0] = 0.0
            self.s3[J0] = 1.0
        self.b3[J0] = 0.0
        self.w1[J0, :] = 0.0
        self.w1[:, C0] = 0.0
        self.w1[J0, C0] = 1.0
        self.s1[C0], self.b1[C0] = 1.0, 0.0

    def full(self, a):
        """a block array -> the launch's array (the block repeated)"""
        if self.repeat is None:
            return a
        if self.unit:
            return np.concatenate([a] * -(-self.N // a.shape[0]), 0)[:self.N]
        return np.concatenate([a] * -(-self.M // a.shape[2]), 2)[:, :, :self.M]

    def outputs(self, cells=None, wq=None):
        """float64 (R2 or None, X', R1') of the distinct pixels WITHOUT a plant, each [pixels, channels].  cells(stage, a) -> the values
        the stage's output cells hold, which the next stage consumes (default: a itself -- enough to bound a runner-up; the planted
        extremes are exact); wq(w) -> the weights the kernel holds."""
        hooks = cells is not None or wq is not None
        if self._out is None or hooks:
            f = lambda a: None if a is None else a.astype(np.float64)
            cells = cells or (lambda stage, a: a)
            wq = wq or f
            r2 = None
            a = f(self.a_in)
            if self.unit:
                r2 = np.maximum(conv_f64(a, wq(self.w2)) * f(self.s2) + f(self.b2), 0.0)
                a2 = cells("r2", r2)
            else:
                a2 = a.reshape(-1, self.C)
            P = a2.shape[0]
            if self.res_mode == 0:
                acc = np.concatenate([a2, f(self.src2).reshape(P, self.CIN2)], 1) @ wq(self.w3) + f(self.b3)
            else:
                s = f(self.src2) if self.res_mode == 1 else f(self.src2)[:, ::2, ::2]
                acc = (a2 @ wq(self.w3)) * f(self.s3) + f(self.b3) + s.reshape(P, 4 * self.C)
            x = np.maximum(acc, 0.0)
            r1 = np.maximum((cells("x", x) @ wq(self.w1)) * f(self.s1) + f(self.b1), 0.0)
            if hooks:
                return r2, x, r1
            self._out = (r2, x, r1)
        return self._out

    def base_max(self):
        """max of (R2, X', R1') without a plant (0 for the chain's missing R2)"""
        return tuple(0.0 if o is None else float(o.max()) for o in self.outputs())


def fused_layer(kind, inst, size, n_cu, mode="plant"):
    C, C1, CIN2, res = inst
    if kind == "chain":
        if size == "big":
            return FusedLayer(C, C1, CIN2, res, (1, 1, chain_big_pixels(n_cu)), repeat=True, mode=mode)
        return FusedLayer(C, C1, CIN2, res, CHAIN_INSTANCES[inst], mode=mode)
    if size == "big":
        return FusedLayer(C, C1, CIN2, res, (unit_big_frames(n_cu), 13, 21), unit=True, repeat=True, mode=mode)
    return FusedLayer(C, C1, CIN2, res, UNIT_MAPS[size], unit=True, mode=mode)


# ------------------------------------------------------------------------------------------------------------------ root block
ROOT_FRAMES = [(33, 65), (75, 101)]


ROOT_MEAN = (123.68, 116.779, 103.939)
ROOT_B = 64.0          # bias of the root block's padding case
ROOT_BATCH = 3


def root_weights(mode="plant"):
    """(w [7,7,3,64], bn_scale [64], bn_bias [64]) float32.
    "plant": positive weights, heaviest at the centre tap, and a negative bias -- a dark frame gives 0, and the conv1 pixel whose window
    is centred on the bright patch beats every pixel that sees the patch off centre.
    "padding" / "zero": all-negative weights and the bias +-ROOT_B on every channel, for frames of 255 (u8 - mean > 0): real conv1 values
    are relu(B - something), largest at the map's corners, where zero padding leaves 16 of 49 taps; a conv1 pixel or pool element
    outside the map that were counted would report relu(B) = B.  With -B everything is 0."""
    rng = np.random.default_rng(4711)
    w = np.abs(rng.standard_normal((7, 7, 3, 64)))
    sc = (rng.random(64) * 0.5 + 0.75).astype(np.float32)
    if mode == "plant":
        w = w * 0.01 + 0.002
        w[3, 3] = 1.0 + rng.random((3, 64))
        bi = -rng.random(64) * 4.0 - 2.0
    else:
        w = -(w * 0.002 + 0.0005)
        bi = np.full(64, ROOT_B if mode == "padding" else -ROOT_B)
    return w.astype(np.float32), sc, bi.astype(np.float32)


def root_frames(H, W, target=None, bright=False):
    """uint8 [ROOT_BATCH, H, W, 3]: dark frames (the mean pixel) with the 3 x 3 patch of `target` = (frame, pool row, pool column) at 255,
    or frames of 255 throughout"""
    f = np.empty((ROOT_BATCH, H, W, 3), np.uint8)
    f[:] = 255 if bright else np.array([124, 117, 104], np.uint8)
    if target is not None:
        b, qy, qx = target
        y0, y1, x0, x1, _ = root_patch(H, W, qy, qx)
        f[b, y0:y1, x0:x1] = 255
    return f


def root_reference(frames, weights, cells, device="cpu"):
    """float64 root block on what the kernel of `cells` ("h2" / "h1") holds (tests/_h1_ref.root_forward, on any device)
    -> per pool cell maxima over the channels, numpy [B, HP, WP]"""
    import torch
    import _h1_ref as R
    t = lambda a: torch.from_numpy(a).to(device)
    _, pool = R.root_forward(t(frames), t(weights[0]), t(weights[1]), t(weights[2]), ROOT_MEAN, cells)
    return pool.amax(3).cpu().numpy()


def root_dominance(per_cell, target):
    """-> (ref_max, runner-up, the maximum lies in the target cell) of a planted root-block case"""
    b, qy, qx = target
    flat = per_cell.reshape(-1).copy()
    arg = int(flat.argmax())
    ref = float(flat[arg])
    flat[arg] = 0.0
    return ref, float(flat.max()), arg == (b * per_cell.shape[1] + qy) * per_cell.shape[2] + qx


def pool_geometry(n):
    out = (n + 1) // 2
    return out, max(0, (out - 1) * 2 + 3 - n) // 2


def root_targets(H, W, B=ROOT_BATCH):
    """name -> (frame, pool row, pool column): the four corners, an interior cell, a cell of the last frame"""
    HP, _ = pool_geometry((H + 1) // 2)
    WP, _ = pool_geometry((W + 1) // 2)
    return {"top_left": (0, 0, 0), "top_right": (0, 0, WP - 1), "bottom_left": (0, HP - 1, 0), "bottom_right": (0, HP - 1, WP - 1),
            "interior": (1, HP // 2, WP // 2 + 1), "last_frame": (B - 1, HP - 2, 1)}


def root_patch(H, W, qy, qx):
    """The frame patch (y0, y1, x0, x1, clipped to the frame) that lights ONE conv1 pixel, the one that lies in pool cell (qy, qx) and in
    no other -- the middle element of the cell's 3 x 3 / 2 window (2 q - pad + 1): the 3 x 3 pixels around the centre of its 7 x 7 window.
    (A 9 x 9 patch covers the window centres of the neighbouring conv1 pixels as well, which lie in the neighbouring pool cells: the
    maximum would be shared, and a cell left out would not show.  The weights of the case are heaviest at the centre tap.)"""
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    _, pt = pool_geometry(H1)
    _, pl = pool_geometry(W1)
    y, x = 2 * qy - pt + 1, 2 * qx - pl + 1
    assert 0 <= y < H1 and 0 <= x < W1, (H, W, qy, qx)
    cy, cx = 2 * y - conv1_pad(H) + 3, 2 * x - conv1_pad(W) + 3
    assert 0 <= cy < H and 0 <= cx < W
    return max(0, cy - 1), min(H, cy + 2), max(0, cx - 1), min(W, cx + 2), (y, x)


def conv1_pad(n):
    """padding in front of the 7 / 2 conv of conv2d_same: total 5 after the fixed padding, smaller half first"""
    out = (n + 1) // 2
    return max(0, (out - 1) * 2 + 7 - n) // 2


PAD_CASES = ["f32_unranged_big", "f32_unranged_cin16", "f32_ranged_3x3", "f32_ranged_tail", "pw_big", "pw_f32out", "tap_3x3", "halo_walk", "tail_h2"]


def pad_case_ids():
    return [(n, t) for n, t in conv_case_ids() if n in PAD_CASES]
