"""Inputs of the temporal-clique tests (test_temporal_clique_cpu.py / test_temporal_clique_gpu.py) and their reference runs.

Two levers make a case exact: a VISIBLE frame takes its marker positions from the labels (px = 8 * label + 4), so a test that makes every
frame visible writes r0, c0, r1, c1 itself; and nt = 2, nj = 1 is ONE pair, wt_loss = (relu(D - wt_max) + wt_max) * w * C, from which the
pair's flow weight can be read back.  Hidden frames take their positions from the soft-argmax of sharp peaks (+14 on one cell of a
low-noise map), which is where the gradient goes.  Every reference run is cached: it is computed once and shared."""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

STRIDE = 8.0
N_TOT, N_VIS_TOT = 500.0, 37.0
F32 = np.float32


def px_to_label(p):
    """label (map units, float32) whose position 8 * label + 4, rounded to float32 as the kernel rounds it, is returned with it"""
    t = F32((np.float64(p) - 4.0) / 8.0)
    return t, F32(np.float64(t) * 8.0 + 4.0)


def wavy_field(n, Hin, Win, base=1.6):
    """flow magnitude > 1 everywhere (so d w / d m != 0), different in every frame pair, with a gradient in both directions"""
    yy, xx = np.mgrid[0:Hin, 0:Win]
    return np.stack([base + 0.5 * np.sin(xx / 9.0 + t) * np.cos(yy / 7.0 + 0.3 * t) for t in range(n)]).astype(F32)


@dataclass
class Case:
    name: str
    nt: int
    H: int
    W: int
    nj: int
    batch: dict
    pred: np.ndarray
    loc: np.ndarray
    wt: float = 50.0
    wt_max: float = 0.0
    extra: dict = field(default_factory=dict)

    def hyper(self, **kw):
        from deepgraphpose_amd.loss import DGPHyper
        return DGPHyper(**dict(dict(gm2=0, gm3=0, wt=self.wt, wt_max=self.wt_max), **kw))

    def cfg(self, **kw):
        nj = self.nj
        c = dict(nj=nj, S0=np.zeros((0, nj)), ws=np.zeros(0), ws_max=np.zeros(0), stride=STRIDE, gamma=1.0, gauss_len=1, lengthscale=1.0,
                 gm2=0, gm3=0, wn_visible=5.0, wn_hidden=3.0, locref_loss_weight=0.05, locref_huber_loss=True, n_frames_total=N_TOT,
                 n_visible_frames_total=N_VIS_TOT, wt=self.wt, wt_max=self.wt_max, wt_zero_dist_grad=True)
        c.update(kw)
        return c


def _batch(nt, H, W, nj, vis_frames, labels, vf, mask=None):
    from deepgraphpose_amd import dataset as D
    vis_frames = np.asarray(vis_frames, dtype=int)
    hid_frames = np.setdiff1d(np.arange(nt), vis_frames)
    labels = np.asarray(labels, dtype=np.float64).reshape(len(vis_frames), nj, 2)
    vm, hm, vt = D.gen_idx_chunk(vis_frames, hid_frames, labels)
    z = np.zeros((nt, H, W, 2 * nj), dtype=np.float32)
    b = dict(targets=labels, locref_map=z, locref_mask=z.copy(), visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt, nt=nt,
             vector_field=np.asarray(vf, dtype=F32))
    if mask is not None:
        b["wt_batch_mask"] = np.asarray(mask, dtype=F32)
    return b


def one_pair(name, p0, p1, vf, H=12, W=16, wt=50.0, wt_max=0.0, seed=0):
    """nt = 2, nj = 1, both frames visible: the pair's positions are p0 = (r0, c0) and p1 = (r1, c1) px (rounded to what float32 labels give)"""
    rng = np.random.default_rng(seed)
    lab = [[px_to_label(p0[0])[0], px_to_label(p0[1])[0]], [px_to_label(p1[0])[0], px_to_label(p1[1])[0]]]
    pred = rng.standard_normal((2, H, W, 1)).astype(F32)
    loc = rng.standard_normal((2, H, W, 2)).astype(F32)
    return Case(name, 2, H, W, 1, _batch(2, H, W, 1, [0, 1], lab, np.asarray(vf)[None] if np.ndim(vf) == 2 else vf), pred, loc, wt, wt_max)


def peaks(name, H, W, cells, vis_labels, vf, mask, wt, wt_max, seed=0, height=14.0, extra=None):
    """frame 0 visible at vis_labels [nj, 2]; frames 1.. hidden, frame n joint j peaking at cells[n-1][j] = (row, col)"""
    rng = np.random.default_rng(seed)
    nt, nj = len(cells) + 1, len(cells[0])
    pred = (0.01 * rng.standard_normal((nt, H, W, nj))).astype(F32)
    for n, row in enumerate(cells):
        for j, (r, c) in enumerate(row):
            pred[n + 1, r, c, j] += height
    loc = rng.standard_normal((nt, H, W, 2 * nj)).astype(F32)
    return Case(name, nt, H, W, nj, _batch(nt, H, W, nj, [0], [vis_labels], vf, mask), pred, loc, wt, wt_max, extra or {})


@functools.lru_cache(maxsize=None)
def reference(case_name, weight_grad=True, coord="float32"):
    """-> dict(loss {name: float}, grad [nt,H,W,nj] float64 (d total / d pred), info (P, D, m, clamped, rows, cols, w per pair))"""
    from oracle import dgp_train_oracle as T
    c = CASES[case_name]()
    pt = torch.tensor(c.pred, dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(c.loc, dtype=torch.float64, requires_grad=True)
    L = T.dgp_loss(pt, lt, c.batch, c.cfg(wt_weight_grad=weight_grad, wt_coord_dtype=np.dtype(coord)))
    L["total_loss"].backward()
    info = L.pop("_wt_info")
    L.pop("_mu")
    return dict(loss={k: float(v.detach()) for k, v in L.items()}, grad=pt.grad.numpy().copy(), info=info)


def near_tie(info, mask):
    """True if an unmasked pair's two rows or two columns differ by less than 1e-3 px without being equal.  Which of two positions is the
    minimum, and whether they tie, is a float32 decision in the kernel; a hidden position is the kernel's float32 soft-argmax, a few ulp
    (1e-6 px) from the oracle's, so below that resolution the reference cannot say which way the kernel decides.  Two frames that peak in
    the same row differ there by the maps' noise only; the gradient cases keep such pairs out (an exact tie is grad_tie's subject)."""
    d = np.abs(info["P"][:-1] - info["P"][1:])[np.asarray(mask, dtype=bool)]
    return bool(((d > 0) & (d < 1e-3)).any())


def case(name):
    return CASES[name]()


# ---------------------------------------------------------------------------------------------------------------- forward boxes
HIN, WIN = 96, 128
# the two positions test_temporal_clique_cpu.py's search finds first (float32 labels, map units): the box ends on the frame's bottom /
# right edge and the fused float32 coordinate of the last row / column lands above Hin - 1 / Win - 1
DROP_BOTTOM_LABEL = 10.589323043823242
DROP_RIGHT_LABEL = 14.948661804199219


def _vf1():
    return wavy_field(1, HIN, WIN)


BOXES = {
    # name: (p0, p1, expected clamps (y1, x1, y2, x2))
    "top": ((6.0, 40.0), (30.0, 70.0), (1, 0, 0, 0)),
    "left": ((40.0, 5.0), (60.0, 50.0), (0, 1, 0, 0)),
    "bottom": ((60.0, 40.0), (90.0, 70.0), (0, 0, 1, 0)),
    "right": ((30.0, 70.0), (50.0, 122.0), (0, 0, 0, 1)),
    "none": ((30.0, 40.0), (50.0, 70.0), (0, 0, 0, 0)),
    "corner_tl_br": ((3.0, 4.5), (92.0, 125.0), (1, 1, 1, 1)),
    "corner_br_tl": ((92.0, 125.0), (3.0, 4.5), (1, 1, 1, 1)),
    "corner_tr_bl": ((5.0, 121.0), (90.5, 7.0), (1, 1, 1, 1)),
    "corner_bl_tr": ((90.5, 7.0), (5.0, 121.0), (1, 1, 1, 1)),
    "whole_frame": ((0.0, 0.0), (96.0, 128.0), (1, 1, 1, 1)),
    "same_row": ((44.0, 30.0), (44.0, 80.0), (0, 0, 0, 0)),
    "same_col": ((30.0, 61.0), (70.0, 61.0), (0, 0, 0, 0)),
}
CASES = {}
for _n, (_p0, _p1, _cl) in BOXES.items():
    CASES["box_" + _n] = functools.partial(one_pair, "box_" + _n, _p0, _p1, _vf1())


def _outside(name, p0, p1):
    return one_pair(name, p0, p1, wavy_field(1, 75, 83), H=10, W=11)


CASES["outside_row"] = functools.partial(_outside, "outside_row", (78.5, 40.0), (60.0, 52.0))          # r0 > Hin = 75
CASES["outside_col"] = functools.partial(_outside, "outside_col", (30.0, 86.25), (44.0, 70.0))         # c0 > Win = 83
CASES["outside_both_rows"] = functools.partial(_outside, "outside_both_rows", (78.5, 40.0), (79.75, 52.0))
CASES["drop_bottom"] = lambda: one_pair("drop_bottom", (DROP_BOTTOM_LABEL * 8 + 4, 40.0), (DROP_BOTTOM_LABEL * 8 + 4, 60.0), _vf1())
CASES["drop_right"] = lambda: one_pair("drop_right", (40.0, DROP_RIGHT_LABEL * 8 + 4), (60.0, DROP_RIGHT_LABEL * 8 + 4), _vf1())
CASES["m_below_1"] = lambda: one_pair("m_below_1", (30.0, 40.0), (50.0, 70.0), np.full((HIN, WIN), 0.999, F32))
CASES["m_above_1"] = lambda: one_pair("m_above_1", (30.0, 40.0), (50.0, 70.0), np.full((HIN, WIN), 1.001, F32))
CASES["zero_field"] = lambda: one_pair("zero_field", (30.0, 40.0), (50.0, 70.0), np.zeros((HIN, WIN), F32))
CASES["hin_1"] = lambda: one_pair("hin_1", (30.0, 40.0), (50.0, 70.0), wavy_field(1, 1, WIN))
CASES["win_1"] = lambda: one_pair("win_1", (30.0, 40.0), (50.0, 70.0), wavy_field(1, HIN, 1) + F32(0.2) * np.cos(np.arange(HIN, dtype=F32))[None, :, None])
CASES["hin_win_1"] = lambda: one_pair("hin_win_1", (30.0, 40.0), (50.0, 70.0), np.full((1, 1), 1.7, F32))
# relu kink: a 3-4-5 displacement in map units is D = 40 px exactly
for _n, _wm in (("below", 50.0), ("at", 40.0), ("above", 30.0)):
    CASES["kink_" + _n] = functools.partial(one_pair, "kink_" + _n, (28.0, 36.0), (28.0 + 24.0, 36.0 + 32.0), _vf1(), wt_max=_wm)

# ---------------------------------------------------------------------------------------------------------------- gradients
BIG_WT = 1e8          # the temporal term dominates d total / d pred
_VIS = [[2.25, 3.125], [8.5, 11.0]]
GRAD_CELLS = {
    # frames 1 and 2 hidden, two joints; cells (row, col) on the 12 x 16 map
    "inactive": ([[(4, 5), (6, 10)], [(7, 9), (4, 8)]], [0, 1], ((0, 0, 0, 0), (0, 0, 0, 0))),
    "top_bottom": ([[(0, 5), (11, 10)], [(11, 9), (0, 12)]], [0, 1], ((1, 0, 1, 0), (1, 0, 1, 0))),
    "left_right": ([[(4, 0), (6, 15)], [(7, 15), (5, 0)]], [0, 1], ((0, 1, 0, 1), (0, 1, 0, 1))),
    "visible_hidden": ([[(6, 8), (4, 5)], [(7, 9), (3, 6)]], [1, 0], None),
}
# wt_max between the unmasked pairs' distances (px; every case asserts the reference's D on either side of it)
WTMAX_MID = {"inactive": 30.0, "top_bottom": 85.0, "left_right": 115.25, "visible_hidden": 55.0}
for _n, (_cells, _mask, _cl) in GRAD_CELLS.items():
    for _k, _wm in (("weight_only", 1000.0), ("wtmax0", 0.0), ("wtmax_mid", WTMAX_MID[_n])):
        CASES["grad_%s_%s" % (_n, _k)] = functools.partial(peaks, "grad_%s_%s" % (_n, _k), 12, 16, _cells, _VIS, wavy_field(2, HIN, WIN), _mask,
                                                           BIG_WT, _wm)
GRAD_CASES = ["grad_%s_%s" % (n, k) for n in GRAD_CELLS for k in ("weight_only", "wtmax0", "wtmax_mid")]


def _tie():
    c = peaks("grad_tie", 12, 16, [[(5, 6), (7, 11)], [(5, 6), (7, 11)]], _VIS, wavy_field(2, HIN, WIN), [0, 1], BIG_WT, 6.0)
    c.pred[2] = c.pred[1]           # bitwise identical maps: r0 == r1, c0 == c1, D == 0
    return c


CASES["grad_tie"] = _tie


def _many_pairs():
    """nt = 14, nj = 20: 260 pairs, beyond one pass of loss_temporal's 256 threads; frames 0 and 7 visible.  Peaks and labels stay out of
    the last row and column, so no box ends on the bottom or right edge (the top and left clamps are active in many): whether such a
    box loses its last sample depends on the last bit of the position (oracle/dgp_train_oracle.py _crop_axis), and a hidden position
    is the kernel's float32 soft-argmax, a few ulp from the oracle's."""
    rng = np.random.default_rng(260)
    nt, H, W, nj = 14, 6, 8, 20
    from deepgraphpose_amd import dataset as D
    vis = np.array([0, 7])
    lab = np.stack([rng.uniform(0.5, H - 2.5, (2, nj)), rng.uniform(0.5, W - 2.5, (2, nj))], -1).astype(F32)
    pred = (0.01 * rng.standard_normal((nt, H, W, nj))).astype(F32)
    cell = np.zeros((nt, nj, 2), dtype=int)
    for n in range(nt):
        for j in range(nj):
            while True:          # another row AND another column than in the frame before (see near_tie)
                cell[n, j] = rng.integers(0, H - 1), rng.integers(0, W - 1)
                if n == 0 or (cell[n, j] != cell[n - 1, j]).all():
                    break
            pred[n, cell[n, j, 0], cell[n, j, 1], j] += 12.0
    loc = rng.standard_normal((nt, H, W, 2 * nj)).astype(F32)
    mask = np.ones(nt - 1)
    mask[4] = 0
    return Case("grad_260_pairs", nt, H, W, nj, _batch(nt, H, W, nj, vis, lab, wavy_field(nt - 1, 48, 64), mask), pred, loc, BIG_WT, 12.0)


CASES["grad_260_pairs"] = _many_pairs


def _beyond_lds():
    """136 x 240 maps (test_loss_on_maps_beyond_the_lds_limit_matches_autograd's shape: loss_ce_backward streams), the peaks inside a
    272 x 480 field (a quarter of stride * H x stride * W) so that the float64 oracle stays within a few seconds; +20 on the peak's
    cell, since the softmax's tail over 32 640 cells would pull a +14 peak several cells towards the centre"""
    nt, H, W, nj = 3, 136, 240, 4
    rng = np.random.default_rng(136)
    cells = [[(int(rng.integers(0, 32)), int(rng.integers(0, 58))) for _ in range(nj)] for _ in range(nt - 1)]
    cells[0][0], cells[1][0] = (0, 7), (33, 3)              # top clamp; bottom clamp (33 * 8 + 4 + 10 >= 272)
    lab = np.stack([rng.uniform(2, 30, nj), rng.uniform(2, 55, nj)], -1).astype(F32)
    return peaks("grad_beyond_lds", H, W, cells, lab, wavy_field(nt - 1, 272, 480), [1, 1], BIG_WT, 220.0, seed=137, height=20.0)


CASES["grad_beyond_lds"] = _beyond_lds
