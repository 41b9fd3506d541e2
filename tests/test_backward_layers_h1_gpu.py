"""Layer-level tests of the 16-bit tier's backward kernels against float64 ON THE SAME fp16 OPERANDS: wgrad_dma_h1, the H1 -> H1 data
gradient (H1 gate, H1 residual on the same and on the coarse grid, predicted scales, the zero-stuffed stride-2 form), the fused stem weight
gradient (stem_wgrad_h1_kernel + stem_wgrad_reduce_kernel), the merged heads' backward and the predicted-scale converters.

test_backward_layers_gpu.py holds the parity tier's kernels to 1e-5; the 16-bit tier was only judged through the whole network, by the
bands of a reported tier (cosine >= 0.999, 3e-2 per tensor).  Its kernels' arithmetic allows the parity bound: products of two fp16 values
are exact in fp32 and the accumulation is the same fp32 MFMA + float atomics.  Every case therefore
  1. asserts that the H1 tensors the entry point left behind equal tests/_h1_ref.h1(x, predicted scale) BIT FOR BIT,
  2. compares the result with float64 arithmetic on those cells (tests/_h1_ref.py lists the by-design rounding points),
  3. asserts on the reference alone that the contribution at risk (last row / column / tap / channel cell, the residual) moves the
     reference by more than 100 times the bound -- a passing comparison cannot be an insensitive one.
Bounds (none tuned to the code under test):
  fp32 results   max |got - ref| / max |ref| < 1e-5            (REL_TOL of test_backward_layers_gpu.py: fp32 accumulation)
  H1 results     |got - ref| <= 2^-11 |ref| + 2^-25 + 1e-5 max |ref| per element in scaled units (half an fp16 ulp, normal or subnormal,
                 plus the accumulation bound); exactly zero wherever the gate's half is not positive.
Measured on the MI355X (worst case of each group; every test prints its figure before it asserts):
  wgrad_h1 dw / colsum             1.9e-7  (bound 1e-5); subnormal operands 1.8e-7; the three failed-prediction ratios raise flag bit 2
  dgrad_h1 |err| / bound           0.96    (bound 1: the rounding of the output cell itself uses the half ulp)
  h1_to_f32_pred, plain and gated  exact
  stem_wgrad_h1 dw / colsum        1.3e-7  (bound 1e-5)
  heads dw / db                    1.7e-7  (bound 1e-5); d features |err| / bound 0.96
No kernel or launcher fault was found: every case passed on the first run of the code under test.
That the comparisons bite was checked once against a build with four faults that change values only: the last 8 output channels dropped
from wgrad_dma_h1's partly filled 64-column tile, the coarse-grid residual read with its scale exponent one off, a pool window of the
last band routed to the neighbouring conv1 pixel, the locref head finalised from a column one off.  The 64-column weight-gradient cases,
the add_mode -2 data-gradient cases, the stem cases and every heads case failed; the other 28 cases passed.
"""
import numpy as np
import pytest
import torch

import _h1_ref as R

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
SENSITIVE = 100.0


def _seed(case):
    return hash(tuple(case)) % (2 ** 31)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_cells(cells, x, s, what):
    """The H1 tensor the entry point made is h1(x, s), bit for bit."""
    exp = R.h1(x, s)
    bad = int((_bits(cells) != _bits(exp)).sum())
    assert bad == 0, "%s: %d of %d cells differ from float16(x * %g)" % (what, bad, exp.numel(), s)


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _h1_excess(cells, ref_scaled):
    """Worst |got - ref| / bound of an H1 result (scaled units) and the bound's largest value."""
    bound = 2.0 ** -11 * ref_scaled.abs() + 2.0 ** -25 + REL_TOL * ref_scaled.abs().max()
    return float(((cells.double() - ref_scaled).abs() / bound).max()), float(bound.max())


def _wgrad_inputs(case):
    N, H, W, Cin, Cout, k, stride, rate = case
    g = torch.Generator(device="cuda").manual_seed(_seed(case))
    pad_t, Ho = R.same_pads(H, k, stride, rate)
    pad_l, Wo = R.same_pads(W, k, stride, rate)
    x = torch.relu(torch.randn((N, H, W, Cin), generator=g, device="cuda"))           # post-ReLU activations
    dy = torch.randn((N, Ho, Wo, Cout), generator=g, device="cuda") * 1e-3
    dy[torch.rand((N, Ho, Wo, Cout), generator=g, device="cuda") < 0.4] = 0.0           # gated gradient
    return x, dy, pad_t, pad_l


# (N, H, W, Cin, Cout, k, stride, rate)
_RAGGED = (3, 13, 17, 64, 136, 3, 1, 1)          # ragged everything, Cout % 128 != 0
_DEEP = (2, 30, 40, 1024, 256, 1, 1, 1)          # M = 2400 over ten pixel slices, the last one ragged, deep K
H1_WGRAD_CASES = [
    _RAGGED,
    (2, 9, 11, 32, 128, 3, 2, 1),                # the last k-tile is part empty
    (3, 10, 13, 128, 128, 3, 2, 1),              # stride 2, odd grid
    (3, 5, 9, 128, 128, 3, 2, 1),                # stride 2, odd on both axes
    (3, 5, 7, 512, 512, 3, 1, 2),                # dilated, most taps in the padding
    (3, 19, 26, 256, 64, 1, 1, 1),               # 64-column partly filled tile (H1 only)
    (3, 19, 26, 64, 64, 3, 1, 1),                # 64-column partly filled tile (H1 only)
    (3, 19, 26, 64, 256, 1, 1, 1),               # block1 conv3 (Cout 256)
    (1, 3, 5, 128, 128, 1, 1, 1),                # M = 15: less than one 16-pixel step
    _DEEP,
]
_DMA_RATIOS = [(1.0, 1.0), (0.4, 3.0), (2.0 ** -6, 1.0), (1.0, 2.0 ** 8), (0.0, 1.0)]
_WORST = {}


def _note(group, value):
    _WORST[group] = max(_WORST.get(group, 0.0), value)
    print("measured %s: %.3g (worst so far %.3g)" % (group, value, _WORST[group]))


def _check_wgrad(case, x, dy, pad_t, pad_l, ratio, group):
    from deepgraphpose_amd import engine
    N, H, W, Cin, Cout, k, stride, rate = case
    mx, my = float(x.abs().max()), float(dy.abs().max())
    px, py = mx * ratio[0], my * ratio[1]
    sx, sy = R.pred_scale(px), R.pred_scale(py)
    dw, cs, xc, dyc, flag = engine.conv2d_wgrad_h1(x, dy, k, stride, rate, pad_t, pad_l, prev_max=(px, py))
    if not (R.usable(sx, mx) and R.usable(sy, my)):
        # a tensor left the window its predicted scale covers: the kernel has no fp32 path to fall back to (the parity tier's wgrad_dma
        # has); it raises the failure flag, writes nothing, and the trainer repeats the step on the parity path
        assert flag & 2, (case, ratio, flag)
        assert float(dw.abs().max()) == 0.0 and float(cs.abs().max()) == 0.0
        return
    assert flag == 0, (case, ratio, flag)
    _same_cells(xc, x, sx, "x")
    _same_cells(dyc, dy, sy, "dy")
    xq, dyq = xc.double() / sx, dyc.double() / sy
    ref, cref = R.wgrad(xq, dyq, k, stride, rate, pad_t, pad_l)
    # edge conditions on the reference alone: what the last output row / column, the last tap and the last 8-channel cells contribute
    top = float(ref.abs().max())
    last_row, last_col = torch.zeros_like(dyq), torch.zeros_like(dyq)
    last_row[:, -1], last_col[:, :, -1] = dyq[:, -1], dyq[:, :, -1]
    for what, part in (("last output row", R.wgrad(xq, last_row, k, stride, rate, pad_t, pad_l)[0]),
                       ("last output column", R.wgrad(xq, last_col, k, stride, rate, pad_t, pad_l)[0]),
                       ("last tap", ref[k - 1, k - 1]), ("last 8 input channels", ref[:, :, -8:]), ("last 8 output channels", ref[..., -8:])):
        assert float(part.abs().max()) > SENSITIVE * REL_TOL * top, (case, what)
    err, cerr = _rel(dw, ref), float((cs.double() - cref).abs().max() / cref.abs().max())
    _note(group, max(err, cerr))
    assert err < REL_TOL, (case, ratio, err)
    assert cerr < REL_TOL, (case, ratio, cerr)


@pytest.mark.parametrize("case,ratio", [(c, r) for c in H1_WGRAD_CASES for r in _DMA_RATIOS if r == (1.0, 1.0) or c in (_RAGGED, _DEEP)])
def test_wgrad_h1_matches_float64_on_the_same_cells(lib_built, case, ratio):
    """ratio = (previous / current maximum) of (x, dy): inside the usable window the kernel must match, outside it -- or with no previous
    range -- it must raise flag bit 2."""
    x, dy, pad_t, pad_l = _wgrad_inputs(case)
    _check_wgrad(case, x, dy, pad_t, pad_l, ratio, "wgrad_h1")


def test_wgrad_h1_subnormal_operands_keep_their_bits(lib_built):
    """One outlier sets each scale and the bulk lies 2^-22 .. 2^-26 below it (40 % exact zeros, as a ReLU / a gate leaves them): in scaled
    units the bulk is 2^-11.5 .. 2^-15.5 -- the lower half fp16 subnormals with 1 .. 9 significant bits.  The outlier's row / column of dW is
    outlier x bulk: it vanishes if the matrix pipe flushes subnormals."""
    case = (3, 19, 26, 64, 64, 3, 1, 1)
    N, H, W, Cin, Cout, k, stride, rate = case
    g = torch.Generator(device="cuda").manual_seed(5)
    u = lambda C: torch.rand((N, H, W, C), generator=g, device="cuda")
    x = 1.5 * torch.exp2(-(22.0 + 4.0 * u(Cin))) * (u(Cin) < 0.6)
    x[1, 7, 9, 3] = 1.5
    dy = 1.25 * torch.exp2(-(22.0 + 4.0 * u(Cout))) * torch.sign(u(Cout) - 0.5) * (u(Cout) < 0.6)
    dy[2, 11, 5, 6] = -1.25
    from deepgraphpose_amd import engine
    sx, sy = R.pred_scale(1.5), R.pred_scale(1.25)
    dw, cs, xc, dyc, flag = engine.conv2d_wgrad_h1(x, dy, k, stride, rate, 1, 1)
    assert flag == 0
    _same_cells(xc, x, sx, "x")
    _same_cells(dyc, dy, sy, "dy")
    sub = lambda c: (c != 0) & (c.abs() < 2.0 ** -14)
    for c in (xc, dyc):
        assert float(sub(c).float().mean()) > 0.15 and float((c == 0).float().mean()) > 0.3
    xq, dyq = xc.double() / sx, dyc.double() / sy
    ref, cref = R.wgrad(xq, dyq, k, stride, rate, 1, 1)
    flushed, _ = R.wgrad(torch.where(sub(xc), torch.zeros_like(xq), xq), torch.where(sub(dyc), torch.zeros_like(dyq), dyq), k, stride, rate, 1, 1)
    assert float((flushed - ref).abs().max()) > SENSITIVE * REL_TOL * float(ref.abs().max())
    err = _rel(dw, ref)
    _note("wgrad_h1 subnormal", err)
    assert err < REL_TOL, err
    assert float((cs.double() - cref).abs().max() / cref.abs().max()) < REL_TOL


# ---------------------------------------------------------------------------------------------------------------
# N, H, W, Cin, Cout, k, stride, rate, add_mode (0 none, 1 same grid, -2 coarser grid), gate
H1_DGRAD_CASES = [
    (3, 5, 7, 512, 2048, 1, 1, 1, 0, True),          # conv3
    (3, 5, 7, 512, 512, 3, 1, 2, 0, True),           # dilated conv2
    (3, 19, 26, 64, 64, 3, 2, 1, 0, True),           # zero-stuff, odd rows
    (3, 10, 13, 128, 128, 3, 2, 1, 0, True),         # zero-stuff, odd columns
    (3, 5, 9, 128, 128, 3, 2, 1, 0, True),           # zero-stuff, odd on both axes
    (3, 19, 26, 256, 64, 1, 1, 1, -2, True),         # coarse-grid H1 residual
    (3, 5, 9, 512, 128, 1, 1, 1, -2, True),          # coarse-grid H1 residual
    (3, 10, 13, 512, 128, 1, 1, 1, 1, True),         # same-grid H1 residual
    (3, 19, 26, 64, 256, 1, 1, 1, 0, False),         # no gate: the shortcut conv's form
    (3, 7, 9, 128, 128, 3, 1, 1, 0, True),           # frames smaller than a tile
]
# a residual whose range differs from dy's by 2^6: a swapped or missing residual scale cannot cancel
H1_DGRAD_RUNS = [(c, 1.0) for c in H1_DGRAD_CASES] + [((3, 19, 26, 256, 64, 1, 1, 1, -2, True), 64.0), ((3, 10, 13, 512, 128, 1, 1, 1, 1, True), 64.0)]


@pytest.mark.parametrize("case,add_gain", H1_DGRAD_RUNS)
def test_dgrad_h1_matches_float64_on_the_same_cells(lib_built, case, add_gain):
    from deepgraphpose_amd import engine
    N, H, W, Cin, Cout, k, stride, rate, add_mode, gated = case
    g = torch.Generator(device="cuda").manual_seed(_seed(case))
    pad_t, Ho = R.same_pads(H, k, stride, rate)
    pad_l, Wo = R.same_pads(W, k, stride, rate)
    dy = torch.randn((N, Ho, Wo, Cout), generator=g, device="cuda") * 1e-3
    dy[torch.rand((N, Ho, Wo, Cout), generator=g, device="cuda") < 0.4] = 0.0
    w = torch.randn((k, k, Cin, Cout), generator=g, device="cuda") / float(np.sqrt(k * k * Cin))
    scale = 1.0 + 0.1 * torch.randn(Cout, generator=g, device="cuda")
    mask = torch.relu(torch.randn((N, H, W, Cin), generator=g, device="cuda"))
    add = None
    if add_mode == 1:
        add = torch.randn((N, H, W, Cin), generator=g, device="cuda") * (1e-3 * add_gain)
    elif add_mode == -2:
        add = torch.randn((N, (H + 1) // 2, (W + 1) // 2, Cin), generator=g, device="cuda") * (1e-3 * add_gain)
    # the gate as the forward pass left it: an H1 tensor with a scale of its own (only its sign is read)
    gate_cells = engine.f32_to_h1(mask, 7) if gated else None
    dy_prev = float(dy.abs().max())
    add_prev = float(add.abs().max()) if add is not None else 0.0
    s_dy, s_add = R.pred_scale(dy_prev), R.pred_scale(add_prev)
    # float64 on the operands as the cells hold them (the cells themselves are asserted below)
    dyq = R.h1_values(dy, s_dy)
    wq = R.panel_values(w, scale)
    addq = R.h1_values(add, s_add) if add is not None else None
    conv = R.dgrad(dyq, wq, H, W, stride, rate, pad_t, pad_l)
    ref = R.gate(R.add_residual(conv, addq, add_mode), gate_cells)
    dx_prev = float(ref.abs().max())                  # "last step" had the same range
    s_dx = R.pred_scale(dx_prev)
    out = engine.conv2d_dgrad_h1(dy, w, (H, W), stride, rate, pad_t, pad_l, scale=scale, gate_h1=gate_cells, dx_add=add,
                                 add_mode=add_mode if add is not None else 1, dy_prev=dy_prev, dx_prev=dx_prev, add_prev=add_prev)
    assert out["flag"] == 0, out["flag"]
    _same_cells(out["dy"], dy, s_dy, "dy")
    if add is not None:
        _same_cells(out["add"], add, s_add, "dx_add")
    if stride == 2:
        assert torch.equal(_bits(out["stuffed"]), _bits(R.zero_stuff(out["dy"]))), "zero-stuffed copy"
        assert torch.allclose(R.dgrad_stuffed(dyq, wq, H, W, rate, pad_t, pad_l), conv, rtol=0, atol=1e-12 * float(conv.abs().max()))
    ref_s = ref * s_dx
    excess, bound = _h1_excess(out["dx"], ref_s)
    # edge conditions on the reference alone, after the gate, in scaled units
    part_row, part_col = torch.zeros_like(dyq), torch.zeros_like(dyq)
    part_row[:, -1], part_col[:, :, -1] = dyq[:, -1], dyq[:, :, -1]
    parts = [("last row of dy", R.dgrad(part_row, wq, H, W, stride, rate, pad_t, pad_l)),
             ("last column of dy", R.dgrad(part_col, wq, H, W, stride, rate, pad_t, pad_l))]
    if k > 1:
        wl = torch.zeros_like(wq)
        wl[k - 1, k - 1] = wq[k - 1, k - 1]
        parts.append(("last tap", R.dgrad(dyq, wl, H, W, stride, rate, pad_t, pad_l)))
    if add_gain != 1.0:
        parts = []                # (a residual 2^6 above the conv's part sets the range: these runs are about the residual's scale alone)
    if add is not None:
        parts.append(("residual", R.add_residual(torch.zeros_like(conv), addq, add_mode)))
    for what, part in parts:
        assert float(R.gate(part, gate_cells).abs().max()) * s_dx > SENSITIVE * bound, (case, what)
    _note("dgrad_h1 (|err| / bound)", excess)
    assert excess <= 1.0, (case, add_gain, excess)
    if gated:
        closed = ~(gate_cells > 0)
        assert int(closed.sum()) > 0 and float(out["dx"][closed].abs().max()) == 0.0
    # the converter that takes a gradient out of the H1 units: exact
    assert torch.equal(out["dx_f32"], out["dx"].float() / float(s_dx))


def test_h1_to_f32_pred_gated_form_is_exact(lib_built):
    """h1_to_f32_pred_kernel with a gate tensor: value / predicted scale where the gate's half is positive, +0 elsewhere (-0 and NaN gates
    are closed); the ungated form keeps every bit, subnormals and -0 included."""
    from deepgraphpose_amd import engine
    g = torch.Generator(device="cuda").manual_seed(11)
    cells = (torch.randn((3, 7, 9, 64), generator=g, device="cuda") * 300.0).to(torch.float16)
    cells[0, 0, 0, :4] = torch.tensor([2.0 ** -24, -2.0 ** -24, -0.0, 65504.0], dtype=torch.float16, device="cuda")
    gate = torch.randn((3, 7, 9, 64), generator=g, device="cuda").to(torch.float16)
    gate[0, 0, 0, :4] = torch.tensor([2.0 ** -24, -0.0, 0.0, float("nan")], dtype=torch.float16, device="cuda")
    for prev in (3.7e-4, 1.0, 900.0):
        s = R.pred_scale(prev)
        exp = cells.float() / float(s)
        assert torch.equal(engine.h1_to_f32_pred(cells, prev).view(torch.int32), exp.view(torch.int32))
        got = engine.h1_to_f32_pred(cells, prev, gate_h1=gate)
        assert torch.equal(got.view(torch.int32), torch.where(gate > 0, exp, torch.zeros_like(exp)).view(torch.int32))
    assert float(engine.h1_to_f32_pred(cells, 0.0).abs().max()) == 0.0          # no previous range: no scale, zeros


# ---------------------------------------------------------------------------------------------------------------
# frames (H, W) whose conv1 maps are 17 x 33 (pool padding starts at 1 on both axes; last band one row, last chunk one column),
# 32 x 48 (padding starts at 0; one and a half chunks), 51 x 45, 38 x 51 (padding 0 on rows, 1 on columns)
STEM_FRAMES = [(33, 65), (64, 96), (102, 89), (75, 101)]


def _hand_record(kind, B, H1, W1, dev):
    """shared: every window names the pixel it shares with its neighbours (window pairs (2m, 2m + 1): the odd one's origin), so one conv1
    pixel collects four windows; corner: every window names its own top-left valid pixel."""
    HP, pt = R.pool_geometry(H1)
    WP, pl = R.pool_geometry(W1)
    qy, qx = torch.arange(HP, device=dev), torch.arange(WP, device=dev)
    if kind == "shared":
        # (an unpaired last window names the pixel it shares with the window before it)
        a = torch.where((qy % 2 == 1) | (qy == HP - 1), 0, 2)
        b = torch.where((qx % 2 == 1) | (qx == WP - 1), 0, 2)
    else:
        a, b = torch.clamp(pt - 2 * qy, min=0), torch.clamp(pl - 2 * qx, min=0)
    rec = (a[:, None] * 3 + b[None, :]).to(torch.uint8)
    return rec[None, :, :, None].expand(B, HP, WP, 64).contiguous()


@pytest.mark.parametrize("record", ["first maximum", "shared", "corner"])
@pytest.mark.parametrize("frame", STEM_FRAMES)
def test_stem_wgrad_h1_matches_float64_on_the_same_cells(lib_built, frame, record):
    from deepgraphpose_amd import engine
    B, (H, W) = 2, frame
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    HP, WP = R.pool_geometry(H1)[0], R.pool_geometry(W1)[0]
    assert (H1, W1) in ((17, 33), (32, 48), (51, 45), (38, 51))
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + W)
    x = torch.zeros((B, H, W, 4), device="cuda")
    x[..., :3] = torch.randint(0, 256, (B, H, W, 3), generator=g, device="cuda").float() - torch.tensor([123.68, 116.779, 103.939], device="cuda")
    if record == "first maximum":
        rec = R.pool_first_max(torch.randn((B, H1, W1, 64), generator=g, device="cuda"))[1]
    else:
        rec = _hand_record(record, B, H1, W1, "cuda")
    dpool = torch.randn((B, HP, WP, 64), generator=g, device="cuda") * 1e-3
    dpool[torch.rand((B, HP, WP, 64), generator=g, device="cuda") < 0.3] = 0.0
    prev = float(dpool.abs().max())
    s = R.pred_scale(prev)
    dw, cs, cells = engine.stem_wgrad_h1(x, dpool, rec, prev)
    _same_cells(cells, dpool, s, "dpool")
    ref, cref, dc1 = R.stem_wgrad(x, cells, rec, s)
    if record == "shared":
        four = R.pool_backward(torch.ones_like(dpool), rec, H1, W1)
        assert float(four.max()) == 4.0                                           # four windows meet in one pixel
    top = float(ref[:, :, :3].abs().max())
    # (the last conv1 row / column that holds a gradient: a hand-made record leaves some rows and columns empty)
    r = int(torch.nonzero(dc1.abs().amax((0, 2, 3)) > 0)[-1])
    c = int(torch.nonzero(dc1.abs().amax((0, 1, 3)) > 0)[-1])
    assert r >= H1 - 2 and c >= W1 - 2 and (record != "first maximum" or (r, c) == (H1 - 1, W1 - 1))
    last_row, last_col = torch.zeros_like(dc1), torch.zeros_like(dc1)
    last_row[:, r], last_col[:, :, c] = dc1[:, r], dc1[:, :, c]
    xh = x.to(torch.float16).double()
    for what, part in (("last conv1 row",R.wgrad(xh, last_row, 7, 2, 1, 3, 3)[0] / s), ("last conv1 column", R.wgrad(xh, last_col, 7, 2, 1, 3, 3)[0] / s),
                       ("last tap", ref[6, 6])):
        assert float(part[..., :3, :].abs().max()) > SENSITIVE * REL_TOL * top, (frame, record, what)
    err = _rel(dw[:, :, :3], ref[:, :, :3])
    cerr = float((cs.double() - cref).abs().max() / cref.abs().max())
    _note("stem_wgrad_h1", max(err, cerr))
    assert err < REL_TOL, (frame, record, err)
    assert cerr < REL_TOL, (frame, record, cerr)
    assert float(dw[:, :, 3].abs().max()) == 0.0          # the padded fourth input channel


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [1, 2, 3, 5])
@pytest.mark.parametrize("fmap", [(2, 2, 2), (3, 5, 7), (3, 3, 5)])
def test_heads_backward_h1_matches_float64_on_the_same_cells(lib_built, fmap, nj):
    """Both heads through the merged H1 tensor.  The locref gradient is 2^-8 of the scoremap gradient, as in training, and shares its scale."""
    from deepgraphpose_amd import engine
    N, h, w = fmap
    Cin = 2048
    g = torch.Generator(device="cuda").manual_seed(_seed(fmap + (nj,)))
    feat = torch.relu(torch.randn((N, h, w, Cin), generator=g, device="cuda"))
    dsc = torch.randn((N, 2 * h, 2 * w, nj), generator=g, device="cuda") * 1e-3
    dloc = torch.randn((N, 2 * h, 2 * w, 2 * nj), generator=g, device="cuda") * (1e-3 * 2.0 ** -8)
    w0 = torch.randn((3, 3, nj, Cin), generator=g, device="cuda") * 0.05
    w1 = torch.randn((3, 3, 2 * nj, Cin), generator=g, device="cuda") * 0.05
    c0, c1, CT = R.heads_layout(nj)
    feat_prev, dph_prev = float(feat.abs().max()), float(max(dsc.abs().max(), dloc.abs().max()))
    sf, sg = R.pred_scale(feat_prev), R.pred_scale(dph_prev)
    merged = R.heads_gather(dsc, dloc)
    Gq = R.h1_values(merged, sg)
    featq = R.h1_values(feat, sf)
    sw = R.panel_scale(float(max(w0.abs().max(), w1.abs().max())))          # ONE panel holds both heads: one scale
    dq = R.heads_scatter(Gq, nj)
    wq = [R.h1_values(w0, sw), R.h1_values(w1, sw)]
    refs = [R.head_backward(featq, dq[0], wq[0]), R.head_backward(featq, dq[1], wq[1])]
    dfeat_ref = R.gate(refs[0][2] + refs[1][2], featq)
    dfeat_prev = float(dfeat_ref.abs().max())
    s_out = R.pred_scale(dfeat_prev)
    out = engine.heads_backward_h1(feat, dsc, dloc, w0, w1, CT, feat_prev, dph_prev, dfeat_prev)
    assert out["flag"] == 0, out["flag"]
    _same_cells(out["feat"], feat, sf, "features")
    _same_cells(out["merged"], merged, sg, "merged gradient")
    pad = torch.ones(CT, dtype=torch.bool, device="cuda")
    pad[:4 * nj] = False
    pad[c0:c0 + 8 * nj] = False
    assert int(pad.sum()) == CT - 12 * nj and float(out["merged"][..., pad].abs().max()) == 0.0      # the padding columns hold nothing
    worst = 0.0
    fl, fc = torch.zeros_like(featq), torch.zeros_like(featq)
    fl[:, -1], fc[:, :, -1] = featq[:, -1], featq[:, :, -1]
    for k, name in enumerate(("part", "locref")):
        dw, db, _ = refs[k]
        top = float(dw.abs().max())
        # at risk: the feature map's last row / column (taps 0 and 1 read them), the last tap, the head's last column
        for what, part in (("last feature row", R.head_backward(fl, dq[k], wq[k])[0]), ("last feature column", R.head_backward(fc, dq[k], wq[k])[0]),
                           ("last tap", dw[2, 2]), ("last joint", dw[:, :, -1])):
            assert float(part.abs().max()) > SENSITIVE * REL_TOL * top, (fmap, nj, name, what)
        e_w, e_b = _rel(out["dw_" + name], dw), _rel(out["db_" + name], db)
        worst = max(worst, e_w, e_b)
        assert e_w < REL_TOL, (fmap, nj, name, "dw", e_w)
        assert e_b < REL_TOL, (fmap, nj, name, "db", e_b)
    _note("heads_backward_h1 dw / db", worst)
    ref_s = dfeat_ref * s_out
    excess, bound = _h1_excess(out["dfeat"], ref_s)
    wl = torch.zeros_like(wq[0])
    wl[2, 2] = wq[0][2, 2]
    last_tap = R.gate(R.head_backward(featq, dq[0], wl)[2], featq)
    assert float(last_tap.abs().max()) * s_out > SENSITIVE * bound, (fmap, nj, "last tap of d features")
    _note("heads_backward_h1 dfeat (|err| / bound)", excess)
    assert excess <= 1.0, (fmap, nj, excess)
    closed = ~(out["feat"] > 0)
    assert float(out["dfeat"][closed].abs().max()) == 0.0
