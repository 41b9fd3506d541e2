"""tests/_h1_ref.py -- the float64 reference the 16-bit tier's backward kernels are compared with (test_backward_layers_h1_gpu.py) --
checked on its own against closed forms and float64 torch autograd.  No GPU, no project code."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _h1_ref as R


def test_predicted_scale_known_values():
    assert R.pred_scale(1.0) == 1024.0                      # 1.0 = 1.0 x 2^0 -> [2^10, 2^11)
    assert R.pred_scale(1.999) == 1024.0
    assert R.pred_scale(2.0) == 512.0
    assert R.pred_scale(65504.0) == 2.0 ** -5               # 65504 = 1.999 x 2^15
    assert R.pred_scale(1e-30) == 2.0 ** 110                # 1e-30 = 1.27 x 2^-100
    assert R.pred_scale(0.0) == 0.0
    assert R.pred_scale(float("inf")) == 0.0
    assert R.pred_scale(float("nan")) == 0.0
    assert R.pred_scale(1e-40) == 0.0                       # a subnormal maximum: no scale
    for m in (1.0, 1.999, 2.0, 65504.0, 1e-30, 3.7e-4):
        assert 1024.0 <= np.float32(m) * R.pred_scale(m) < 2048.0


def test_usable_window():
    s = R.pred_scale(1.0)
    assert R.usable(s, 1.0) and R.usable(s, 16.0 / 1024.0) and R.usable(s, 63.4)
    assert not R.usable(s, 15.99 / 1024.0)                  # below 16 after scaling
    assert not R.usable(s, 65000.0 / 1024.0)                # [16, 65000)
    assert not R.usable(0.0, 1.0) and not R.usable(s, float("nan"))
    # the ratios of the weight-gradient test: previous / current maximum
    assert R.usable(R.pred_scale(0.4), 1.0) and R.usable(R.pred_scale(3.0), 1.0)
    assert not R.usable(R.pred_scale(2.0 ** -6), 1.0) and not R.usable(R.pred_scale(2.0 ** 8), 1.0)


def test_h1_rounds_once_to_nearest_even_with_subnormals():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 70000.0])
    got = R.h1(x, 1.0)
    exp = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -9, -0.0, 0.0, 2.0 ** -23, 2.0 ** -14, float("inf")], dtype=torch.float16)
    assert torch.equal(got.view(torch.int16), exp.view(torch.int16))
    assert torch.equal(R.h1(x[:3] / 512.0, 512.0), exp[:3])                 # a power-of-two scale moves no rounding boundary
    assert R.panel_scale(1.0) == 2.0 ** 14 and R.panel_scale(0.0) == 1.0 and R.panel_scale(0.3) == 2.0 ** 16


# ---- pool -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(17, 33), (32, 48), (51, 45), (38, 51)])
def test_pool_record_and_backward_match_autograd(hw):
    H1, W1 = hw
    g = torch.Generator().manual_seed(H1 * 100 + W1)
    c1 = torch.randn((2, H1, W1, 5), generator=g, dtype=torch.float64)          # continuous values: no ties
    HP, pt = R.pool_geometry(H1)
    WP, pl = R.pool_geometry(W1)
    assert (pt, pl) == {(17, 33): (1, 1), (32, 48): (0, 0), (51, 45): (1, 1), (38, 51): (0, 1)}[hw]
    x = c1.permute(0, 3, 1, 2).clone().requires_grad_(True)
    xp = F.pad(x, (pl, 2 * WP + 1 - W1 - pl, pt, 2 * HP + 1 - H1 - pt), value=-float("inf"))
    y = F.max_pool2d(xp, 3, 2)[:, :, :HP, :WP]
    pool, rec = R.pool_first_max(c1)
    assert torch.equal(pool, y.detach().permute(0, 2, 3, 1))
    dpool = torch.randn((2, HP, WP, 5), generator=g, dtype=torch.float64)
    y.backward(dpool.permute(0, 3, 1, 2))
    got = R.pool_backward(dpool, rec, H1, W1)
    assert torch.allclose(got, x.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-14)
    assert int(rec.max()) <= 8


def test_pool_ties_go_to_the_first_maximum():
    c1 = torch.zeros((1, 5, 5, 1), dtype=torch.float64)                         # all equal: every window's first VALID position wins
    pool, rec = R.pool_first_max(c1)                                            # 5 -> 3 windows, padding starts at 1
    assert rec[0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]
    c1[0, 1, 1, 0] = 1.0                                                        # windows start at rows / columns -1, 1, 3: pixel (1, 1) lies in four
    c1[0, 1, 2, 0] = 1.0                                                        # an equal value right of it: windows (., 1) hold both, the earlier wins
    _, rec = R.pool_first_max(c1)
    assert rec[0, :2, :2, 0].tolist() == [[2 * 3 + 2, 2 * 3 + 0], [0 * 3 + 2, 0 * 3 + 0]]
    d = R.pool_backward(torch.ones((1, 3, 3, 1), dtype=torch.float64), rec, 5, 5)
    assert float(d.sum()) == 9.0 and float(d[0, 1, 1, 0]) == 4.0 and float(d[0, 1, 2, 0]) == 0.0


# ---- data gradient ----------------------------------------------------------------------------------------------------------------
def _conv_fwd(x, w, stride, rate, pad_t, pad_l, Ho, Wo):
    keff = (w.shape[0] - 1) * rate + 1
    xp = F.pad(x.permute(0, 3, 1, 2), (pad_l, max(0, (Wo - 1) * stride + keff - x.shape[2] - pad_l), pad_t,
                                       max(0, (Ho - 1) * stride + keff - x.shape[1] - pad_t)))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=stride, dilation=rate)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", [(2, 9, 11, 8, 16, 3, 2, 1), (2, 10, 13, 8, 8, 3, 2, 1), (1, 5, 7, 8, 8, 3, 1, 2), (2, 5, 9, 16, 8, 1, 1, 1),
                                  (2, 6, 8, 8, 8, 3, 2, 1)])
def test_dgrad_wgrad_zero_stuff_residual_and_gate_match_autograd(case):
    N, H, W, Cin, Cout, k, stride, rate = case
    g = torch.Generator().manual_seed(sum(case))
    pad_t, Ho = R.same_pads(H, k, stride, rate)
    pad_l, Wo = R.same_pads(W, k, stride, rate)
    x = torch.randn((N, H, W, Cin), generator=g, dtype=torch.float64)
    w = torch.randn((k, k, Cin, Cout), generator=g, dtype=torch.float64, requires_grad=True)
    add = torch.randn((N, (H + 1) // 2, (W + 1) // 2, Cin), generator=g, dtype=torch.float64)
    dy = torch.randn((N, Ho, Wo, Cout), generator=g, dtype=torch.float64)
    # z = relu(x); loss = <conv(z), dy> + <z[::2, ::2], add>: d loss / dx = gate(convT(dy) + add on the coarse grid)
    xr = x.clone().requires_grad_(True)
    z = torch.relu(xr)
    loss = (_conv_fwd(z, w, stride, rate, pad_t, pad_l, Ho, Wo) * dy).sum() + (z[:, ::2, ::2] * add).sum()
    loss.backward()
    wd = w.detach()
    dx = R.dgrad(dy, wd, H, W, stride, rate, pad_t, pad_l)
    got = R.gate(R.add_residual(dx, add, -2), x)
    assert torch.allclose(got, xr.grad, rtol=0, atol=1e-12)
    assert float((got == 0).double().mean()) > 0.3
    if stride == 2:
        assert torch.allclose(R.dgrad_stuffed(dy, wd, H, W, rate, pad_t, pad_l), dx, rtol=0, atol=1e-12)
        z2 = R.zero_stuff(dy)
        assert z2.shape == (N, 2 * Ho, 2 * Wo, Cout) and torch.equal(z2[:, ::2, ::2], dy) and float(z2.abs().sum()) == float(dy.abs().sum())
    dw, cs = R.wgrad(torch.relu(x), dy, k, stride, rate, pad_t, pad_l)
    assert torch.allclose(dw, w.grad, rtol=0, atol=1e-12) and torch.allclose(cs, dy.sum((0, 1, 2)))
    same = torch.randn(dx.shape, generator=g, dtype=torch.float64)
    assert torch.equal(R.add_residual(dx, same, 1), dx + same)


# ---- heads ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [1, 2, 3, 5])
def test_heads_gather_layout_and_backward_match_autograd(nj):
    N, h, w, Cin = 2, 3, 5, 8
    g = torch.Generator().manual_seed(nj)
    feat = torch.randn((N, h, w, Cin), generator=g, dtype=torch.float64, requires_grad=True)
    c0, c1, CT = R.heads_layout(nj)
    assert (c0, c1, CT) == {1: (4, 8, 64), 2: (8, 16, 64), 3: (16, 32, 64), 5: (32, 64, 128)}[nj]
    douts = [torch.randn((N, 2 * h, 2 * w, njt), generator=g, dtype=torch.float64) for njt in (nj, 2 * nj)]
    G = R.heads_gather(*douts)
    assert G.shape == (N, h, w, CT)
    used = torch.zeros(CT, dtype=torch.bool)
    used[:4 * nj] = True
    used[c0:c0 + 8 * nj] = True
    assert float(G[..., ~used].abs().sum()) == 0.0 and float(G[..., used].abs().min()) > 0.0
    assert float(G[1, 2, 4, 3 * nj + nj - 1]) == float(douts[0][1, 5, 9, nj - 1])              # phase 3 = (odd row, odd column)
    assert float(G[0, 1, 0, c0 + 2 * (2 * nj)]) == float(douts[1][0, 3, 0, 0])                 # phase 2 = (odd row, even column)
    back = R.heads_scatter(G, nj)
    assert torch.equal(back[0], douts[0]) and torch.equal(back[1], douts[1])
    dfeat = torch.zeros((N, h, w, Cin), dtype=torch.float64)
    loss = 0.0
    ws = []
    for dout in douts:
        njt = dout.shape[3]
        wt = torch.randn((3, 3, njt, Cin), generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(njt, dtype=torch.float64, requires_grad=True)
        # conv2d_transpose SAME, 3x3 / stride 2: out = 2 h, total padding (h - 1) 2 + 3 - 2 h = 1, pad_before 0
        full = F.conv_transpose2d(feat.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), stride=2)
        out = full[:, :, :2 * h, :2 * w] + b[None, :, None, None]
        loss = loss + (out.permute(0, 2, 3, 1) * dout).sum()
        ws.append((wt, b))
    loss.backward()
    for dout, (wt, b) in zip(douts, ws):
        dw, db, df = R.head_backward(feat.detach(), dout, wt.detach())
        assert torch.allclose(dw, wt.grad, rtol=0, atol=1e-12) and torch.allclose(db, b.grad, rtol=0, atol=1e-12)
        dfeat += df
    assert torch.allclose(dfeat, feat.grad, rtol=0, atol=1e-12)


def test_stem_reference_rounds_the_patch_and_dc1_only():
    """On values fp16 holds exactly the stem reference IS the float64 chain pool-backward -> weight gradient."""
    g = torch.Generator().manual_seed(7)
    B, H, W = 1, 13, 17
    H1, W1 = 7, 9
    x = torch.randint(-128, 128, (B, H, W, 4), generator=g).float()
    x[..., 3] = 0
    c1 = torch.randn((B, H1, W1, 64), generator=g, dtype=torch.float64)
    _, rec = R.pool_first_max(c1)
    HP, WP = R.pool_geometry(H1)[0], R.pool_geometry(W1)[0]
    cells = torch.randint(-512, 512, (B, HP, WP, 64), generator=g).to(torch.float16)
    dw, cs, dc1 = R.stem_wgrad(x, cells, rec, 4.0)
    d64 = R.pool_backward(cells.double(), rec, H1, W1)
    assert torch.equal(dc1, d64)
    dwr, csr = R.wgrad(x.double(), d64, 7, 2, 1, 3, 3)
    assert torch.equal(dw, dwr / 4.0) and torch.equal(cs, csr / 4.0)
    assert dw.shape == (7, 7, 4, 64) and float(dw[:, :, 3].abs().sum()) == 0.0


def test_pool_first_valid_rule_matches_plain_loops():
    """pool_first_max(first_valid=True): the first position inside the map is taken whatever it holds (a window of -inf records it, not 0);
    afterwards only strictly greater values.  Against loops written from that sentence, on a padded and an unpadded grid."""
    g = torch.Generator().manual_seed(5)
    for H1, W1 in ((5, 7), (6, 4)):
        x = torch.round(torch.randn((1, H1, W1, 3), generator=g) * 2) / 2                  # coarse values: ties
        x[torch.rand(x.shape, generator=g) < 0.3] = -float("inf")
        x[:, :3, :3] = -float("inf")                                                       # whole windows of -inf
        x[0, -1, -1, 0] = -0.0
        pool, rec = R.pool_first_max(x, first_valid=True)
        (HP, pt), (WP, pl) = R.pool_geometry(H1), R.pool_geometry(W1)
        for ho in range(HP):
            for wo in range(WP):
                for c in range(3):
                    m, k = None, None
                    for a in range(3):
                        for b in range(3):
                            hi, wi = 2 * ho - pt + a, 2 * wo - pl + b
                            if 0 <= hi < H1 and 0 <= wi < W1 and (k is None or float(x[0, hi, wi, c]) > m):
                                m, k = float(x[0, hi, wi, c]), a * 3 + b
                    assert int(rec[0, ho, wo, c]) == k and float(pool[0, ho, wo, c]) == m, (H1, W1, ho, wo, c)
        valid = R.pool_valid(H1, W1)
        assert bool(valid[int(rec[0, 0, 0, 0]), 0, 0]) and int(rec[0, 0, 0, 0]) == (4 if pt and pl else 0)
        # without the rule a window of -inf keeps position 0; everywhere else the two agree
        pool0, rec0 = R.pool_first_max(x)
        assert torch.equal(rec0[pool0 > -float("inf")], rec[pool0 > -float("inf")]) and int(rec0[0, 0, 0, 0]) == 0


@pytest.mark.parametrize("hw", [(9, 12), (10, 7)])
def test_root_forward_is_the_root_block(hw):
    """root_forward against torch's float64 conv + BN + ReLU + max-pool; the cell modes differ from it by what their cells drop."""
    H, W = hw
    g = torch.Generator().manual_seed(H * 100 + W)
    fr = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    w = torch.randn((7, 7, 3, 64), generator=g) * 0.05
    sc, bi = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 20
    mean = (123.68, 116.779, 103.939)
    x = (fr.float() - torch.tensor(mean)).double().permute(0, 3, 1, 2)
    y = F.conv2d(x, w.double().permute(3, 2, 0, 1), stride=2, padding=3)
    c1 = torch.relu(y * sc.double()[None, :, None, None] + bi.double()[None, :, None, None])
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    pt, pl = R.pool_geometry(H1)[1], R.pool_geometry(W1)[1]
    HP, WP = R.pool_geometry(H1)[0], R.pool_geometry(W1)[0]
    padded = F.pad(c1, (pl, 2 * WP + 1 - W1 - pl, pt, 2 * HP + 1 - H1 - pt), value=-float("inf"))
    pool = F.max_pool2d(padded, 3, 2)[:, :, :HP, :WP]
    top = float(c1.max())
    got_c1, got_pool = R.root_forward(fr, w, sc, bi, mean, "f32")
    assert got_c1.shape == (2, H1, W1, 64) and got_pool.shape == (2, HP, WP, 64)
    assert float((got_c1 - c1.permute(0, 2, 3, 1)).abs().max()) < 1e-12 * top
    assert float((got_pool - pool.permute(0, 2, 3, 1)).abs().max()) < 1e-12 * top
    # H2 cells keep 22 bits of every weight and the mean's fraction rides on the fourth channel: 49 x 4 products of |x| <= 132
    h2 = R.root_forward(fr, w, sc, bi, mean, "h2")[0]
    assert float((h2 - got_c1).abs().max()) < 196 * 132 * 2.0 ** -22 * float(w.abs().max()) * 1.5
    # H1 cells keep 11 bits; scaled units scale both results
    h1 = R.root_forward(fr, w, sc, bi, mean, "h1", scale=4.0)
    assert float((h1[0] / 4.0 - got_c1).abs().max()) < 196 * 132 * 2.0 ** -11 * float(w.abs().max()) * 1.5
    assert float((h1[0] / 4.0 - got_c1).abs().max()) > 100 * float((h2 - got_c1).abs().max())     # (and the two modes are different things)
    # identical patches give bitwise identical values: a frame of one colour, away from the border
    flat = torch.full((1, 40, 40, 3), 77, dtype=torch.uint8)
    inner = R.root_forward(flat, w, sc, bi, mean, "h1")[0][0, 2:-2, 2:-2]
    assert bool((inner == inner[0, 0]).all())
