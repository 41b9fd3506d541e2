"""The halo walk (MODE 3 of conv_igemm_split_ls, csrc/dgp_conv_split.hip: the K loop of every 3 x 3 / stride-1 conv of blocks 2-4 at
batch 32, on both cell tiers) against float64, at the edges of its ring.  The walk takes a launch only where the grid has more than one
tile per CU (the deep ring wins below that on H2), so every case builds its shape from the device's own CU count, ASSERTS THROUGH THE
PLAN QUERY (engine.conv2d_plan) the path it is about -- mode, deep, h1, tail_ksplit == 0, st_gn == 0; a case whose plan differs fails --
runs the layer through engine.conv2d_h2 / conv2d_h1 into a NaN-filled output and compares with a float64 reference that convolves the
values the cells hold (H1: weights rounded to fp16 on the panel's scale), computed tap by tap on the device.  Scale, bias and ReLU are
on in every case; Cout = 512 (four column tiles), so a case has about 33 n_cu pixels.

Tolerances are the project's own: H2 max error < 2e-5 of max |ref| and the tracked range within 1e-4 (tests/test_h2_gpu.py); H1 the
per-element bound 2^-11 |ref| (1 + 1e-3) + 2^-24 2^-y_exp + 4e-6 max |ref| and the range within 1e-4 (tests/test_h1_gpu.py).  The tap probes
are exact.  Measured errors: EXPERIMENTS.md, "The halo walk against float64"."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_h1_gpu import _w_exp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
TIERS = ("h2", "h1")
COUT = 512


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    return engine


@pytest.fixture(scope="module")
def n_cu(eng):
    return eng.conv2d_plan((1, 1, 128, 64), (1, 1, 64, 128))["n_cu"]


def _frames(n_cu, H, W, extra_tiles=1):
    """the smallest N whose N x H x W frames give more than n_cu tiles of 128 pixels x 128 of the 512 columns, with a ragged last tile"""
    N = -(-(n_cu // 4 + extra_tiles - 1) * 128 // (H * W))
    while -(-N * H * W // 128) * 4 <= n_cu or (N * H * W) % 128 == 0:
        N += 1
    return N, H, W


def _conv_f64(xq, wq, d):
    """float64 3 x 3 / stride 1 / pad d conv, tap by tap: xq [N,H,W,Cin] float64 (device), wq [3,3,Cin,Cout] float64 (device)"""
    N, H, W, Cin = xq.shape
    xp = torch.zeros((N, H + 2 * d, W + 2 * d, Cin), dtype=torch.float64, device="cuda")
    xp[:, d:d + H, d:d + W] = xq
    acc = torch.zeros((N * H * W, wq.shape[3]), dtype=torch.float64, device="cuda")
    for a in range(3):
        for b in range(3):
            acc += xp[:, a * d:a * d + H, b * d:b * d + W].reshape(N * H * W, Cin) @ wq[a, b]
    return acc.reshape(N, H, W, -1)


def _to_cells(eng, tier, t, e):
    """fp32 -> (cells, the float64 values they hold)"""
    if tier == "h2":
        c = eng.f32_to_h2(t, e)
        return c, eng.h2_to_f32(c, e).double()
    c = eng.f32_to_h1(t, e)
    return c, eng.h1_to_f32(c, e).double()


def _launch(eng, tier, nhw, cin, d, x, w, scale, bias, ref_lin, want, label, res=None, exact=False):
    """plan query (asserted against `want`) -> cells -> launch into a NaN-filled output -> error against relu(ref_lin(xq, wq) [+ residual])"""
    N, H, W = nhw
    h1 = tier == "h1"
    fmt = 2 if h1 else 1
    pl = eng.conv2d_plan((N, H, W, cin), w.shape, rate=d, pad_t=d, pad_l=d, in_fmt=fmt, out_fmt=fmt, res_fmt=fmt if res == "cells" else 0,
                         res_stride=1 if res else 0, res_hw=(H, W) if res else (0, 0))
    want = dict(want, h1=int(h1), tail_ksplit=0, st_gn=0, tile=16)
    assert {k: pl[k] for k in want} == want and pl["grid"] == pl["mtiles"] * pl["ntiles"], (label, tier, pl, want)
    x_exp = eng.h2_exp_for(float(x.abs().max()))
    xh, xq = _to_cells(eng, tier, x, x_exp)
    if exact:
        assert torch.equal(xq, x.double())
    wt = torch.from_numpy(w).cuda()
    wq = (wt * 2.0 ** _w_exp(w)).to(torch.float16).double() * 2.0 ** -_w_exp(w) if h1 else wt.double()
    ref = ref_lin(xq, wq)
    if scale is not None:
        ref = ref * torch.from_numpy(scale).double().cuda()
    ref = ref + torch.from_numpy(bias).double().cuda()
    res_t, res_exp = None, 0
    if res:
        g = torch.Generator(device="cuda").manual_seed(N * H * W)
        r = torch.randn((N, H, W, w.shape[3]), device="cuda", generator=g) * 2.0
        if res == "cells":
            res_exp = eng.h2_exp_for(float(r.abs().max()))
            res_t, rq = _to_cells(eng, tier, r, res_exp)
        else:
            res_t, rq = r, r.double()
        ref = ref + rq
    ref = torch.relu(ref)
    mx = float(ref.abs().max())
    y_exp = eng.h2_exp_for(mx)
    kw = dict(rate=d, pad_t=d, pad_l=d, out_hw=(H, W), scale=scale, bias=bias, residual=res_t, res_stride=1 if res else 0, res_exp=res_exp,
              relu=True, y_exp=y_exp)
    if h1:
        y = torch.full((N, H, W, w.shape[3]), NAN, device="cuda", dtype=torch.float16)
        y2, yr = eng.conv2d_h1(xh, x_exp, w, y_is_h1=True, out=y, **kw)
        out = eng.h1_to_f32(y, y_exp).double()
        tol = 2.0 ** -11 * ref.abs() * (1 + 1e-3) + 2.0 ** -24 * 2.0 ** -y_exp + 4e-6 * mx
    else:
        y = torch.full((N, H, W, w.shape[3]), NAN, device="cuda")
        y2, yr = eng.conv2d_h2(xh, x_exp, w, y_is_h2=True, res_is_h2=res == "cells", out=y, **kw)
        out = eng.h2_to_f32(y, y_exp).double()
        tol = torch.full_like(ref, 2e-5 * mx)
    assert y2 is y
    diff = (out - ref).abs()                                         # (NaN where a tile was not written: fails every bound)
    err, worst = float(diff.max() / mx), float((diff / tol).max())
    print("[halo-walk] %s %s %dx%dx%d d %d cin %d res %s: mode %d deep %d grid %d: err %.3g of max |ref|, %.3g of the bound"
          % (label, tier, N, H, W, d, cin, res, pl["mode"], pl["deep"], pl["grid"], err, worst))
    if exact:
        assert torch.equal(out, ref), (label, tier, int((out != ref).sum()))
    assert bool((diff <= tol).all()) and not bool(torch.isnan(out).any()), (label, tier, err, worst)
    assert abs(float(yr.max()) - mx) <= 1e-4 * mx, (label, tier, float(yr.max()), mx)
    return err


def _layer(eng, tier, nhw, cin, d, want, label, res=None, cout=COUT):
    """a random layer: ReLU'd activations, weights ~ N(0, 1 / K), scale 1 +- 0.1, bias +- 0.1"""
    N, H, W = nhw
    seed = (N * 1000003 + H * 1009 + W * 31 + cin + d) % (2 ** 31)
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    x = torch.relu(torch.randn((N, H, W, cin), device="cuda", generator=g)) * 3.0
    w = (rng.standard_normal((3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    scale = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    return _launch(eng, tier, nhw, cin, d, x, w, scale, bias, lambda xq, wq: _conv_f64(xq, wq, d), want, label, res)


def _tap_probe(eng, tier, nhw, d, want, label):
    """One-hot weights: output channel co copies tap co % 9 of input channel co // 9 (57 of 64 channels: one H1 chunk, two H2 chunks);
    activations 1 + (131 m + 17 c) mod P name pixel and channel and are never 0, what a masked tap reads (P = 8191 on H2: both cells of a
    pair are needed; 2047 on H1: integers fp16 holds).  Every sum has one non-zero term, biases are integers <= 0: exact, output cell included."""
    N, H, W = nhw
    cin, M = 64, N * H * W
    P = 2047 if tier == "h1" else 8191
    x = (1 + (torch.arange(M, device="cuda")[:, None] * 131 + torch.arange(cin, device="cuda")[None, :] * 17) % P).float().reshape(N, H, W, cin)
    w = np.zeros((3, 3, cin, COUT), np.float32)
    co = np.arange(COUT)
    w[(co % 9) // 3, (co % 9) % 3, co // 9, co] = 1.0
    bias = -((co * 37) % 301).astype(np.float32) * (co % 3 != 0)
    err = _launch(eng, tier, nhw, cin, d, x, w, None, bias, lambda xq, wq: _conv_f64(xq, wq, d), want, label + " probe", exact=True)
    assert err == 0.0


def _respawn(request, **env):
    """Switches read once per process: True in a process that has them (the body runs); otherwise the test runs again in a child pytest
    process with them, must pass there, and the body returns at once"""
    if all(os.environ.get(k) == v for k, v in env.items()):
        return True
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-rA", "-s", "-m", "gpu", "-p", "no:cacheprovider"], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("[halo-walk]")))
    assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    return False


WALK, PER_TAP = dict(mode=3, deep=0), dict(mode=1, deep=0)
CHUNK = {"h2": 32, "h1": 64}           # channels of one K-step's 128-byte line per pixel

# name -> (H, W, dilation, Cin (None: one chunk), the path at the default switches)
DEFAULT_CASES = {
    "frames_7x9": (7, 9, 1, 128, WALK),             # a 128-pixel window spans three frames; every kind of masked tap in every row block
    "single_row_frames": (1, 29, 1, 128, WALK),     # H = 1: every tap off the centre row is masked
    "w_2": (5, 2, 1, 128, WALK),                    # two pixels per row: every tap but the centre column masked somewhere
    "w_1": (9, 1, 1, 128, PER_TAP),                 # one pixel per row: not the walk
    "d1_w115": (5, 115, 1, 128, WALK),              # S = 360: the last strip that fits the ring whole
    "d1_w116": (5, 116, 1, 128, PER_TAP),           # S = 362
    "d2_w57": (5, 57, 2, 128, WALK),                # S = 360
    "d2_w58": (5, 58, 2, 128, PER_TAP),             # S = 364
    "d3_w37": (7, 37, 3, 128, WALK),                # S = 356
    "d3_w38": (7, 38, 3, 128, PER_TAP),             # S = 362
    "one_chunk": (11, 13, 1, None, WALK),           # nine K-steps in all, the loaders two steps ahead
    "block4_cin512_d2": (30, 40, 2, 512, WALK),     # the deepest K loop: 144 K-steps (72 on H1)
}


def _run_case(eng, n_cu, tier, name, want=None, probe=False):
    H, W, d, cin, path = DEFAULT_CASES[name]
    if probe:
        return _tap_probe(eng, tier, _frames(n_cu, H, W), d, want or path, name)
    return _layer(eng, tier, _frames(n_cu, H, W), cin or CHUNK[tier], d, want or path, name)


# ---------------------------------------------------------------- default switches
@pytest.mark.parametrize("name", list(DEFAULT_CASES))
@pytest.mark.parametrize("tier", TIERS)
def test_ring_edges_at_the_default_switches(eng, n_cu, tier, name):
    _run_case(eng, n_cu, tier, name)


@pytest.mark.parametrize("tier,res", [("h2", "cells"), ("h2", "f32"), ("h1", "cells")])
def test_walk_with_a_residual(eng, n_cu, tier, res):
    """same-grid residual in the tier's cells, and on H2 in fp32 (the 16-bit tier has H1 residuals only), on the 7 x 9 frames"""
    _layer(eng, tier, _frames(n_cu, 7, 9), 128, 1, WALK, "frames_7x9", res)


@pytest.mark.parametrize("extra_tiles,want", [(0, dict(mode=1, deep=1)), (1, WALK)])
def test_one_tile_per_cu_is_the_deep_ring_a_few_more_the_walk(eng, n_cu, extra_tiles, want):
    """the same H2 layer (3 x H x 41, 128 -> 512) on n_cu / 4 row tiles -- at most one tile per CU: deep ring, per-tap loaders -- and on one
    row tile more"""
    mt = n_cu // 4 + extra_tiles
    h = (mt * 128 - 1) // (3 * 41)
    assert -(-3 * h * 41 // 128) == mt and (3 * h * 41) % 128 != 0
    _layer(eng, "h2", (3, h, 41), 128, 1, dict(want, mtiles=mt, ntiles=4, grid=4 * mt), "one tile per CU + %d" % extra_tiles)


@pytest.mark.parametrize("name", ["frames_7x9", "w_2", "d1_w115", "d1_w116", "d2_w57", "d3_w37"])
@pytest.mark.parametrize("tier", TIERS)
def test_every_tap_of_every_pixel_exact(eng, n_cu, tier, name):
    _run_case(eng, n_cu, tier, name, probe=True)


# ---------------------------------------------------------------- the switch set: child processes
@pytest.mark.parametrize("tier", TIERS)
def test_sliding_ring_with_the_walk_forced(eng, n_cu, tier, request):
    """DGP_HALO=2: strips longer than the ring (S = 364 .. 588 pixels of 360), which slide through it inside a channel chunk, up to the hard
    capacity d (W - 2) + 128 = 352 (d 2 at W 114, d 1 at W 226: the next step's window starts where the ring's last free group ends) and
    the per-tap loaders one pixel beyond it; dilation 3 on odd sizes; block4 conv2 of the 1280 x 720 network"""
    if not _respawn(request, DGP_HALO="2"):
        return
    for H, W, d, want in ((5, 58, 2, WALK), (5, 114, 2, WALK), (5, 115, 2, PER_TAP), (5, 226, 1, WALK), (5, 227, 1, PER_TAP), (33, 47, 3, WALK)):
        _layer(eng, tier, _frames(n_cu, H, W), 128, d, want, "forced d%d_w%d" % (d, W))
    _layer(eng, tier, (max(3, _frames(n_cu, 45, 80)[0]), 45, 80), 512, 2, WALK, "forced 45x80")
    for H, W, d in ((5, 114, 2), (5, 226, 1), (33, 47, 3)):
        _tap_probe(eng, tier, _frames(n_cu, H, W), d, WALK, "forced d%d_w%d" % (d, W))


@pytest.mark.parametrize("tier", TIERS)
def test_per_tap_loaders_with_the_walk_switched_off(eng, n_cu, tier, request):
    """DGP_HALO=0: every default case on the three-stage per-tap LDS-DMA kernel (mode 1, not the deep ring), and the probes"""
    if not _respawn(request, DGP_HALO="0"):
        return
    for name in DEFAULT_CASES:
        _run_case(eng, n_cu, tier, name, want=PER_TAP)
    for name in ("frames_7x9", "w_2", "d2_w57"):
        _run_case(eng, n_cu, tier, name, want=PER_TAP, probe=True)


