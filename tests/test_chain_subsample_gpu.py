"""X' keep stride of the chain / unit kernels (csrc/dgp_chain.hip, ChainArgs::xkeep; include/dgp_hip.h dgp_chain_xkeep / dgp_unit_xkeep).

slim's resnet_v1 puts a block's stride on its last unit, whose shortcut is subsample(x, 2) = x[:, ::2, ::2].  The engine's launch in
front of such a unit computes that unit's conv1 itself, so its X' is read at even rows and columns only, and only those pixels are
stored (DGP_XOUT_SUBSAMPLE, default 1).  Nothing else may change: the kept pixels, R1' and every range slot are bit-identical to the
full store, and the dropped pixels are not written at all.  Every condition here is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5

CHAIN_CASES = [
    # N, Ho, Wo, C, C1          (identity units: CIN2 = 0, res_mode 1)
    (2, 15, 21, 128, 128),      # block2: odd rows and columns, ragged last tile, frame boundary inside a 16-pixel row block
    (2, 17, 23, 64, 64),        # block1's chain instance
    (1, 1, 1, 128, 128),        # one pixel
]
UNIT_CASES = [
    # N, H, W                   (C = C1 = 64, identity)
    (2, 13, 21),                # ragged in both directions
    (1, 4, 16),                 # exactly one tile
    (1, 5, 17),                 # one row and one column past a tile
]


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], t.shape[1], t.shape[2], -1)


def _sentinel_like(t):
    b = torch.empty_like(t)
    b.view(torch.uint8).fill_(SENTINEL)
    return b


def _check_pair(full, sub):
    """full / sub: (x_out, r1, range slots...) of the launch with xout_keep 1 / 2 (x_out of `sub` pre-filled with the sentinel)"""
    xa, xb = _bytes(full[0]), _bytes(sub[0])
    H, W = xa.shape[1], xa.shape[2]
    assert torch.equal(xa[:, ::2, ::2], xb[:, ::2, ::2])
    assert not bool((xa[:, ::2, ::2] == SENTINEL).all())          # (the kept pixels were written, in both runs)
    dropped = torch.ones((H, W), dtype=torch.bool, device=xa.device)
    dropped[::2, ::2] = False
    assert bool((xb[:, dropped] == SENTINEL).all())               # not stored at all, rather than stored and unread
    assert torch.equal(_bytes(full[1]), _bytes(sub[1]))           # R1' everywhere
    for a, b in zip(full[2:], sub[2:]):                           # range slots: every pixel counts, kept or not
        assert torch.equal(a, b)
        assert float(a.max()) > 0.0


def _weights(rng, C, C1):
    C4 = 4 * C
    w3 = (rng.standard_normal((C, C4)) / np.sqrt(C)).astype(np.float32)
    s3 = (1 + 0.1 * rng.standard_normal(C4)).astype(np.float32)
    b3 = (0.1 * rng.standard_normal(C4)).astype(np.float32)
    w1 = (rng.standard_normal((C4, C1)) / np.sqrt(C4)).astype(np.float32)
    s1 = (1 + 0.1 * rng.standard_normal(C1)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(C1)).astype(np.float32)
    return w3, s3, b3, w1, s1, b1


def _tail_exps(engine, r2, x, w3, s3, b3, w1, s1, b1):
    """scale exponents of X' and R1' from an fp32 evaluation of the two pointwise convs (any sane scale serves: both runs share it)"""
    t = lambda a: torch.from_numpy(a).cuda()
    xo = torch.relu((r2.reshape(-1, r2.shape[-1]) @ t(w3)) * t(s3) + t(b3) + x.reshape(-1, x.shape[-1]))
    r1 = torch.relu((xo @ t(w1)) * t(s1) + t(b1))
    return engine.h2_exp_for(float(xo.max())), engine.h2_exp_for(float(r1.max()))


@pytest.mark.parametrize("h1", [False, True], ids=["h2", "h1"])
@pytest.mark.parametrize("case", CHAIN_CASES)
def test_chain_kernel_stores_only_the_even_pixels(lib_built, case, h1):
    from deepgraphpose_amd import engine
    N, Ho, Wo, C, C1 = case
    seed = 1000 + 7 * Ho + Wo + C
    g = torch.Generator(device="cuda").manual_seed(seed)
    r2 = torch.relu(torch.randn((N, Ho, Wo, C), device="cuda", generator=g)) * 3.0
    x = torch.relu(torch.randn((N, Ho, Wo, 4 * C), device="cuda", generator=g)) * 2.0
    wts = _weights(np.random.default_rng(seed), C, C1)
    e_r2, e_x = engine.h2_exp_for(float(r2.max())), engine.h2_exp_for(float(x.max()))
    e_xo, e_r1 = _tail_exps(engine, r2, x, *wts)
    pack = engine.f32_to_h1 if h1 else engine.f32_to_h2
    r2c, xc = pack(r2, e_r2), pack(x, e_x)
    full = engine.chain_h2(r2c, e_r2, xc, e_x, *wts, 1, e_xo, e_r1, h1=h1, xout_keep=1)
    buf = _sentinel_like(full[0])
    sub = engine.chain_h2(r2c, e_r2, xc, e_x, *wts, 1, e_xo, e_r1, h1=h1, xout_keep=2, xout=buf)
    assert sub[0].data_ptr() == buf.data_ptr()
    _check_pair(full, sub)


@pytest.mark.parametrize("h1", [False, True], ids=["h2", "h1"])
@pytest.mark.parametrize("case", UNIT_CASES)
def test_unit_kernel_stores_only_the_even_pixels(lib_built, case, h1):
    from deepgraphpose_amd import engine
    N, H, W = case
    C = C1 = 64
    seed = 2000 + 7 * H + W
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    r1 = torch.relu(torch.randn((N, H, W, C), device="cuda", generator=g)) * 3.0
    x = torch.relu(torch.randn((N, H, W, 4 * C), device="cuda", generator=g)) * 2.0
    w2 = (rng.standard_normal((3, 3, C, C)) / np.sqrt(9 * C)).astype(np.float32)
    s2 = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(C)).astype(np.float32)
    wts = _weights(rng, C, C1)
    t = lambda a: torch.from_numpy(a).cuda()
    r2 = torch.nn.functional.conv2d(r1.permute(0, 3, 1, 2), t(w2).permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    r2 = torch.relu(r2 * t(s2) + t(b2)).contiguous()
    e_r1, e_x, e_r2 = engine.h2_exp_for(float(r1.max())), engine.h2_exp_for(float(x.max())), engine.h2_exp_for(float(r2.max()))
    e_xo, e_o = _tail_exps(engine, r2, x, *wts)
    pack = engine.f32_to_h1 if h1 else engine.f32_to_h2
    r1c, xc = pack(r1, e_r1), pack(x, e_x)
    full = engine.unit_h2(r1c, e_r1, xc, e_x, w2, s2, b2, e_r2, *wts, 1, e_xo, e_o, h1=h1, xout_keep=1)
    buf = _sentinel_like(full[0])
    sub = engine.unit_h2(r1c, e_r1, xc, e_x, w2, s2, b2, e_r2, *wts, 1, e_xo, e_o, h1=h1, xout_keep=2, xout=buf)
    assert sub[0].data_ptr() == buf.data_ptr()
    _check_pair(full, sub)


@pytest.mark.parametrize("h1", [False, True], ids=["h2", "h1"])
@pytest.mark.parametrize("keep", [0, 3, -1])
def test_an_invalid_keep_stride_is_refused(lib_built, keep, h1):
    from deepgraphpose_amd import _lib, engine
    dt = torch.float16 if h1 else torch.float32
    C = 64
    r = torch.zeros((1, 4, 16, C), device="cuda", dtype=dt)
    x = torch.zeros((1, 4, 16, 4 * C), device="cuda", dtype=dt)
    w3, w1, w2 = np.zeros((C, 4 * C), np.float32), np.zeros((4 * C, C), np.float32), np.zeros((3, 3, C, C), np.float32)
    with pytest.raises(_lib.DgpError, match="xout_keep"):
        engine.chain_h2(r, 0, x, 0, w3, None, None, w1, None, None, 1, 0, 0, h1=h1, xout_keep=keep)
    with pytest.raises(_lib.DgpError, match="xout_keep"):
        engine.unit_h2(r, 0, x, 0, w2, None, None, 0, w3, None, None, w1, None, None, 1, 0, 0, h1=h1, xout_keep=keep)


# ---- whole network: DGP_XOUT_SUBSAMPLE is read once per process, so each setting runs in a child process (all nets in one child) ----------

NETS = [
    # depth, H, W, tier
    (50, 96, 128, "parity"),
    (50, 96, 128, "f16"),
    (50, 100, 132, "parity"),       # block1 on a 25 x 33 grid, block2 on 13 x 17: odd in both directions
    (50, 100, 132, "f16"),
    (101, 96, 128, "parity"),
]

_CHILD = r'''
import sys, numpy as np, torch
from deepgraphpose_amd.engine import DGPNet
from deepgraphpose_amd.synthetic import make_frames, make_weights
out = {}
for k, (depth, H, W, tier) in enumerate(%r):
    net = DGPNet(depth, 4, H, W, max_batch=3, tier=None if tier == "parity" else tier)
    net.load_weights(make_weights(depth, 4, False, seed=5, head_std=0.05))
    frames = torch.from_numpy(make_frames(3, H, W, 4, seed=6)).cuda()
    net.forward(frames)                                   # calibration pass + a chained pass
    sc, feats = net.forward(frames, want_features=True)   # steady state: chained pass only
    mu, conf, idx = net.infer(frames)
    ov, ncal = net.range_status()
    for name, v in (("sc", sc), ("feats", feats), ("mu", mu), ("conf", conf), ("idx", idx)):
        out["%%d_%%s" %% (k, name)] = v.cpu().numpy()
    out["%%d_status" %% k] = np.array([int(ov), ncal])
np.savez(sys.argv[1], **out)
''' % (NETS,)


@pytest.fixture(scope="module")
def ab_runs(lib_built, tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    td = tmp_path_factory.mktemp("xout_subsample")
    runs = {}
    for flag in ("1", "0"):
        path = str(td / ("o%s.npz" % flag))
        subprocess.check_call([sys.executable, "-c", _CHILD, path], env=dict(os.environ, DGP_XOUT_SUBSAMPLE=flag, PYTHONPATH=root), cwd=root)
        runs[flag] = dict(np.load(path))
    return runs


@pytest.mark.parametrize("k", range(len(NETS)), ids=["r%d_%dx%d_%s" % n for n in NETS])
def test_network_is_bit_identical_with_and_without_the_dead_stores(ab_runs, k):
    a, b = ab_runs["1"], ab_runs["0"]
    for name in ("sc", "feats", "mu", "conf", "idx", "status"):
        key = "%d_%s" % (k, name)
        assert a[key].shape == b[key].shape and a[key].size > 0
        assert np.array_equal(a[key], b[key]), key
    assert np.isfinite(a["%d_sc" % k]).all() and a["%d_status" % k][0] == 0
