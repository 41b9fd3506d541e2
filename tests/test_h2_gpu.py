"""The H2 activation format of the inference engine (include/dgp_hip.h, "H2"; EXPERIMENTS.md section 3): fp16 high / low cell pairs
written by the producing epilogue, consumed by K loops that only issue ds_read + MFMA.

Layer tests: fp32 inputs are converted to H2, the conv runs H2 -> H2 (or H2 -> fp32) through the cell kernels, the result is
converted back and compared with a float64 reference.  Tolerance 2e-5 relative, the same as the fp32-activation layer tests: the
format keeps 22 significant bits.  Network-level parity of the H2 path is what every test that calls DGPNet.forward / infer
checks (test_parity_gpu.py); here: calibration, overflow detection and recovery."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_h2_converters_keep_22_bits(lib_built):
    from deepgraphpose_amd import engine
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((3, 17, 64), device="cuda", generator=g) * 37.0
    x[0, 0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e-6, 3e4 / 64, 123.456, -7.25], device="cuda")
    e = engine.h2_exp_for(float(x.abs().max()))
    assert 2 ** 10 <= float(x.abs().max()) * 2.0 ** e < 2 ** 11
    back = engine.h2_to_f32(engine.f32_to_h2(x, e), e)
    err = (back.double() - x.double()).abs()
    floor = torch.tensor(2.0 ** -33 * float(x.abs().max()), device="cuda", dtype=torch.float64)
    assert bool((err <= torch.maximum(2.0 ** -22 * x.double().abs(), floor)).all())      # 22 bits; tiny elements: absolute bound
    assert float(err.max()) <= 2.0 ** -22 * float(x.abs().max())
    # values with <= 22 significant bits survive exactly
    y = (torch.randint(-2 ** 20, 2 ** 20, (4, 5, 16), device="cuda", generator=g).float()) * 2.0 ** -12
    e2 = engine.h2_exp_for(float(y.abs().max()))
    assert torch.equal(engine.h2_to_f32(engine.f32_to_h2(y, e2), e2), y)
    raw = engine.f32_to_h2(x, e).view(torch.int32).cpu().numpy().reshape(-1, 8)      # cell layout: 4 dwords high halves, 4 dwords low
    hi = raw[:, :4].copy().view(np.float16).astype(np.float64)
    lo = raw[:, 4:].copy().view(np.float16).astype(np.float64)
    np.testing.assert_array_equal(hi + lo, back.cpu().numpy().astype(np.float64).reshape(-1, 8) * 2.0 ** e)


H2_CONV_CASES = [
    # N, H, W, Cin, Cout, k, stride, rate, residual (0 none, 1 same grid fp32, 2 same grid H2, 3 strided H2), y_is_h2
    (2, 17, 23, 64, 256, 1, 1, 1, 2, True),        # conv3 of an identity unit (128 x 128 DMA kernel, pointwise loader)
    (1, 30, 40, 256, 64, 1, 1, 1, 0, True),        # conv1 -> 64 channels (128 x 64 kernel)
    (2, 19, 21, 64, 64, 3, 1, 1, 0, True),         # 3x3, 128 x 64 kernel
    (2, 19, 21, 64, 64, 3, 2, 1, 0, True),         # strided 3x3
    (1, 15, 20, 128, 128, 3, 1, 2, 0, True),       # dilated 3x3, 128 x 128 DMA kernel
    (1, 30, 40, 512, 512, 3, 1, 2, 1, True),       # block4 conv2 shape (+ an fp32 residual)
    (2, 20, 24, 256, 512, 1, 2, 1, 0, True),       # strided shortcut conv
    (2, 10, 12, 512, 1024, 1, 1, 1, 3, True),      # conv3 of a strided unit: residual subsampled from the 2x finer grid
    (1, 30, 40, 2048, 128, 1, 1, 1, 0, False),     # the head's pointwise GEMM: H2 in, fp32 out
    (32, 30, 40, 1024, 256, 1, 1, 1, 0, True),     # batch-32 block3 conv1: 600 tiles in the pairing order of two column tiles (no tail slab here: tests/test_conv_plan_gpu.py splits it)
    (32, 30, 40, 512, 512, 3, 1, 2, 2, True),      # batch-32 block4 conv2 (+ an H2 residual): the deepest K loop at its real size
    (11, 30, 40, 2048, 512, 1, 1, 1, 0, True),     # block4 conv1 at 11 frames: 416 tiles, K = 2048
    # round 4, shapes of the halo walk (MODE 3 of the dominant kernel: 3x3 / stride 1 on a pixel ring in LDS, taps masked by the compute waves).
    # The walk takes a launch only where the grid has MORE tiles than the chip has CUs: case12 to case19 have 1 to 116 tiles, so on a
    # full-size chip (256 CUs) every one of them runs the deep ring with the per-tap loaders (mode 1, deep 1), and only the 1200 tiles of
    # case10 above walk the ring.  The test asserts the path each case takes on this device through the plan query; the walk's own edges
    # are the cases of tests/test_halo_walk_gpu.py, which sizes them from the CU count.
    (3, 7, 9, 128, 128, 3, 1, 1, 0, True),         # case12: frames smaller than a tile -- a 128-pixel window spans three frames; ragged last tile (2 tiles)
    (2, 30, 40, 256, 256, 3, 1, 1, 0, True),       # case13: block3 conv2 (38 tiles)
    (1, 60, 80, 128, 128, 3, 1, 1, 2, True),       # case14: block2 conv2 (+ an H2 residual; 38 tiles)
    (1, 20, 118, 128, 128, 3, 1, 2, 0, True),      # case15: d (W - 2) + 128 = 360, beyond the ring's HALO_C - 8 = 352 (the widest row it takes at d = 2 is W = 114): per-tap loaders everywhere
    (1, 9, 200, 128, 128, 3, 1, 2, 0, True),       # case16: wider still -> the per-tap loaders
    (1, 45, 80, 512, 512, 3, 1, 2, 0, True),       # case17: block4 conv2 of the 1280 x 720 network (116 tiles; with more tiles than CUs still per-tap: S = 452 > 360)
    (2, 5, 2, 128, 128, 3, 1, 1, 0, True),         # case18: two pixels per row (every tap but the centre column masked somewhere; 1 tile)
    (1, 33, 47, 128, 256, 3, 1, 3, 0, True),       # case19: dilation 3, odd sizes (26 tiles; with more tiles than CUs per-tap: S = 416 > 360)
]


def _case_geometry(case):
    """-> pad, Ho, Wo of a case of H2_CONV_CASES"""
    N, H, W, Cin, Cout, k, stride, rate = case[:8]
    keff = (k - 1) * rate + 1
    pad = (keff - 1) // 2
    Ho = (H + 2 * pad - keff) // stride + 1 if stride > 1 else H
    Wo = (W + 2 * pad - keff) // stride + 1 if stride > 1 else W
    if k == 1 and stride > 1:
        pad, Ho, Wo = 0, (H + stride - 1) // stride, (W + stride - 1) // stride
    return pad, Ho, Wo


def _path_of(case, n_cu, halo_env):
    """(mode, deep) of a case on n_cu CUs with DGP_HALO = halo_env, from the restated rules (tests/_conv_plan_ref.py): the 128-column tile
    from 128 output channels on, pointwise walk (2) for 1 x 1 / stride 1, else per-tap (1) or the halo ring (3)"""
    import _conv_plan_ref as R
    N, H, W, Cin, Cout, k, stride, rate, _, y_h2 = case
    pad, Ho, Wo = _case_geometry(case)
    bn = 128 if Cout >= 128 else 64
    deep = bn == 128 and R.deep_ring(-(-N * Ho * Wo // 128), Cout // bn, k * k * Cin // 32, n_cu, dma=True)
    halo = R.halo_walk(1, int(y_h2), (k, k), stride, rate, pad, pad, (H, W), (Ho, Wo), dma128=bn == 128, deep=deep, halo_env=halo_env)
    return (3 if halo else 2 if (k == 1 and stride == 1) else 1), int(deep)


def _path_line(case, path):
    return "[h2-path] %r mode %d deep %d" % (case, path[0], path[1])


@pytest.mark.parametrize("case", H2_CONV_CASES)
def test_conv_on_h2_tensors_matches_float64(lib_built, case):
    import os
    from deepgraphpose_amd import engine
    from oracle import dgp_oracle as O
    N, H, W, Cin, Cout, k, stride, rate, res_kind, y_h2 = case
    # the path this launch takes on this device under this process's DGP_HALO, asserted through the plan query and reported
    pad_, Ho_, Wo_ = _case_geometry(case)
    pl = engine.conv2d_plan((N, H, W, Cin), (k, k, Cin, Cout), stride=stride, rate=rate, pad_t=pad_, pad_l=pad_, out_hw=(Ho_, Wo_), in_fmt=1,
                            out_fmt=int(y_h2), res_fmt=int(res_kind in (2, 3)), res_stride={0: 0, 1: 1, 2: 1, 3: 2}[res_kind],
                            res_hw={0: (0, 0), 1: (Ho_, Wo_), 2: (Ho_, Wo_), 3: (2 * Ho_ - 1, 2 * Wo_)}[res_kind])
    print(_path_line(case, (pl["mode"], pl["deep"])))
    assert (pl["mode"], pl["deep"]) == _path_of(case, pl["n_cu"], int(os.environ.get("DGP_HALO", "1"))), pl
    g = torch.Generator(device="cuda").manual_seed(abs(hash(case)) % (2 ** 31))
    x = torch.relu(torch.randn((N, H, W, Cin), device="cuda", generator=g)) * 3.0
    rngw = np.random.default_rng(abs(hash(case)) % (2 ** 31))
    w = (rngw.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    scale = (1 + 0.1 * rngw.standard_normal(Cout)).astype(np.float32)
    bias = (0.1 * rngw.standard_normal(Cout)).astype(np.float32)
    keff = (k - 1) * rate + 1
    pad = (keff - 1) // 2
    Ho = (H + 2 * pad - keff) // stride + 1 if stride > 1 else H
    Wo = (W + 2 * pad - keff) // stride + 1 if stride > 1 else W
    if k == 1 and stride > 1:
        pad, Ho, Wo = 0, (H + stride - 1) // stride, (W + stride - 1) // stride
    x_exp = engine.h2_exp_for(float(x.abs().max()))
    xh = engine.f32_to_h2(x, x_exp)
    xq = engine.h2_to_f32(xh, x_exp).double()                  # what the cells hold (22 bits): the reference convolves THIS
    # float64 reference by im2col
    xp = torch.zeros((N, H + 2 * pad + stride, W + 2 * pad + stride, Cin), dtype=torch.float64, device="cuda")
    xp[:, pad:pad + H, pad:pad + W] = xq
    cols = [xp[:, a * rate: a * rate + (Ho - 1) * stride + 1: stride, b * rate: b * rate + (Wo - 1) * stride + 1: stride]
            for a in range(k) for b in range(k)]
    ref = torch.stack(cols, 3).reshape(N * Ho * Wo, k * k * Cin) @ torch.from_numpy(w.reshape(-1, Cout)).double().cuda()
    ref = ref.reshape(N, Ho, Wo, Cout) * torch.from_numpy(scale).double().cuda() + torch.from_numpy(bias).double().cuda()
    res = res_t = None
    res_exp, res_stride = 0, 0
    if res_kind in (1, 2):
        res = torch.randn((N, Ho, Wo, Cout), device="cuda", generator=g) * 2.0
        res_stride = 1
    elif res_kind == 3:
        res = torch.randn((N, 2 * Ho - 1, 2 * Wo, Cout), device="cuda", generator=g) * 2.0
        res_stride = 2
    if res is not None:
        if res_kind in (2, 3):
            res_exp = engine.h2_exp_for(float(res.abs().max()))
            res_t = engine.f32_to_h2(res, res_exp)
            rq = engine.h2_to_f32(res_t, res_exp).double()
        else:
            res_t, rq = res, res.double()
        ref = ref + (rq if res_stride == 1 else rq[:, ::2, ::2])
    ref = torch.relu(ref)
    y_exp = engine.h2_exp_for(float(ref.abs().max()))
    y, yrng = engine.conv2d_h2(xh, x_exp, w, stride=stride, rate=rate, pad_t=pad, pad_l=pad, out_hw=(Ho, Wo), scale=scale, bias=bias,
                               residual=res_t, res_stride=res_stride, res_is_h2=res_kind in (2, 3), res_exp=res_exp, relu=True,
                               y_is_h2=y_h2, y_exp=y_exp)
    out = engine.h2_to_f32(y, y_exp) if y_h2 else y
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err < 2e-5, (case, err)
    assert abs(float(yrng.max()) - float(ref.abs().max())) <= 1e-4 * float(ref.abs().max())      # tracked range = max |out|


def test_calibration_overflow_detection_and_recovery(lib_built):
    """Scales are calibrated by the first forward and frozen; a later batch whose activations outgrow them is flagged by the
    device-side range check, dgp_net_range_status reports it, and the next forward re-calibrates and is correct again."""
    from deepgraphpose_amd.engine import DGPNet
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    from oracle import dgp_oracle as O
    nj = 3
    wts = make_weights(50, nj, False, seed=31, head_std=0.05)
    net = DGPNet(50, nj, 64, 96, max_batch=4)
    net.load_weights(wts)
    flat = np.full((2, 64, 96, 3), 0, dtype=np.uint8)
    flat[..., 0], flat[..., 1], flat[..., 2] = 124, 117, 104             # ~ the mean pixel: centred input ~ 0 -> tiny activations
    frames = make_frames(2, 64, 96, nj, seed=31)
    raw = dict(check_range=False)                                         # the streaming contract: the caller polls range_status
    net.infer(torch.from_numpy(flat).cuda(), **raw)
    ov, ncal = net.range_status()
    assert not ov and ncal == 1
    mu_flat, _, _ = [t.clone() for t in net.infer(torch.from_numpy(flat).cuda(), **raw)]
    assert net.range_status() == (False, 1)                               # steady state: no re-calibration, no overflow
    net.infer(torch.from_numpy(frames).cuda(), **raw)                     # real frames on scales calibrated for ~zero input
    ov, ncal = net.range_status()
    assert ov and ncal == 1, "activations 16x beyond the calibrated range must be flagged"
    mu, conf, idx = [t.cpu().numpy() for t in net.infer(torch.from_numpy(frames).cuda(), **raw)]      # re-calibrates on this batch
    ov, ncal = net.range_status()
    assert not ov and ncal == 2
    ref = O.infer(frames, wts, 50)
    assert np.abs(mu - ref["mu"]).max() * 8.0 < 1e-3 and np.array_equal(idx, ref["idx"])
    # the wider scales still serve the small-activation batch (headroom costs no accuracy): same answer as before within 1e-3 px
    mu_flat2, _, _ = net.infer(torch.from_numpy(flat).cuda(), **raw)
    assert net.range_status() == (False, 2)
    assert float((mu_flat2 - mu_flat).abs().max()) * 8.0 < 1e-3
    # default calls (check_range=True) recover on their own: same sequence on a fresh engine, no polling by the caller
    net2 = DGPNet(50, nj, 64, 96, max_batch=4)
    net2.load_weights(wts)
    net2.infer(torch.from_numpy(flat).cuda())
    mu2, _, idx2 = [t.cpu().numpy() for t in net2.infer(torch.from_numpy(frames).cuda())]
    assert net2.range_status() == (False, 2)
    assert np.abs(mu2 - ref["mu"]).max() * 8.0 < 1e-3 and np.array_equal(idx2, ref["idx"])
    sc2 = net2.forward(torch.from_numpy(frames).cuda()).cpu().numpy()
    assert np.isfinite(sc2).all() and net2.range_status() == (False, 2)
    # widen(): what a rank does when ANOTHER rank of a sharded run overflowed -- re-calibration with 3 more bits of headroom
    net2.widen()
    mu3, _, idx3 = [t.cpu().numpy() for t in net2.infer(torch.from_numpy(frames).cuda())]
    assert net2.range_status() == (False, 3)
    assert np.abs(mu3 - ref["mu"]).max() * 8.0 < 1e-3 and np.array_equal(idx3, ref["idx"])


def test_h2_network_is_deterministic_and_close_to_fp32_activation_path(lib_built, tmp_path):
    """Same frames twice -> bit-identical outputs; and the H2 engine agrees with the DGP_H2=0 engine (fp32 activations, split in the
    K loop: the round-1 path) to fp32 round-off on the scoremap -- run in a child process because the switch is read once."""
    import os, subprocess, sys
    from deepgraphpose_amd.engine import DGPNet
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    nj = 4
    wts = make_weights(50, nj, False, seed=5, head_std=0.05)
    frames = make_frames(6, 96, 128, nj, seed=6)
    net = DGPNet(50, nj, 96, 128, max_batch=8)
    net.load_weights(wts)
    ft = torch.from_numpy(frames).cuda()
    a = net.forward(ft).clone()
    b = net.forward(ft).clone()
    assert torch.equal(a, b) and net.range_status() == (False, 1)
    np.save(tmp_path / "frames.npy", frames)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import numpy as np, torch, sys\n"
            "from deepgraphpose_amd.engine import DGPNet\n"
            "from deepgraphpose_amd.synthetic import make_weights\n"
            "net = DGPNet(50, 4, 96, 128, max_batch=8); net.load_weights(make_weights(50, 4, False, seed=5, head_std=0.05))\n"
            "sc = net.forward(torch.from_numpy(np.load(sys.argv[1])).cuda())\n"
            "assert net.range_status() == (False, 0)\n"
            "np.save(sys.argv[2], sc.cpu().numpy())\n")
    env = dict(os.environ, DGP_H2="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "frames.npy"), str(tmp_path / "sc.npy")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    sc32 = np.load(tmp_path / "sc.npy")
    assert np.abs(a.cpu().numpy() - sc32).max() <= 2e-5 * np.abs(sc32).max()


def test_reported_16_bit_tier_is_an_11_bit_version_of_the_same_network(lib_built, tmp_path):
    """DGP_CONV_MODE=f16 (bench.py's `tier_f16`): the H2 engine with ONE MFMA per product on the high fp16 cells in the 128-column conv
    kernels.  Not a parity tier -- the test pins what it is: the same network to 11-bit operand accuracy (scoremap within 2e-2 of its
    range, far outside the parity tier's 2e-5 and far inside "wrong"), the same arg-max cells but for near-ties, coordinates within 0.25 px."""
    import os, subprocess, sys
    from deepgraphpose_amd.engine import DGPNet
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    nj = 4
    wts = make_weights(50, nj, False, seed=5, head_std=0.05)
    frames = make_frames(6, 256, 320, nj, seed=6)              # 16 x 20 feature maps: the 128 x 128 kernels run from block2 on
    net = DGPNet(50, nj, 256, 320, max_batch=8)
    net.load_weights(wts)
    ft = torch.from_numpy(frames).cuda()
    a = net.forward(ft).cpu().numpy()
    mu_a, _, idx_a = net.infer(ft)
    np.save(tmp_path / "frames.npy", frames)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import numpy as np, torch, sys\n"
            "from deepgraphpose_amd.engine import DGPNet\n"
            "from deepgraphpose_amd.synthetic import make_weights\n"
            "net = DGPNet(50, 4, 256, 320, max_batch=8); net.load_weights(make_weights(50, 4, False, seed=5, head_std=0.05))\n"
            "ft = torch.from_numpy(np.load(sys.argv[1])).cuda()\n"
            "sc = net.forward(ft).cpu().numpy(); mu, _, idx = net.infer(ft)\n"
            "np.savez(sys.argv[2], sc=sc, mu=mu.cpu().numpy(), idx=idx.cpu().numpy())\n")
    env = dict(os.environ, DGP_CONV_MODE="f16", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "frames.npy"), str(tmp_path / "t16.npz")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    t = np.load(tmp_path / "t16.npz")
    rel = np.abs(a - t["sc"]).max() / np.abs(a).max()
    assert 2e-5 < rel < 2e-2, rel                               # the mode is active, and it is the same network
    # (window indices: an arg-max over 1-4 scoremap cells that may be nearly equal -- the tier's measured agreement is 99.6 % over 256 frames,
    #  one of the 24 pairs of this batch flips with the chain kernels on H1 tensors; the band of tests/test_h1_gpu.py)
    ia, it = idx_a.cpu().numpy(), t["idx"]
    same = (ia == it).all(-1)
    assert same.mean() >= 0.9
    # ... and a pair may flip ONLY at a near-tie: the parity scoremap's values at the two cells differ by no more than twice the distance
    # between the two tiers' scoremaps (everything with a clearer winner agrees exactly)
    noise = float(np.abs(a - t["sc"]).max())
    for b, j in zip(*np.nonzero(~same)):
        gap = abs(float(a[b, ia[b, j, 0], ia[b, j, 1], j]) - float(a[b, it[b, j, 0], it[b, j, 1], j]))
        assert gap <= 2.0 * noise, (int(b), int(j), gap, noise)
    assert np.abs(mu_a.cpu().numpy() - t["mu"]).max() * 8.0 < 0.25


def _cases_in_a_child(indices, halo_env):
    """the conv cases `indices` in a child pytest process under DGP_HALO = halo_env (read once per process).  Each case asserts there,
    through the plan query, the path the restated rules give it; here the path every case REPORTED is held to what the rules give for
    that switch on this device -- the two sides cannot drift apart.  -> {index: (mode, deep)}"""
    import os, subprocess, sys
    from deepgraphpose_amd import engine
    n_cu = engine.conv2d_plan((1, 1, 128, 64), (1, 1, 64, 128))["n_cu"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DGP_HALO=str(halo_env), PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_h2_gpu.py"), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_conv_on_h2_tensors_matches_float64 and (%s)" % " or ".join("case%d" % i for i in indices)], env=env, cwd=root,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "%d passed" % len(indices) in r.stdout and "skipped" not in r.stdout, r.stdout[-1500:] + r.stderr[-500:]
    paths = {i: _path_of(H2_CONV_CASES[i], n_cu, halo_env) for i in indices}
    for i, path in paths.items():
        print(_path_line(H2_CONV_CASES[i], path))
        assert _path_line(H2_CONV_CASES[i], path) in r.stdout, (i, path, r.stdout[-1500:])
    return paths, n_cu


def test_halo_walk_on_strips_longer_than_the_ring_in_a_child_process(lib_built):
    """DGP_HALO=2 lifts the default capacity bound: the walk also takes strips (128 + 2 d (W + 1) pixels) longer than the 360-pixel ring,
    which then slides inside a channel chunk -- where the launch is not on the deep ring and d (W - 2) + 128 <= 352.  Of the three
    cases, case15 misses the hard bound (360) on any chip; case17 (116 tiles) and case19 (26 tiles) walk the ring only on a chip with fewer
    CUs than that and run the deep ring with the per-tap loaders on a full-size one, as at the default.  The forced walk at full size:
    tests/test_halo_walk_gpu.py::test_sliding_ring_with_the_walk_forced."""
    paths, n_cu = _cases_in_a_child((15, 17, 19), 2)
    assert paths[15][0] == 1
    assert paths[17] == ((3, 0) if n_cu < 116 else (1, 1)) and paths[19] == ((3, 0) if n_cu < 26 else (1, 1))


def test_per_tap_loaders_of_the_3x3_layers_in_a_child_process(lib_built):
    """DGP_HALO=0: no launch walks the ring.  The batch-32 block4 conv2 (case10, 1200 tiles: the walk at the default) runs the
    three-stage per-tap LDS-DMA kernel (mode 1, deep 0) the 3x3 / stride-1 layers used before the walk became the default; the cases
    below one tile per CU run the deep per-tap kernel, as they do at the default."""
    paths, n_cu = _cases_in_a_child((4, 5, 10, 12, 13, 19), 0)
    assert all(mode == 1 for mode, _ in paths.values())
    assert paths[10] == ((1, 0) if n_cu < 1200 else (1, 1))


def test_extreme_frames_keep_parity(lib_built):
    """Frames far from the synthetic blobs the other tests use -- all black, all white, uniform noise, one saturated channel -- through
    the H2 engine (calibration on this very batch): finite outputs, no range overflow, coordinates within 1e-3 px of the oracle and
    bit-exact window indices."""
    from deepgraphpose_amd.engine import DGPNet
    from deepgraphpose_amd.synthetic import make_weights
    from oracle import dgp_oracle as O
    nj = 3
    wts = make_weights(50, nj, False, seed=41, head_std=0.05)
    rng = np.random.RandomState(3)
    fr = np.zeros((5, 64, 96, 3), dtype=np.uint8)
    fr[1] = 255
    fr[2] = rng.randint(0, 256, (64, 96, 3))
    fr[3, ..., 0] = 255
    fr[4, 20:40, 30:60] = rng.randint(0, 256, (20, 30, 3))
    net = DGPNet(50, nj, 64, 96, max_batch=8)
    net.load_weights(wts)
    mu, conf, idx = [t.cpu().numpy() for t in net.infer(torch.from_numpy(fr).cuda())]
    assert net.range_status()[0] is False
    assert np.isfinite(mu).all() and np.isfinite(conf).all()
    ref = O.infer(fr, wts, 50)
    assert np.abs(mu - ref["mu"]).max() * 8.0 < 1e-3, np.abs(mu - ref["mu"]).max() * 8.0
    assert np.array_equal(idx, ref["idx"])
    assert np.abs(conf - ref["likelihoods"]).max() < 1e-4


def _stress_case(hw, seed, B=2, nj=4):
    """Weights with trained-network BN statistics (synthetic.make_stress_weights) + frames; the head is rescaled so that the logits
    have a standard deviation of 3 on these frames (the backbone's output scale is not known in advance)."""
    from deepgraphpose_amd.synthetic import make_frames, make_stress_weights
    from oracle import dgp_oracle as O
    wts = make_stress_weights(50, nj, False, seed=seed)
    frames = make_frames(B, hw[0], hw[1], nj, seed=seed + 1)
    s_ref, _ = O.pose_heads(O.resnet_features(frames, wts, 50), wts, False)
    wts["pose/part_pred/block4/weights"] = (wts["pose/part_pred/block4/weights"] * np.float32(3.0 / s_ref.std())).astype(np.float32)
    return wts, frames


def _px_gate(err_oracle32_vs_fp64):
    """The round-4 criterion: a HIP tier may sit as far from the fp64 anchor as 1.5 x the CPU-fp32 oracle itself does, and never needs
    to be closer than the reference's 1e-3 px."""
    return max(1e-3, 1.5 * err_oracle32_vs_fp64)


@pytest.mark.parametrize("hw,seed", [((96, 128), 1), ((96, 128), 2), ((480, 640), 3), ((480, 640), 4), ((480, 640), 5), ((480, 640), 7)])
def test_trained_like_bn_statistics_keep_the_parity_gate(lib_built, hw, seed):
    """The H2 format on weights that look like a trained network: folded BN scales spread over 2^-8 .. 2^4 per layer, channel
    magnitudes over 2^-6 .. 2^2 with 100 x outliers, 5 % dead channels, weight-panel columns differing by up to 2^20.  Likelihood
    indices bit-exact, likelihoods within 1e-4, no range overflow after ONE calibration.
    Coordinates, anchored to FLOAT64 (oracle.infer(dtype=float64): the same graph and fp32 parameters in double precision).  In this
    regime the logits are broad (std 3 over the whole map), so the soft-argmax coordinate amplifies every rounding of the 50 layers
    in front of it: the CPU-fp32 oracle ITSELF is 0.8e-3 .. 5.7e-3 px from float64 at 640 x 480 (1.7e-4 at 96 x 128), i.e. two fp32
    evaluations of this network differ by more than the reference's 1e-3 px whatever computes them.  The gate is therefore relative:
    err_vs_fp64(HIP default) <= max(1e-3 px, 1.5 x err_vs_fp64(CPU-fp32 oracle)); and on the scoremap, where the error is not amplified,
    the engine must be at least as close to float64 as the fp32 oracle is (x 1.25).  Measured (scripts/stress_modes.py, seeds 3 / 4 / 5 /
    7): HIP default 6.3e-3 / 0.52e-3 / 0.55e-3 / 1.8e-3 px against the oracle's 5.7e-3 / 0.76e-3 / 2.6e-3 / 1.9e-3; scoremap 3.4 .. 6.5e-6
    relative against 5.2e-6 .. 1.26e-5."""
    from deepgraphpose_amd.engine import DGPNet
    from oracle import dgp_oracle as O
    wts, frames = _stress_case(hw, seed)
    ref = O.infer(frames, wts, 50, 8.0, 1.0, 1)
    r64 = O.infer(frames, wts, 50, 8.0, 1.0, 1, dtype=np.float64)
    assert np.isfinite(ref["scmap"]).all() and 1.0 < ref["scmap"].std() < 10.0
    net = DGPNet(50, 4, hw[0], hw[1], max_batch=frames.shape[0])
    net.load_weights(wts)
    sc = torch.empty((frames.shape[0], net.out_h, net.out_w, 4), device="cuda")
    mu, conf, idx = net.infer(torch.from_numpy(frames).cuda(), scmap_out=sc)
    assert net.range_status() == (False, 1)
    mu = mu.cpu().numpy().astype(np.float64)
    sc = sc.cpu().numpy().astype(np.float64)
    err_oracle = np.abs(ref["mu"] - r64["mu"]).max() * 8.0
    err_hip = np.abs(mu - r64["mu"]).max() * 8.0
    print("px vs fp64: HIP default %.3g, CPU-fp32 oracle %.3g; HIP vs oracle %.3g" % (err_hip, err_oracle, np.abs(mu - ref["mu"]).max() * 8.0))
    assert err_hip <= _px_gate(err_oracle), (err_hip, err_oracle)
    if hw == (96, 128):                      # well inside the reference's tolerance at the small size, against the fp32 oracle too
        assert np.abs(mu - ref["mu"]).max() * 8.0 < 1e-3
    s_scale = np.abs(r64["scmap"]).max()
    sc_hip, sc_oracle = np.abs(sc - r64["scmap"]).max() / s_scale, np.abs(ref["scmap"] - r64["scmap"]).max() / s_scale
    assert sc_hip <= max(1.25 * sc_oracle, 4e-6), (sc_hip, sc_oracle)
    assert np.array_equal(idx.cpu().numpy(), ref["idx"])
    assert np.array_equal(ref["idx"], r64["idx"])
    assert np.abs(conf.cpu().numpy() - ref["likelihoods"]).max() < 1e-4


def test_three_distances_from_the_fp64_anchor(lib_built, tmp_path):
    """The three numbers of the round-3 review at the headline shape (640 x 480, stress seed 3): |HIP default - fp64|,
    |HIP DGP_CONV_MODE=f32 - fp64| (IEEE-fp32 MFMA kernels, a child process: the mode is read once) and |CPU-fp32 oracle - fp64|.
    Both HIP tiers must meet the same relative gate; the fp16-split default must not be worse than the strict-fp32 tier by more
    than 2 x on the scoremap (measured: it is closer to float64 than the strict tier, 6.5e-6 against 1.2e-5)."""
    import os
    import subprocess
    import sys
    from deepgraphpose_amd.engine import DGPNet
    from oracle import dgp_oracle as O
    hw = (480, 640)
    wts, frames = _stress_case(hw, 3)
    ref = O.infer(frames, wts, 50, 8.0, 1.0, 1)
    r64 = O.infer(frames, wts, 50, 8.0, 1.0, 1, dtype=np.float64)
    np.savez(tmp_path / "case.npz", frames=frames, **wts)
    code = r"""
import sys, numpy as np, torch
from deepgraphpose_amd.engine import DGPNet
d = dict(np.load(sys.argv[1]))
frames = d.pop("frames")
net = DGPNet(50, 4, frames.shape[1], frames.shape[2], max_batch=frames.shape[0]); net.load_weights(d)
sc = torch.empty((frames.shape[0], net.out_h, net.out_w, 4), device="cuda")
mu, conf, idx = net.infer(torch.from_numpy(frames).cuda(), scmap_out=sc)
np.savez(sys.argv[2], mu=mu.cpu().numpy(), idx=idx.cpu().numpy(), sc=sc.cpu().numpy())
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for tier, env in (("default", {}), ("f32", {"DGP_CONV_MODE": "f32"})):
        subprocess.check_call([sys.executable, "-c", code, str(tmp_path / "case.npz"), str(tmp_path / (tier + ".npz"))],
                              env=dict(os.environ, PYTHONPATH=root, **env), cwd=root)
        out[tier] = np.load(tmp_path / (tier + ".npz"))
    err_oracle = np.abs(ref["mu"] - r64["mu"]).max() * 8.0
    errs = {t: np.abs(o["mu"].astype(np.float64) - r64["mu"]).max() * 8.0 for t, o in out.items()}
    scs = {t: np.abs(o["sc"].astype(np.float64) - r64["scmap"]).max() / np.abs(r64["scmap"]).max() for t, o in out.items()}
    print("px vs fp64: HIP default %.3g, HIP f32 %.3g, CPU-fp32 oracle %.3g; scoremap rel %.3g / %.3g" % (
        errs["default"], errs["f32"], err_oracle, scs["default"], scs["f32"]))
    for t in out:
        assert errs[t] <= _px_gate(err_oracle), (t, errs[t], err_oracle)
        assert np.array_equal(out[t]["idx"], r64["idx"])
    assert scs["default"] <= 2.0 * scs["f32"]


def test_trained_like_bn_statistics_on_fp32_activations(lib_built, tmp_path):
    """The same weights through DGP_H2=0 (fp32 activations, operands split in the K loop; ranges tracked per tensor, nothing
    calibrated) in a child process: same gate."""
    import os
    import subprocess
    import sys
    from oracle import dgp_oracle as O
    wts, frames = _stress_case((96, 128), 1)
    ref = O.infer(frames, wts, 50, 8.0, 1.0, 1)
    np.savez(tmp_path / "case.npz", frames=frames, **wts)
    code = r"""
import sys, numpy as np, torch
from deepgraphpose_amd.engine import DGPNet
d = dict(np.load(sys.argv[1]))
frames = d.pop("frames")
net = DGPNet(50, 4, frames.shape[1], frames.shape[2], max_batch=frames.shape[0]); net.load_weights(d)
mu, conf, idx = net.infer(torch.from_numpy(frames).cuda())
assert net.range_status()[1] == 0            # no H2 calibration happened: fp32 activations
np.savez(sys.argv[2], mu=mu.cpu().numpy(), idx=idx.cpu().numpy())
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DGP_H2="0", PYTHONPATH=root)
    subprocess.check_call([sys.executable, "-c", code, str(tmp_path / "case.npz"), str(tmp_path / "out.npz")], env=env, cwd=root)
    out = np.load(tmp_path / "out.npz")
    assert np.abs(out["mu"] - ref["mu"]).max() * 8.0 < 1e-3
    assert np.array_equal(out["idx"], ref["idx"])


def test_h2_residual_with_an_fp32_output_is_rejected(lib_built):
    """The fp32-output epilogue (the heads' pointwise GEMM) adds fp32 residuals only; with an H2 residual it used to read the cells as
    floats and return garbage (found by scripts/fuzz_conv_h2.py).  The combination is DGP_ERR_INVALID now; the fp32 residual still works."""
    from deepgraphpose_amd import _lib, engine
    rng = np.random.default_rng(3)
    x = torch.relu(torch.randn((2, 9, 11, 64), device="cuda"))
    res = torch.randn((2, 9, 11, 128), device="cuda")
    w = (rng.standard_normal((1, 1, 64, 128)) / 8.0).astype(np.float32)
    xe = engine.h2_exp_for(float(x.abs().max())); xh = engine.f32_to_h2(x, xe)
    re_ = engine.h2_exp_for(float(res.abs().max())); rh = engine.f32_to_h2(res, re_)
    with pytest.raises(_lib.DgpError, match="H2 residual needs an H2 output"):
        engine.conv2d_h2(xh, xe, w, residual=rh, res_stride=1, res_is_h2=True, res_exp=re_, y_is_h2=False)
    y, _ = engine.conv2d_h2(xh, xe, w, residual=res, res_stride=1, res_is_h2=False, y_is_h2=False)
    ref = torch.einsum("nhwc,co->nhwo", engine.h2_to_f32(xh, xe).double(), torch.from_numpy(w[0, 0]).double().cuda()) + res.double()
    assert float((y.double() - ref).abs().max() / ref.abs().max()) < 2e-5
