"""The two compute-wave layouts of the cell-input conv kernels on 128 x 128 tiles (conv_igemm_split_ls, csrc/dgp_conv_split.hip): 2 x 2 waves
of 64 x 64 (DGP_WAVE_2X2=1, the default) and 4 x 1 waves of 32 x 128 (=0).  Both accumulate the same products in the same order, so
every output must be the same BITS; and the 2 x 2 result must agree with float64.

The switch is read once per process, so each layout runs ONCE in a child process (this file as a script) that runs every case through
the layer entry points (engine.conv2d_h2 / conv2d_h1) into a NaN-filled output, compares with a float64 reference (im2col + matmul on
the device, of the values the cells hold; H1: weights rounded to fp16 on the panel's scale), records the plan (engine.conv2d_plan) and
dumps the raw output bytes.  The tests read the two records: per case the plan reports the forced layout and the expected walk, the bytes
are equal, no NaN is left, the error is inside the bound and the tracked range is max |y| within 1e-4.

Shapes.  The "narrow" cases are the smallest at which the loop can go wrong (one and two K-steps, a 2-row last tile, a half-empty
column tile, frame wrap inside a wave's 64 rows).  Their grids have at most one tile per CU, where H2 launches with >= 6 K-steps take the
deep ring (per-tap loaders, never the halo walk).  So that the 80-KB kernels and the halo walk also run on H2, the "wide" cases keep the
pixels and choose Cout from the device's CU count so that the grid has more than one tile per CU; the plan query asserts which walk a
case took.

Bounds are the project's own: H2 2e-5 of max |ref| (EXPERIMENTS.md section D); the 16-bit tier writes fp16 cells and reads 11-bit
operands, so ITS cases are held to the per-element bound of tests/test_h1_gpu.py, 2^-11 |ref| (1 + 1e-3) + 2^-24 2^-y_exp + 4e-6 max |ref|
(an H1 output cannot be closer than half an fp16 ulp to anything); fp32 outputs of H1 inputs to 2e-5 like H2.

One more pair of child processes runs TAIL_CASES under DGP_TAIL_SPLIT=2: the K-split tail's raw slab store from the 2 x 2 layout's
64-row staging, against float64 and against the 4 x 1 layout's bits."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# epilogue variants: (scale, bias, residual (None / "cells" / "f32"), relu)
EPI = {"plain": (False, False, None, False), "affine": (True, True, None, False), "relu": (True, True, None, True),
       "res_cells": (True, True, "cells", True), "res_f32": (True, True, "f32", False)}


def _cases():
    """name -> dict(tier, N, H, W, cin, cout (int, or "wide"), k, stride, d, epi, y_cells, mode: the walk the plan must report (None: any))"""
    c = {}
    epis = list(EPI)
    n = 0
    for M in (130, 128 + 64 + 1):
        for K in (32, 64, 256):
            for cout in (128, 192):
                # narrow grids: K = 256 is 8 K-steps -> the deep ring; K = 32 / 64 the 80-KB kernel
                c["pw_m%d_k%d_n%d" % (M, K, cout)] = dict(tier="h2", N=1, H=1, W=M, cin=K, cout=cout, k=1, stride=1, d=1, epi=epis[n % len(epis)],
                                                          y_cells=True, mode=2, deep=int(K == 256))
                n += 1
    for e in epis:                                                      # every epilogue variant on one shape
        c["pw_epi_" + e] = dict(tier="h2", N=1, H=1, W=193, cin=64, cout=192, k=1, stride=1, d=1, epi=e, y_cells=True, mode=2, deep=0)
    c["pw_wide_k256"] = dict(tier="h2", N=1, H=1, W=130, cin=256, cout="wide", k=1, stride=1, d=1, epi="res_cells", y_cells=True, mode=2, deep=0)
    c["pw_f32out"] = dict(tier="h2", N=1, H=1, W=193, cin=64, cout=192, k=1, stride=1, d=1, epi="res_f32", y_cells=False, mode=2, deep=0)
    for cin in (32, 64):                                                # per-tap 3 x 3, stride 2, two frames
        for H, W in ((9, 11), (30, 40)):
            c["tap_s2_%dx%d_c%d" % (H, W, cin)] = dict(tier="h2", N=2, H=H, W=W, cin=cin, cout=128, k=3, stride=2, d=1, epi="relu", y_cells=True,
                                                       mode=1, deep=1)
    c["tap_s2_wide"] = dict(tier="h2", N=2, H=30, W=40, cin=32, cout="wide", k=3, stride=2, d=1, epi="res_cells", y_cells=True, mode=1, deep=0)
    for d in (1, 2):                                                    # halo walk: 3 x 3, stride 1, 30 x 40, 1 - 3 frames
        for N in (1, 2, 3):
            for cin in (32, 64):
                c["halo_d%d_n%d_c%d" % (d, N, cin)] = dict(tier="h2", N=N, H=30, W=40, cin=cin, cout="wide", k=3, stride=1, d=d,
                                                           epi=("relu", "res_cells", "res_f32")[N - 1], y_cells=True, mode=3, deep=0)
    c["halo_narrow"] = dict(tier="h2", N=1, H=30, W=40, cin=64, cout=128, k=3, stride=1, d=1, epi="relu", y_cells=True, mode=1, deep=1)
    # 16-bit tier (never the deep ring)
    c["h1_pw_k64"] = dict(tier="h1", N=1, H=1, W=193, cin=64, cout=192, k=1, stride=1, d=1, epi="res_cells", y_cells=True, mode=2, deep=0)
    c["h1_pw_f32out"] = dict(tier="h1", N=1, H=1, W=193, cin=64, cout=192, k=1, stride=1, d=1, epi="affine", y_cells=False, mode=2, deep=0)
    c["h1_halo_d2"] = dict(tier="h1", N=2, H=30, W=40, cin=64, cout=128, k=3, stride=1, d=2, epi="res_cells", y_cells=True, mode=3, deep=0)
    return c


CASES = _cases()

# The K-split of the grid's tail on cell inputs (forced: DGP_TAIL_SPLIT=2, its own pair of child processes): the tail slices leave
# the wave tiles through ls_store_raw, which reads the 64-row staging of the 2 x 2 layout.  Row tiles from the CU count so that the
# grid is one full round of two workgroups per CU plus at most 16 tiles; K = 256 is 8 K-steps, which the rule splits two ways
# (parts of fewer than 4 K-steps are refused).  The output is 34 MB at 256 CUs, so the children hand back its SHA-256, not its bytes.
TAIL_CASES = {"pw_tail_split": dict(tier="h2", N=1, H=1, W="tail", cin=256, cout=1024, k=1, stride=1, d=1, epi="res_cells", y_cells=True,
                                    mode=2, deep=0, slab_floats=16 * 2 * 128 * 128)}


# ---------------------------------------------------------------- the child: one layout, every case
def _w_exp(w):
    return 14 - (math.frexp(float(np.abs(w).max()))[1] - 1)


def _conv_f64(torch, xq, wq, stride, d, pad):
    """float64 conv as im2col + matmul, one tap's columns at a time: xq [N,H,W,Cin], wq [k,k,Cin,Cout] (device, float64)"""
    N, H, W, Cin = xq.shape
    k = wq.shape[0]
    Ho, Wo = (H + 2 * pad - (k - 1) * d - 1) // stride + 1, (W + 2 * pad - (k - 1) * d - 1) // stride + 1
    xp = torch.zeros((N, H + 2 * pad, W + 2 * pad, Cin), dtype=torch.float64, device="cuda")
    xp[:, pad:pad + H, pad:pad + W] = xq
    acc = torch.zeros((N * Ho * Wo, wq.shape[3]), dtype=torch.float64, device="cuda")
    for a in range(k):
        for b in range(k):
            cols = xp[:, a * d:a * d + (Ho - 1) * stride + 1:stride, b * d:b * d + (Wo - 1) * stride + 1:stride]
            acc += cols.reshape(N * Ho * Wo, Cin) @ wq[a, b]
    return acc.reshape(N, Ho, Wo, -1)


def _run_case(torch, eng, name, c, n_cu, seed):
    h1 = c["tier"] == "h1"
    fmt = 2 if h1 else 1
    N, H, W, cin, k, s, d = c["N"], c["H"], c["W"], c["cin"], c["k"], c["stride"], c["d"]
    if W == "tail":                                                                  # one round of 2 n_cu tiles and a tail of 9 .. 16
        W = 128 * ((2 * n_cu) // 8 + 1) + 2
    pad = d if k == 3 else 0
    Ho, Wo = (H + 2 * pad - (k - 1) * d - 1) // s + 1, (W + 2 * pad - (k - 1) * d - 1) // s + 1
    mtiles = -(-N * Ho * Wo // 128)
    cout = c["cout"] if c["cout"] != "wide" else 128 * (n_cu // mtiles + 1)          # more than one tile per CU
    use_scale, use_bias, res, relu = EPI[c["epi"]]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    x = torch.relu(torch.randn((N, H, W, cin), device="cuda", generator=g)) * 3.0
    w = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    scale = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32) if use_scale else None
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32) if use_bias else None
    ycells = c["y_cells"]
    slab = torch.full((c["slab_floats"],), NAN, device="cuda") if c.get("slab_floats") else None
    pl = eng.conv2d_plan((N, H, W, cin), w.shape, stride=s, rate=d, pad_t=pad, pad_l=pad, in_fmt=fmt, out_fmt=fmt if ycells else 0,
                         res_fmt=fmt if res == "cells" else 0, res_stride=1 if res else 0, res_hw=(Ho, Wo) if res else (0, 0), slab_bytes=4 * c.get("slab_floats", 0))
    x_exp = eng.h2_exp_for(float(x.abs().max()))
    if h1:
        xh = eng.f32_to_h1(x, x_exp); xq = eng.h1_to_f32(xh, x_exp).double()
        wt = torch.from_numpy(w).cuda()
        wq = (wt * 2.0 ** _w_exp(w)).to(torch.float16).double() * 2.0 ** -_w_exp(w)
    else:
        xh = eng.f32_to_h2(x, x_exp); xq = eng.h2_to_f32(xh, x_exp).double()
        wq = torch.from_numpy(w).cuda().double()
    ref = _conv_f64(torch, xq, wq, s, d, pad)
    if scale is not None:
        ref = ref * torch.from_numpy(scale).double().cuda()
    if bias is not None:
        ref = ref + torch.from_numpy(bias).double().cuda()
    res_t, res_exp = None, 0
    if res:
        r = torch.randn((N, Ho, Wo, cout), device="cuda", generator=g) * 2.0
        if res == "cells":
            res_exp = eng.h2_exp_for(float(r.abs().max()))
            if h1:
                res_t = eng.f32_to_h1(r, res_exp); rq = eng.h1_to_f32(res_t, res_exp).double()
            else:
                res_t = eng.f32_to_h2(r, res_exp); rq = eng.h2_to_f32(res_t, res_exp).double()
        else:
            res_t, rq = r, r.double()
        ref = ref + rq
    if relu:
        ref = torch.relu(ref)
    mx = float(ref.abs().max())
    y_exp = eng.h2_exp_for(mx)
    kw = dict(stride=s, rate=d, pad_t=pad, pad_l=pad, out_hw=(Ho, Wo), scale=scale, bias=bias, residual=res_t, res_stride=1 if res else 0,
              res_exp=res_exp, relu=relu, y_exp=y_exp)
    y = torch.full((N, Ho, Wo, cout), NAN, device="cuda", dtype=torch.float16 if (h1 and ycells) else torch.float32)
    if h1:
        y2, yr = eng.conv2d_h1(xh, x_exp, w, y_is_h1=ycells, out=y, **kw)
        out = eng.h1_to_f32(y, y_exp).double() if ycells else y.double()
    else:
        y2, yr = eng.conv2d_h2(xh, x_exp, w, y_is_h2=ycells, res_is_h2=res == "cells", tail_slab=slab, out=y, **kw)
        out = eng.h2_to_f32(y, y_exp).double() if ycells else y.double()
    assert y2 is y
    if h1 and ycells:
        tol = 2.0 ** -11 * ref.abs() * (1 + 1e-3) + 2.0 ** -24 * 2.0 ** -y_exp + 4e-6 * mx
    else:
        tol = torch.full_like(ref, 2e-5 * mx)
    diff = (out - ref).abs()
    raw = y.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)
    rec = dict(plan={k_: pl[k_] for k_ in ("tile", "mode", "deep", "w22", "h1", "ah2", "oh2", "dma", "grid", "n_cu", "tail_ksplit")},
               sha=hashlib.sha256(raw.tobytes()).hexdigest(), nan=int(torch.isnan(out).sum()), err=float(diff.nan_to_num(float("inf")).max() / mx),
               worst=float((diff / tol).nan_to_num(float("inf")).max()), range_err=abs(float(yr.max()) - mx) / mx, cout=int(cout))
    print("[wave-tile] %-22s w22 %d mode %d deep %d grid %4d: err %.3g of max |ref|, %.3g of the bound, range %.2g"
          % (name, pl["w22"], pl["mode"], pl["deep"], pl["grid"], rec["err"], rec["worst"], rec["range_err"]), flush=True)
    return rec, raw


def _run_network(torch, eng):
    """the smallest network the suite builds (smoke's: ResNet-50, 4 joints, 96 x 128 frames, batch 2), both tiers: scoremaps and read-outs"""
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    wts = make_weights(50, 4, False, seed=1, head_std=0.05)
    ft = torch.from_numpy(make_frames(2, 96, 128, 4, seed=2)).cuda()
    out = {}
    for tier in ("parity", "f16"):
        net = eng.DGPNet(50, 4, 96, 128, max_batch=2, device=0, tier=tier)
        net.load_weights(wts)
        sc = net.forward(ft).clone()
        mu, conf, idx = net.infer(ft, 1.0, 1)
        for n_, t in (("sc", sc), ("mu", mu), ("conf", conf), ("idx", idx)):
            out["net_%s_%s" % (tier, n_)] = t.contiguous().cpu().numpy()
    return out


def _child(path, tail):
    import torch
    from deepgraphpose_amd import engine as eng
    n_cu = eng.conv2d_plan((1, 1, 128, 64), (1, 1, 64, 128))["n_cu"]
    recs, arrays = {}, {}
    if tail:                                                            # (DGP_TAIL_SPLIT=2 in the environment)
        for i, (name, c) in enumerate(TAIL_CASES.items()):
            recs[name], _ = _run_case(torch, eng, name, c, n_cu, 2000 + i)
    else:
        for i, (name, c) in enumerate(CASES.items()):
            recs[name], arrays[name] = _run_case(torch, eng, name, c, n_cu, 1000 + i)
        arrays.update(_run_network(torch, eng))
        np.savez(path + ".npz", **arrays)
    with open(path + ".json", "w") as f:
        json.dump(recs, f)


if __name__ == "__main__":
    _child(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "tail")
    sys.exit(0)


# ---------------------------------------------------------------- the tests: read the two records
def _spawn(path, w22, tail):
    env = dict(os.environ, DGP_WAVE_2X2=str(w22), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    if tail:
        env["DGP_TAIL_SPLIT"] = "2"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path] + (["tail"] if tail else []), env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("[wave-tile]")))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(path + ".json") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(lib_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("wave_tile")
    out = {}
    for w22 in (0, 1):
        path = str(d / ("w22_%d" % w22))
        out[w22] = (_spawn(path, w22, False), np.load(path + ".npz"))
    return out


@pytest.fixture(scope="module")
def tail_runs(lib_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("wave_tile_tail")
    return {w22: _spawn(str(d / ("w22_%d" % w22)), w22, True) for w22 in (0, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_layouts_give_the_same_bits_and_agree_with_float64(runs, name):
    c = CASES[name]
    for w22 in (0, 1):
        rec = runs[w22][0][name]
        pl = rec["plan"]
        want = dict(tile=16, w22=w22, mode=c["mode"], deep=c["deep"], h1=int(c["tier"] == "h1"), ah2=1, oh2=int(c["y_cells"]), dma=1, tail_ksplit=0)
        assert {k: pl[k] for k in want} == want, (name, w22, pl)
        if c["cout"] == "wide":
            assert pl["grid"] > pl["n_cu"], (name, pl)
        assert rec["nan"] == 0, (name, w22, rec)
        assert rec["worst"] <= 1.0, (name, w22, rec)                    # float64, inside the tier's bound (both layouts: same bits)
        assert rec["range_err"] <= 1e-4, (name, w22, rec)
    a, b = runs[0][1][name], runs[1][1][name]
    assert a.shape == b.shape and np.array_equal(a, b), (name, int((a != b).sum()))


@pytest.mark.parametrize("tier", ["parity", "f16"])
def test_network_outputs_are_the_same_bits(runs, tier):
    for n in ("sc", "mu", "conf", "idx"):
        a, b = runs[0][1]["net_%s_%s" % (tier, n)], runs[1][1]["net_%s_%s" % (tier, n)]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tier, n)


@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_split_tail_slices_leave_both_layouts_the_same_way(tail_runs, name):
    """the raw slab store of a K-split tail (DGP_TAIL_SPLIT=2 on cell inputs) from the 64-row staging: split two ways on both layouts,
    no NaN left in the output (the slab was NaN-filled), float64 within 2e-5 of max |ref|, the same bits"""
    c = TAIL_CASES[name]
    for w22 in (0, 1):
        rec = tail_runs[w22][name]
        pl = rec["plan"]
        want = dict(tile=16, w22=w22, mode=c["mode"], deep=0, h1=0, ah2=1, oh2=1, dma=1, tail_ksplit=2)
        assert {k: pl[k] for k in want} == want, (name, w22, pl)
        assert pl["grid"] > 2 * pl["n_cu"], (name, pl)
        assert rec["nan"] == 0, (name, w22, rec)
        assert rec["worst"] <= 1.0, (name, w22, rec)
        assert rec["range_err"] <= 1e-4, (name, w22, rec)
    assert tail_runs[0][name]["sha"] == tail_runs[1][name]["sha"], name
