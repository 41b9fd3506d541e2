"""The case tables of tests/test_range_tracking_gpu.py, checked without a GPU: every case's plan (dgp_conv2d_plan for 256 CUs) is the path
the case is named after, the planted positions derived from it are where they should be, and THE PLANT DOMINATES: in the float64
reference, with the seeds the GPU test uses, the planted element is the maximum and everything else is at most a quarter of it.  So an
element an epilogue leaves out shows on the GPU as an error of at least 75 %, never as one inside the 1e-4 bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _range_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = RC.N_CU_CPU
_LAYERS = {}


def _plan(lib_built, name, tier):
    from deepgraphpose_amd import engine
    kw = RC.conv_plan_args(name, tier, N_CU)
    env = RC.CONV_CASES[name].get("env")
    if not env:
        return engine.conv2d_plan(n_cu=N_CU, **kw)
    code = "import json, sys; from deepgraphpose_amd import engine; print(json.dumps(engine.conv2d_plan(n_cu=%d, **json.loads(sys.argv[1]))))" % N_CU
    r = subprocess.run([sys.executable, "-c", code, json.dumps(kw)], env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _layer(name, tier):
    if (name, tier) not in _LAYERS:
        _LAYERS[(name, tier)] = RC.ConvLayer(name, tier, N_CU)
    return _LAYERS[(name, tier)]


@pytest.mark.parametrize("name,tier", RC.conv_case_ids())
def test_conv_case_takes_its_path_and_the_positions_follow_the_plan(lib_built, name, tier):
    pl = _plan(lib_built, name, tier)
    want = RC.conv_want(name, tier, N_CU)
    assert {k: pl[k] for k in want} == want, (pl, want)
    assert pl["grid"] == pl["n_main"] + (pl["mtiles"] * pl["ntiles"] - pl["n_main"]) * max(1, pl["tail_ksplit"]) or pl["family"] == 0, pl
    N, H, W = RC.conv_shape(RC.CONV_CASES[name]["shape"], N_CU)
    Ho, Wo = RC.out_hw(H, W, RC.CONV_CASES[name]["k"], RC.CONV_CASES[name].get("stride", 1), 1)
    M = N * Ho * Wo
    rows = RC.conv_rows(M, pl)
    assert M % RC.BM != 0 and RC.COUT % RC.BN != 0                            # padding in both directions
    assert rows["last"] == M - 1 and rows["ragged_first"] // RC.BM == pl["mtiles"] - 1 and rows["last_full_tile_last"] % RC.BM == RC.BM - 1
    assert rows["last_full_tile_last"] + 1 == rows["ragged_first"] <= rows["last"]
    if RC.CONV_CASES[name]["shape"] == "rounds":
        tile_of = lambda r: r // RC.BM * pl["ntiles"]                         # tiles in the row tiles in front of the row's
        assert pl["mtiles"] * pl["ntiles"] > 2 * N_CU                         # more tiles than workgroups resident at once
        assert tile_of(rows["high_row_tile"]) >= 2 * N_CU and rows["high_row_tile"] < M and 0 < rows["high_row_tile"] % RC.BM < RC.BM - 1
        if RC.CONV_CASES[name].get("slab"):
            assert tile_of(rows["tail_first"]) == pl["n_main"] and tile_of(rows["tail_first"] - 1) < pl["n_main"]
            assert rows["tail_first"] < rows["tail_middle"] < rows["tail_last"] == M - 1
    if RC.CONV_CASES[name]["shape"] == "walk":
        assert pl["grid"] > N_CU                                              # more than one tile per CU: not the deep ring
    cross = RC.conv_cross(M, pl)
    assert {c for _, _, c in cross} >= set(RC.conv_cols()) and {r for _, r, _ in cross} >= set(rows.values())
    assert len(cross) <= 2 * len(rows) + 2 * len(RC.conv_cols())


@pytest.mark.parametrize("name,tier", RC.conv_case_ids())
def test_conv_plant_dominates_at_every_position(lib_built, name, tier):
    pl = _plan(lib_built, name, tier)
    L = _layer(name, tier)
    assert float(L.x.max()) <= 15.0 and np.array_equal(L.x * 16, np.round(L.x * 16))          # exact in fp16 cells at any power-of-two scale
    worst = 0.0
    for label, m, c in RC.conv_cross(L.M, pl):
        ref, runner = L.planted(m, c)
        worst = max(worst, runner / ref)
        assert ref >= RC.DOMINANCE * runner and ref > 0.5 * RC.V, (label, m, c, ref, runner)
    print("%s %s: base max %.3g, worst runner-up %.3g of the plant" % (name, tier, L.ref_max(), worst))
    if L.wire is not None:                                                    # the wire reaches one output pixel: the centre tap of m
        n, h, w = L.wire_pixel(L.M - 1)
        assert (n, h, w) == (L.N - 1, (L.Ho - 1) * L.stride, (L.Wo - 1) * L.stride) and h < L.H and w < L.W
        assert not L.x[..., L.wire].any() and not L.w[:, :, L.wire].any() and L.w_for(7)[L.k // 2, L.k // 2, L.wire, 7] == 1.0


@pytest.mark.parametrize("name,tier", RC.pad_case_ids())
def test_conv_padding_case_keeps_every_real_output_below_the_bias(name, tier):
    L = RC.ConvLayer(name, tier, N_CU, mode="padding")
    top = L.ref_max()
    print("%s: B %.3g, max real output %.3g" % (name, L.B, top))
    assert 0.05 * L.B < top <= 0.8 * L.B                                      # a counted padded row (relu(B) = B) is an error of >= 25 %
    Z = RC.ConvLayer(name, tier, N_CU, mode="zero")
    assert Z.ref_max() == 0.0 and Z.B < 0


def _fused_cases():
    out = [("chain", inst, "small") for inst in RC.CHAIN_INSTANCES] + [("chain", inst, "big") for inst in RC.CHAIN_BIG]
    out += [("unit", (64, 64) + inst, m) for inst in RC.UNIT_INSTANCES for m in list(RC.UNIT_MAPS) + ["big"]]
    return out


fused_layer = RC.fused_layer


@pytest.mark.parametrize("kind,inst,size", _fused_cases())
def test_fused_kernel_plant_dominates_and_the_wires_are_clean(kind, inst, size):
    L = fused_layer(kind, inst, size, N_CU)
    tops = L.base_max()
    print("%s %s %s: base maxima R2 %.3g X' %.3g R1' %.3g" % (kind, inst, size, *tops))
    assert all(RC.DOMINANCE * t <= RC.V for t in tops), tops
    r2, x, r1 = L.outputs()
    assert not x[:, L.J0].any() and not r1[:, L.C0].any() and (r2 is None or not r2[:, L.K0].any())      # a wire carries the plant and nothing else
    f = lambda a: a.astype(np.float64)
    assert f(L.w3)[:, L.J0].sum() == (2.0 if L.res_mode == 0 else 1.0) and f(L.w1)[:, L.C0].sum() == 1.0 and L.b3[L.J0] == 0 and L.b1[L.C0] == 0 and L.s1[L.C0] == 1
    if kind == "chain":
        px = RC.chain_pixels(L.N, L.H, L.W, size == "big", N_CU)
        F = L.H * L.W
        if size == "small":
            assert F % 16 != 0 and px["frame_seam_a"] // 16 == px["frame_seam_b"] // 16           # the frame seam lies inside a row block
            assert px["row_block_15"] // 16 != px["row_block_16"] // 16
        else:
            assert px["second_round"] // max(RC.CHAIN_TILES) >= RC.MAX_WGS_PER_CU * N_CU and px["second_round"] < px["later_round"] < L.M
            assert px["later_round"] // max(RC.CHAIN_TILES) >= 2 * RC.MAX_WGS_PER_CU * N_CU
    else:
        px = RC.unit_pixels(L.N, L.H, L.W)
        ys, xs = {p[1] for p in px.values()}, {p[2] for p in px.values()}
        assert ys >= {0, L.H - 1} and xs >= {0, L.W - 1} and {p[0] for p in px.values()} == {0, L.N - 1}
        if size != "narrow":
            assert ys >= {RC.UNIT_TH - 1, RC.UNIT_TH} and xs >= {RC.UNIT_TW - 1, RC.UNIT_TW} and L.H % RC.UNIT_TH != 0 and L.W % RC.UNIT_TW != 0
        else:
            assert L.W < RC.UNIT_TW and L.H < RC.UNIT_TH
        if size == "big":                                                         # the last frame's tiles come after 8 n_cu others
            assert (L.N - 1) * -(-L.H // RC.UNIT_TH) * -(-L.W // RC.UNIT_TW) >= RC.BIG_TILES_PER_CU * N_CU > 2 * RC.MAX_WGS_PER_CU * N_CU


@pytest.mark.parametrize("kind,inst", [("chain", (64, 64, 0, 1)), ("chain", (64, 64, 64, 0)), ("unit", (64, 64, 0, 1)), ("unit", (64, 64, 64, 0))])
def test_fused_padding_case_has_positive_maxima(kind, inst):
    L = fused_layer(kind, inst, "small" if kind == "chain" else "ragged", N_CU, mode="padding")
    r2, x, r1 = L.outputs()
    print("%s %s: maxima R2 %s X' %.3g (B %.3g) R1' %.3g (B %.3g)" % (kind, inst, None if r2 is None else "%.3g" % r2.max(), x.max(), L.b3[0], r1.max(), L.b1[0]))
    # a counted padded pixel reports B: at least 10 % above the real maximum of R2 and X'.  R1' is not guarded in this direction: a padded
    # pixel's X' is B3, so its R1' = relu(B1 - |w1| . B3) is below the real maxima, and a real pixel whose X' is all zero reports B1 itself
    assert 0 < x.max() <= 0.9 * L.b3[0] and 0 < r1.max() <= L.b1[0] and (r2 is None or 0 < r2.max() <= 0.9 * L.b2[0])
    Z = fused_layer(kind, inst, "small" if kind == "chain" else "ragged", N_CU, mode="zero")
    assert all(o is None or o.max() == 0.0 for o in Z.outputs())


@pytest.mark.parametrize("frame", RC.ROOT_FRAMES)
def test_root_block_patches_sit_around_one_pool_cell_each(frame):
    H, W = frame
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    HP, pt = RC.pool_geometry(H1)
    WP, pl = RC.pool_geometry(W1)
    for name, (b, qy, qx) in RC.root_targets(H, W).items():
        y0, y1, x0, x1, (y, x) = RC.root_patch(H, W, qy, qx)
        assert 0 <= qy < HP and 0 <= qx < WP and 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W and 2 <= y1 - y0 <= 3 and 2 <= x1 - x0 <= 3
        cells_y = [q for q in range(HP) if 2 * q - pt <= y <= 2 * q - pt + 2]
        cells_x = [q for q in range(WP) if 2 * q - pl <= x <= 2 * q - pl + 2]
        assert cells_y == [qy] and cells_x == [qx], (name, cells_y, cells_x)


@pytest.mark.parametrize("cells", ["h2", "h1"])
@pytest.mark.parametrize("frame", RC.ROOT_FRAMES)
def test_root_block_plant_dominates_in_its_pool_cell(frame, cells):
    """float64 on the cells the kernel holds, on the CPU: the pool maximum lies in the targeted cell, every other cell is at most a quarter"""
    H, W = frame
    wts = RC.root_weights()
    for name, target in RC.root_targets(H, W).items():
        ref, runner, hit = RC.root_dominance(RC.root_reference(RC.root_frames(H, W, target), wts, cells), target)
        print("root %s %s %s: maximum %.6g, runner-up %.3g of it" % (frame, cells, name, ref, runner / ref))
        assert hit and RC.DOMINANCE * runner <= ref and ref > 50, (name, ref, runner, hit)


@pytest.mark.parametrize("cells", ["h2", "h1"])
@pytest.mark.parametrize("frame", RC.ROOT_FRAMES)
def test_root_block_padding_case_keeps_every_real_output_below_the_bias(frame, cells):
    H, W = frame
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    HP, WP = RC.pool_geometry(H1)[0], RC.pool_geometry(W1)[0]
    # ragged against the kernel's tiles of 5 (H2 cells) or 3 (H1 cells) pool rows x 16 pool columns (launch_root_block, csrc/dgp_ops.hip)
    assert WP % 16 and HP % 5 and (HP % 3 or (H, W) == RC.ROOT_FRAMES[0])
    top = float(RC.root_reference(RC.root_frames(H, W, bright=True), RC.root_weights("padding"), cells).max())
    print("root %s %s: B %.3g, max real output %.6g" % (frame, cells, RC.ROOT_B, top))
    assert 0.05 * RC.ROOT_B < top <= 0.9 * RC.ROOT_B                              # a counted element outside the map (relu(B) = B): an error of >= 11 %
    assert float(RC.root_reference(RC.root_frames(H, W, bright=True), RC.root_weights("zero"), cells).max()) == 0.0
