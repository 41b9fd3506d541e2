"""The tracked ranges: "the maximum of a tensor's ABSMAX_SLOTS floats is the maximum of |y| over every real element and of nothing else",
for the epilogues of the conv kernels (fp32, split, cell inputs, the K-split tail's fix-up kernels), the chain and unit kernels (R2, X',
R1', with X' stores dropped by xout_keep = 2) and the root block.

Method (tests/_range_cases.py has the tables, the references and the reasoning; tests/test_range_cases_cpu.py checks them without a GPU):
one planted extreme per launch that dominates every other element by a factor of four, moved over the places where ownership of output
elements changes hands -- derived from the launch's own plan (engine.conv2d_plan), which every case also asserts the path it is named
after.  After each launch:

    |max(slots) - ref_max| <= 1e-4 ref_max          ref_max from float64; 1e-4 is the project's bound for a range tracked in fp32
                                                    before the cell rounding (tests/test_h2_gpu.py)
    max(slots) == max |y| bit for bit               fp32 outputs (tests/test_conv_plan_gpu.py)

The opposite direction: x > 0, w < 0, bias B > 0 on every channel and ReLU -- a padded row or pixel that were counted would report
relu(B) = B, above every real output; with B < 0 every output is 0 and the slots must hold exactly 0.0.  And infinity: +inf (-inf without
ReLU) in an fp32 residual must arrive in the slots, which is what makes h2_range_check_kernel's !(x < 60000) fire.

Switches read once per process (DGP_WAVE_2X2=0: the 4 x 1 wave layout; DGP_TAIL_SPLIT=2: the K-split tail on cell inputs) run their
cases in child pytest processes.  Measured: EXPERIMENTS.md, "Tracked ranges with planted extremes"."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _range_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, TOL = RC.V, RC.TOL
INF = float("inf")


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    return engine


@pytest.fixture(scope="module")
def n_cu(eng):
    return eng.conv2d_plan((1, 1, 128, 64), (1, 1, 64, 128))["n_cu"]


def _close(got, ref, what):
    print("[range] %s: slots %.9g, float64 %.9g" % (what, got, ref))
    assert abs(got - ref) <= TOL * ref, (what, got, ref)


def _respawn(request, **env):
    """Switches read once per process: True in a process that has them (the body runs); otherwise the test runs again in a child pytest
    process with them, must pass there, and the body returns at once"""
    if all(os.environ.get(k) == v for k, v in env.items()):
        return True
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-rA", "-m", "gpu", "-p", "no:cacheprovider"], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    return False


# ------------------------------------------------------------------------------------------------------------------ conv layers
class DevConv:
    """one conv case on the device: operands uploaded once, one launch per plant"""

    def __init__(self, eng, L, n_cu, w22=None):
        self.eng, self.L = eng, L
        c = L.c
        self.pl = eng.conv2d_plan(**RC.conv_plan_args(L.name, L.tier, n_cu, with_res=L.res is not None))
        want = RC.conv_want(L.name, L.tier, n_cu)
        if w22 is not None and c["entry"] == "cells":
            want["w22"] = w22
        assert {k: self.pl[k] for k in want} == want, (L.name, L.tier, self.pl, want)
        self.x = torch.from_numpy(L.x).cuda()
        self.cells = L.tier != "f32"
        self.ycells = bool(c.get("ycells")) and self.cells
        self.y = torch.empty((L.N, L.Ho, L.Wo, RC.COUT), device="cuda", dtype=torch.float16 if (self.ycells and L.tier == "h1") else torch.float32)
        self.slab = torch.zeros(RC.SLAB_FLOATS, device="cuda") if c.get("slab") else None
        self.res = None
        if L.res:
            shape = (L.N, 2 * L.Ho - 1, 2 * L.Wo, RC.COUT) if L.res == "cells2" else (L.N, L.Ho, L.Wo, RC.COUT)
            self.res = torch.zeros(shape, device="cuda")
        self.xq = None

    def _to_cells(self, t, e):
        if self.L.tier == "h1":
            c = self.eng.f32_to_h1(t, e)
            return c, self.eng.h1_to_f32(c, e)
        c = self.eng.f32_to_h2(t, e)
        return c, self.eng.h2_to_f32(c, e)

    def launch(self, w, ref_max, x=None, res_value=None):
        """-> (max of the slots, max |y| of an fp32 output or None)"""
        eng, L = self.eng, self.L
        k, pad = L.k, (L.k - 1) // 2
        kw = dict(stride=L.stride, pad_t=pad, pad_l=pad, out_hw=(L.Ho, L.Wo), scale=L.scale, bias=L.bias, relu=L.relu, out=self.y)
        res_t, res_exp = None, 0
        if self.res is not None:
            kw["res_stride"] = 2 if L.res == "cells2" else 1
            res_t = self.res
            if L.res.startswith("cells"):
                res_exp = eng.h2_exp_for(V)
                res_t, rq = self._to_cells(self.res, res_exp)
                assert torch.equal(rq, self.res)
        if not self.cells:
            y, slots = eng.conv2d(self.x if x is None else x, w, residual=res_t, ranged=L.c["ranged"], return_range=True, tail_slab=self.slab, **kw)
        else:
            if x is not None or self.xq is None:
                src = self.x if x is None else x
                x_exp = eng.h2_exp_for(float(src.abs().max()))
                xh, xq = self._to_cells(src, x_exp)
                assert torch.equal(xq, src)                                  # the cells hold the operands exactly
                if x is None:
                    self.xq = (xh, x_exp)
            else:
                xh, x_exp = self.xq
            y_exp = eng.h2_exp_for(ref_max) if ref_max > 0 and ref_max < INF else 0
            if L.tier == "h1":
                y, slots = eng.conv2d_h1(xh, x_exp, w, residual=res_t, res_exp=res_exp, y_is_h1=self.ycells, y_exp=y_exp, **kw)
            else:
                y, slots = eng.conv2d_h2(xh, x_exp, w, residual=res_t, res_is_h2=bool(L.res and L.res.startswith("cells")), res_exp=res_exp,
                                         y_is_h2=self.ycells, y_exp=y_exp, tail_slab=self.slab, **kw)
        assert y is self.y
        return float(slots.max()), (None if self.ycells else float(y.abs().max()))

    def plant(self, m, c, value=None):
        """one launch with the plant at output element (m, c) -> what launch() returns"""
        L = self.L
        ref, _ = L.planted(m, c)
        v = L.sign() * V if value is None else value
        if L.wire is None:
            n, h, w_ = L.res_pixel(m)
            self.res[n, h, w_, c] = v
            out = self.launch(L.w, ref)
            self.res[n, h, w_, c] = 0.0
        else:
            n, h, w_ = L.wire_pixel(m)
            x = self.x.clone()
            x[n, h, w_, L.wire] = v
            out = self.launch(L.w_for(c), ref, x=x)
        return out, ref


def _conv_case(eng, n_cu, name, tier, w22=None):
    L = RC.ConvLayer(name, tier, n_cu)
    D = DevConv(eng, L, n_cu, w22)
    cross = RC.conv_cross(L.M, D.pl)
    rows = RC.conv_rows(L.M, D.pl)
    if L.c["shape"] == "rounds":
        assert "high_row_tile" in rows and (not L.c.get("slab") or {"tail_first", "tail_middle", "tail_last"} <= set(rows)), rows
    t0 = time.time()
    for label, m, c in cross:
        ref, runner = L.planted(m, c)
        assert ref >= RC.DOMINANCE * runner                                   # (a condition on the reference: tests/test_range_cases_cpu.py)
        (got, ymax), _ = D.plant(m, c)
        print("[range] %s %s %s (%d, %d): slots %.9g, float64 %.9g" % (name, tier, label, m, c, got, ref))
        assert abs(got - ref) <= TOL * ref, (name, tier, label, m, c, got, ref, runner)
        if ymax is not None:
            assert got == ymax, (name, tier, label, m, c, got, ymax)
    torch.cuda.synchronize()
    print("[range] %s %s: %d launches on %s, %.2f s" % (name, tier, len(cross), D.pl["kernel_name"], time.time() - t0))
    return D


CONV_IDS = [(n, t) for n, t in RC.conv_case_ids() if not RC.CONV_CASES[n].get("env")]
CELL_IDS = [(n, t) for n, t in CONV_IDS if t != "f32"]


@pytest.mark.parametrize("name,tier", CONV_IDS)
def test_conv_range_finds_the_plant_at_every_seam(eng, n_cu, name, tier):
    _conv_case(eng, n_cu, name, tier, w22=1)


def test_cell_kernels_on_the_4x1_wave_layout(eng, n_cu, request):
    """DGP_WAVE_2X2=0: every cell case once more on 4 x 1 waves of 32 x 128 (a child process; w22 asserted through the plan)"""
    if not _respawn(request, DGP_WAVE_2X2="0"):
        return
    for name, tier in CELL_IDS:
        _conv_case(eng, n_cu, name, tier, w22=0)


@pytest.mark.parametrize("w22", [1, 0])
def test_k_split_tail_on_cell_inputs(eng, n_cu, w22, request):
    """DGP_TAIL_SPLIT=2 (a child process): tail_fixup_h2_kernel owns the rows of the tail tiles; plants, the padding case and the zero case"""
    if not _respawn(request, DGP_TAIL_SPLIT="2", DGP_WAVE_2X2=str(w22)):
        return
    _conv_case(eng, n_cu, "tail_h2", "h2", w22=w22)
    _padding_case(eng, n_cu, "tail_h2", "h2")


def _padding_case(eng, n_cu, name, tier):
    for mode in ("padding", "zero"):
        L = RC.ConvLayer(name, tier, n_cu, mode=mode)
        D = DevConv(eng, L, n_cu)
        assert L.M % RC.BM != 0 and RC.COUT % RC.BN != 0
        ref = L.ref_max()
        got, ymax = D.launch(L.w, ref)
        print("[range] %s %s %s: B %.3g, slots %.9g, float64 %.9g" % (name, tier, mode, L.B, got, ref))
        if mode == "zero":
            assert got == 0.0 and ref == 0.0, (name, tier, got)
        else:
            assert 0 < ref <= 0.8 * L.B and abs(got - ref) <= TOL * ref, (name, tier, got, ref, L.B)
        if ymax is not None:
            assert got == ymax


@pytest.mark.parametrize("name,tier", [(n, t) for n, t in RC.pad_case_ids() if not RC.CONV_CASES[n].get("env")])
def test_conv_range_does_not_count_padded_rows_or_channels(eng, n_cu, name, tier):
    _padding_case(eng, n_cu, name, tier)


@pytest.mark.parametrize("name,tier", [(n, t) for n, t in CONV_IDS if (RC.CONV_CASES[n]["res"]["h2"] if isinstance(RC.CONV_CASES[n]["res"], dict)
                                                                      else RC.CONV_CASES[n]["res"]) == "f32" and t != "h1"])
def test_conv_range_carries_infinity(eng, n_cu, name, tier):
    L = RC.ConvLayer(name, tier, n_cu)
    D = DevConv(eng, L, n_cu)
    rows = RC.conv_rows(L.M, D.pl)
    for m, c in ((rows["last"], RC.COUT - 1), (rows.get("high_row_tile", 64), 5)):
        (got, ymax), _ = D.plant(m, c, value=L.sign() * INF)
        assert got == INF and ymax == INF, (name, tier, m, c, got, ymax)


# ------------------------------------------------------------------------------------------------------------------ chain and unit kernels
class DevFused:
    def __init__(self, eng, L, h1):
        self.eng, self.L, self.h1 = eng, L, h1
        self.e = eng.h2_exp_for(V)                                           # one scale for every tensor: what it holds is exact up to V
        self.a = torch.from_numpy(L.full(L.a_in)).cuda()
        self.s2 = torch.from_numpy(L.full(L.src2)).cuda()
        self.ah = self.cells(self.a)
        self.s2h = self.cells(self.s2)

    def cells(self, t, e=None):
        e = self.e if e is None else e
        if self.h1:
            c = self.eng.f32_to_h1(t, e)
            assert torch.equal(self.eng.h1_to_f32(c, e), t)
        else:
            c = self.eng.f32_to_h2(t, e)
            assert torch.equal(self.eng.h2_to_f32(c, e), t)
        return c

    def launch(self, ah=None, s2h=None, keep=1, xout=None, exps=None):
        """-> (xout, {slot set: max})"""
        L, eng = self.L, self.eng
        ah = self.ah if ah is None else ah
        s2h = self.s2h if s2h is None else s2h
        e_in, e_r2, e_x, e_o = exps or (self.e,) * 4
        if L.unit:
            xo, r1o, r2r, xr, orr = eng.unit_h2(ah, e_in, s2h, e_in if L.res_mode != 0 else e_r2, L.w2, L.s2, L.b2, e_r2, L.w3, L.s3, L.b3, L.w1, L.s1, L.b1,
                                                L.res_mode, e_x, e_o, h1=self.h1, xout_keep=keep, xout=xout)
            return xo, dict(r2=float(r2r.max()), x=float(xr.max()), r1=float(orr.max()))
        xo, r1, xr, rr = eng.chain_h2(ah, e_in, s2h, e_in, L.w3, L.s3, L.b3, L.w1, L.s1, L.b1, L.res_mode, e_x, e_o, h1=self.h1, xout_keep=keep, xout=xout)
        return xo, dict(x=float(xr.max()), r1=float(rr.max()))

    def plant_in(self, n, y, x, **kw):
        """V on the wire of the first input (R1 of the unit kernel, R2 of the chain) at pixel (n, y, x): arrives in every slot set"""
        L = self.L
        ch = L.K00 if L.unit else L.K0
        self.a[n, y, x, ch] = V
        out = self.launch(ah=self.cells(self.a), **kw)
        self.a[n, y, x, ch] = 0.0
        return out

    def plant_src2(self, n, y, x, **kw):
        """V on the wire of the second source (the residual's channel J0, or channel K1 of the K-concatenated source): X' and R1'"""
        L = self.L
        ch = L.K1 if L.res_mode == 0 else L.J0
        yy, xx = (2 * y, 2 * x) if L.res_mode == 2 else (y, x)
        self.s2[n, yy, xx, ch] = V
        out = self.launch(s2h=self.cells(self.s2), **kw)
        self.s2[n, yy, xx, ch] = 0.0
        return out


def _fused_plants(eng, n_cu, kind, inst, size, h1):
    L = RC.fused_layer(kind, inst, size, n_cu)
    tops = L.base_max()
    assert all(RC.DOMINANCE * t <= V for t in tops), tops                     # (tests/test_range_cases_cpu.py)
    D = DevFused(eng, L, h1)
    if kind == "chain":
        px = {k: divmod(p, L.H * L.W) for k, p in RC.chain_pixels(L.N, L.H, L.W, size == "big", n_cu).items()}
        px = {k: (n,) + divmod(r, L.W) for k, (n, r) in px.items()}
        if size == "big":
            assert {"second_round", "later_round"} <= set(px)
    else:
        px = RC.unit_pixels(L.N, L.H, L.W)
    t0 = time.time()
    for label, (n, y, x) in px.items():
        _, got = D.plant_in(n, y, x)
        print("[range] %s %s %s h1 %d %s: through the first input %s" % (kind, inst, size, h1, label, got))
        for k, g in got.items():
            assert abs(g - V) <= TOL * V, (kind, inst, size, h1, label, "first input", k, g)
        _, got = D.plant_src2(n, y, x)
        print("[range] %s %s %s h1 %d %s: through the second source %s" % (kind, inst, size, h1, label, got))
        for k in ("x", "r1"):
            assert abs(got[k] - V) <= TOL * V, (kind, inst, size, h1, label, "second source", k, got[k])
        if "r2" in got:                                                       # R2 did not see this plant: its range is the base's
            assert abs(got["r2"] - tops[0]) <= TOL * tops[0], (kind, inst, size, h1, label, got["r2"], tops[0])
    torch.cuda.synchronize()
    print("[range] %s %s %s h1 %d: %d launches, %.2f s" % (kind, inst, size, h1, 2 * len(px), time.time() - t0))


@pytest.mark.parametrize("h1", [False, True])
@pytest.mark.parametrize("inst,size", [(i, "small") for i in RC.CHAIN_INSTANCES] + [(i, "big") for i in RC.CHAIN_BIG])
def test_chain_ranges_find_the_plant(eng, n_cu, inst, size, h1):
    _fused_plants(eng, n_cu, "chain", inst, size, h1)


@pytest.mark.parametrize("h1", [False, True])
@pytest.mark.parametrize("inst,size", [((64, 64) + i, s) for i in RC.UNIT_INSTANCES for s in list(RC.UNIT_MAPS) + ["big"]])
def test_unit_ranges_find_the_plant(eng, n_cu, inst, size, h1):
    _fused_plants(eng, n_cu, "unit", inst, size, h1)


@pytest.mark.parametrize("h1", [False, True])
@pytest.mark.parametrize("kind", ["chain", "unit"])
def test_ranges_cover_the_pixels_whose_x_is_not_stored(eng, n_cu, kind, h1):
    """xout_keep = 2 stores X' at even rows and columns only; a plant at an odd / odd pixel (and an odd / even, an even / odd one) is not
    stored -- the caller's buffer keeps its bits there -- and the slots must still report it"""
    L = RC.fused_layer(kind, (64, 64, 0, 1), "small" if kind == "chain" else "ragged", n_cu)
    D = DevFused(eng, L, h1)
    for n, y, x in ((0, 1, 1), (L.N - 1, L.H - 2, L.W - 2), (0, 7, 15), (0, 3, 4), (1, 4, 3), (0, 2, 2)):
        stored = y % 2 == 0 and x % 2 == 0
        for plant in (D.plant_src2, D.plant_in):
            xout = torch.zeros((L.N, L.H, L.W, 4 * L.C), device="cuda", dtype=torch.float16 if h1 else torch.float32)
            xo, got = plant(n, y, x, keep=2, xout=xout)
            print("[range] %s xkeep 2 h1 %d pixel (%d, %d, %d) stored %d: %s" % (kind, h1, n, y, x, stored, got))
            for k, g in got.items():
                if k != "r2" or plant == D.plant_in:                         # (the second source does not reach R2)
                    assert abs(g - V) <= TOL * V, (kind, h1, (n, y, x), k, g)
            assert bool((xo[n, y, x].view(torch.int16) != 0).any()) == stored


@pytest.mark.parametrize("h1", [False, True])
@pytest.mark.parametrize("kind,inst", [("chain", (64, 64, 0, 1)), ("chain", (64, 64, 64, 0)), ("unit", (64, 64, 0, 1)), ("unit", (64, 64, 64, 0))])
def test_fused_ranges_do_not_count_padded_pixels(eng, n_cu, kind, inst, h1):
    """ragged tiles in both directions (782 pixels; 13 x 21 maps): a padded pixel would report relu(B) = B for R2 and X'.  R1' is NOT
    guarded in this direction: a padded pixel's X' is B3, so its R1' = relu(B1 - |w1| . B3) lies below the real maxima (a real pixel whose
    X' is all zero reports B1 itself); its slots are only held to the float64 maximum.  The zero form likewise guards R2 and X'."""
    size = "small" if kind == "chain" else "ragged"
    for mode in ("padding", "zero"):
        L = RC.fused_layer(kind, inst, size, n_cu, mode=mode)
        D = DevFused(eng, L, h1)
        exps, force = {}, {}

        def cells(stage, a):
            """the values the stage's output cells hold, at the scale its maximum asks for (the engine's own converters)"""
            exps[stage] = e = force.get(stage, eng.h2_exp_for(float(a.max())))
            t = torch.from_numpy(a.astype(np.float32)).cuda()
            q = eng.h1_to_f32(eng.f32_to_h1(t, e), e) if h1 else eng.h2_to_f32(eng.f32_to_h2(t, e), e)
            return q.double().cpu().numpy()

        e_in = D.e
        if L.unit and L.res_mode == 0:                                        # R2 and the K-concatenated source share one scale
            force["r2"] = eng.h2_exp_for(max(float(L.outputs()[0].max()), float(L.src2.max())))
            D.s2h = D.cells(D.s2, force["r2"])
        r2, x, r1 = L.outputs(cells=cells)
        e_r2 = exps.get("r2", e_in)
        _, got = D.launch(exps=(e_in, e_r2, exps["x"], eng.h2_exp_for(float(r1.max()))))
        refs = dict(r2=None if r2 is None else float(r2.max()), x=float(x.max()), r1=float(r1.max()))
        print("[range] %s %s h1 %d %s: slots %s, float64 %s" % (kind, inst, h1, mode, got, refs))
        for k, g in got.items():
            if mode == "zero":
                assert g == 0.0 and refs[k] == 0.0, (kind, inst, h1, k, g)
            else:
                assert refs[k] > 0 and abs(g - refs[k]) <= TOL * refs[k], (kind, inst, h1, k, g, refs[k])


# ------------------------------------------------------------------------------------------------------------------ root block
def _root_launch(eng, frames, wts, cells, ref):
    t = lambda a: torch.from_numpy(a).cuda()
    _, _, got = eng.root_block(t(frames), t(wts[0]), t(wts[1]), t(wts[2]), RC.ROOT_MEAN, cells=cells, out_exp=eng.h2_exp_for(ref))
    return got


@pytest.mark.parametrize("cells", ["h2", "h1"])
@pytest.mark.parametrize("frame", RC.ROOT_FRAMES)
def test_root_block_range_finds_a_bright_patch_in_every_corner(eng, frame, cells):
    """Dark frames (the mean pixel) with one bright 3 x 3 patch at the centre of the window of the conv1 pixel that lies in ONE pool cell
    (tests/_range_cases.root_patch): the float64 pool maximum lies in that cell and every other cell is at most a quarter of it
    (tests/test_range_cases_cpu.py asserts the same on the CPU)."""
    H, W = frame
    assert tuple(eng.MEAN_PIXEL) == RC.ROOT_MEAN
    wts = RC.root_weights()
    for name, target in RC.root_targets(H, W).items():
        frames = RC.root_frames(H, W, target)
        ref, runner, hit = RC.root_dominance(RC.root_reference(frames, wts, cells, "cuda"), target)
        assert hit and RC.DOMINANCE * runner <= ref and ref > 50, (name, ref, runner, hit)
        _close(_root_launch(eng, frames, wts, cells, ref), ref, "root block %s %s %s" % (frame, cells, name))


@pytest.mark.parametrize("cells", ["h2", "h1"])
@pytest.mark.parametrize("frame", RC.ROOT_FRAMES)
def test_root_block_range_does_not_count_elements_outside_the_map(eng, frame, cells):
    """Frames of 255, all-negative weights, bias B on every channel: real conv1 values are relu(B - something); a conv1 pixel outside the
    map (the kernel computes whole tiles and masks them) or a padded pool cell that were counted would report B.  Both frames are ragged
    against the kernel's pool tiles.  With -B every output is 0 and the tracked maximum must be exactly 0.0."""
    H, W = frame
    frames = RC.root_frames(H, W, bright=True)
    wts = RC.root_weights("padding")
    ref = float(RC.root_reference(frames, wts, cells, "cuda").max())
    assert 0 < ref <= 0.9 * RC.ROOT_B, (ref, RC.ROOT_B)
    _close(_root_launch(eng, frames, wts, cells, ref), ref, "root block %s %s padding, B %g" % (frame, cells, RC.ROOT_B))
    wts = RC.root_weights("zero")
    assert float(RC.root_reference(frames, wts, cells, "cuda").max()) == 0.0
    got = _root_launch(eng, frames, wts, cells, 0.0)
    print("[range] root block %s %s zero: %r" % (frame, cells, got))
    assert got == 0.0, got
