"""The grid plans of the conv launch layer against float64: the K-split of the grid's tail (raw slabs + tail_fixup_kernel /
tail_fixup_h2_kernel), the supertile order and the deep ring.  A plan is decided at full-size grids only, so every case builds its
shape from the device's own CU count, ASSERTS THROUGH THE PLAN QUERY (engine.conv2d_plan) that the launch takes the plan the case is
about -- a case cannot go vacuous -- runs the layer through the layer-level entry points with the caller's tail slab, and compares with
a float64 reference computed on the device (im2col + matmul; on cell inputs the reference convolves what the cells hold).  Output and
slab are pre-filled with NaN, so a tile or a slab slice nobody wrote shows.  Every case has a ragged last row tile, scale, bias and ReLU.

Tolerances are the project's own (a K-split only reorders at most four fp32 partial sums): 2e-5 of max |ref| (3e-4 on the 3-term bf16
tiles 8 and 11, tests/test_parity_gpu.py::test_every_tile_variant_matches_oracle), 2e-5 on cells; the tracked output range equals
max |y| exactly for fp32 outputs and within 1e-4 for cell outputs (tests/test_h2_gpu.py).  Measured errors: EXPERIMENTS.md, "Conv grid
plans against float64"."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _conv_plan_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.fixture(scope="module")
def eng(lib_built):
    from deepgraphpose_amd import engine
    return engine


@pytest.fixture(scope="module")
def n_cu(eng):
    return eng.conv2d_plan((1, 1, 128, 64), (1, 1, 64, 128))["n_cu"]


def _tol(tile):
    return 3e-4 if tile in (8, 11) else 2e-5


def _grid(mtiles, n=3, w=41):
    """(N, H, W) with ceil(N H W / 128) == mtiles and a ragged last row tile"""
    h = (mtiles * 128 - 1) // (n * w)
    M = n * h * w
    assert -(-M // 128) == mtiles and M % 128 != 0
    return n, h, w


def _im2col_matmul(xq, w, k, pad, rate=1):
    """float64 conv, stride 1, output on the input grid: xq [N,H,W,Cin] float64 (device), w [k,k,Cin,Cout] numpy -> [N,H,W,Cout]"""
    N, H, W, Cin = xq.shape
    wt = torch.from_numpy(w.reshape(-1, w.shape[3])).double().cuda()
    if k == 1:
        return (xq.reshape(-1, Cin) @ wt).reshape(N, H, W, -1)
    xp = torch.zeros((N, H + 2 * pad, W + 2 * pad, Cin), dtype=torch.float64, device="cuda")
    xp[:, pad:pad + H, pad:pad + W] = xq
    cols = [xp[:, a * rate: a * rate + H, b * rate: b * rate + W] for a in range(k) for b in range(k)]
    return (torch.stack(cols, 3).reshape(N * H * W, k * k * Cin) @ wt).reshape(N, H, W, -1)


class Layer:
    """One layer's operands and its float64 reference without the residual (computed once, shared by the cases on it)"""

    def __init__(self, seed, nhw, cin, cout, k=1, cells=False, eng=None):
        N, H, W = nhw
        g = torch.Generator(device="cuda").manual_seed(seed)
        rng = np.random.default_rng(seed)
        self.k, self.pad, self.shape = k, (k - 1) // 2, (N, H, W, cin)
        self.w = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
        self.scale = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
        self.bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        x = torch.randn((N, H, W, cin), device="cuda", generator=g) * 3.0
        self.seed, self.cout, self._res = seed, cout, {}
        if cells:
            x = torch.relu(x)
            self.x_exp = eng.h2_exp_for(float(x.abs().max()))
            self.x = eng.f32_to_h2(x, self.x_exp)
            xq = eng.h2_to_f32(self.x, self.x_exp).double()
        else:
            self.x, xq = x, x.double()
        self.base = _im2col_matmul(xq, self.w, k, self.pad) * torch.from_numpy(self.scale).double().cuda() + torch.from_numpy(self.bias).double().cuda()

    def res(self, res_stride):
        """the residual on the output grid (1) or on the 2x finer one (2), made on first use"""
        if res_stride not in self._res:
            N, H, W, _ = self.shape
            g = torch.Generator(device="cuda").manual_seed(self.seed * 7 + res_stride)
            shape = (N, H, W, self.cout) if res_stride == 1 else (N, 2 * H - 1, 2 * W, self.cout)
            self._res[res_stride] = torch.randn(shape, device="cuda", generator=g) * 2.0
        return self._res[res_stride]

    def ref(self, res_stride=0, resq=None):
        if not res_stride:
            return torch.relu(self.base)
        r = (self.res(res_stride) if resq is None else resq).double()
        return torch.relu(self.base + (r if res_stride == 1 else r[:, ::2, ::2]))

    def plan_args(self, res_stride=0):
        rs = self.res(res_stride).shape if res_stride else (0, 0, 0)
        return dict(x_shape=self.shape, w_shape=self.w.shape, pad_t=self.pad, pad_l=self.pad, res_stride=res_stride, res_hw=(rs[1], rs[2]))


def _run_fp32(eng, L, slab_floats, res_stride=0, want=None, cells=False, ranged=True, label=""):
    """plan query (asserted against `want`) -> launch with NaN-filled output and slab -> (y, error against float64, the plan)"""
    slab = torch.full((slab_floats,), NAN, device="cuda") if slab_floats else None
    pl = eng.conv2d_plan(**L.plan_args(res_stride), slab_bytes=4 * slab_floats, cells=cells, ranged=ranged)
    if want:
        assert {k: pl[k] for k in want} == want, (pl, want)
    N, H, W, _ = L.shape
    y = torch.full((N, H, W, L.w.shape[3]), NAN, device="cuda")
    y2, yr = eng.conv2d(L.x, L.w, pad_t=L.pad, pad_l=L.pad, out_hw=(H, W), scale=L.scale, bias=L.bias,
                        residual=L.res(res_stride) if res_stride else None, res_stride=res_stride, relu=True, ranged=ranged,
                        return_range=True, tail_slab=slab, out=y)
    assert y2 is y
    ref = L.ref(res_stride)
    err = float((y.double() - ref).abs().max() / ref.abs().max())          # (NaN where a tile was not written: fails every bound)
    print("[conv-plan] %s tile %d ks %d grid %d: err %.3g (tol %.0e)" % (label, pl["tile"], pl["tail_ksplit"], pl["grid"], err, _tol(pl["tile"])))
    assert float(yr.max()) == float(y.abs().max())                         # the tracked range is exact, fix-up launch included
    return y, err, pl


def _run_h2(eng, L, slab_floats, res_kind=None, res_stride=0, y_h2=True, want=None, label=""):
    """as _run_fp32 on H2 cells; res_kind 'h2' / 'f32'"""
    slab = torch.full((slab_floats,), NAN, device="cuda") if slab_floats else None
    res = res_t = resq = None
    res_exp = 0
    if res_stride:
        res = L.res(res_stride)
        if res_kind == "h2":
            res_exp = eng.h2_exp_for(float(res.abs().max()))
            res_t = eng.f32_to_h2(res, res_exp)
            resq = eng.h2_to_f32(res_t, res_exp)
        else:
            res_t = resq = res
    pl = eng.conv2d_plan(**L.plan_args(res_stride), in_fmt=1, out_fmt=int(y_h2), res_fmt=int(res_kind == "h2"), slab_bytes=4 * slab_floats)
    if want:
        assert {k: pl[k] for k in want} == want, (pl, want)
    ref = L.ref(res_stride, resq)
    y_exp = eng.h2_exp_for(float(ref.abs().max()))
    N, H, W, _ = L.shape
    y = torch.full((N, H, W, L.w.shape[3]), NAN, device="cuda")
    y2, yr = eng.conv2d_h2(L.x, L.x_exp, L.w, pad_t=L.pad, pad_l=L.pad, out_hw=(H, W), scale=L.scale, bias=L.bias, residual=res_t,
                           res_stride=res_stride, res_is_h2=res_kind == "h2", res_exp=res_exp, relu=True, y_is_h2=y_h2, y_exp=y_exp,
                           tail_slab=slab, out=y)
    assert y2 is y
    out = eng.h2_to_f32(y, y_exp) if y_h2 else y
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print("[conv-plan] %s ks %d grid %d st_gn %d deep %d: err %.3g (tol 2e-05)" % (label, pl["tail_ksplit"], pl["grid"], pl["st_gn"], pl["deep"], err))
    if y_h2:
        assert abs(float(yr.max()) - float(ref.abs().max())) <= 1e-4 * float(ref.abs().max())
    else:
        assert float(yr.max()) == float(y.abs().max())
    return out, err, pl


def _respawn(request, **env):
    """Switches read once per process: True in a process that has them (the body runs); otherwise the test runs again in a child pytest
    process with them, must pass there, and the body returns at once"""
    if all(os.environ.get(k) == v for k, v in env.items()):
        return True
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    r = subprocess.run([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-rA", "-s", "-m", "gpu", "-p", "no:cacheprovider"], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    sys.stdout.write("".join(line + "\n" for line in r.stdout.splitlines() if line.startswith("[conv-plan]")))
    assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    return False


# ---------------------------------------------------------------- tail K-split, fp32 in and out
SLAB_32MB = (32 << 20) // 4


@pytest.fixture(scope="module")
def t1(eng, n_cu):
    """T1, pointwise 512 -> 512 on slots / 4 + 2 row tiles: 8 tail tiles, split 4 ways"""
    return Layer(101, _grid(2 * n_cu // 4 + 2), 512, 512)


@pytest.fixture(scope="module")
def t3(eng, n_cu):
    """T3, 3 x 3 / stride 1, 64 -> 128 on slots + 1 row tiles (one column tile): 18 K-steps, the per-tap loader walk"""
    return Layer(103, _grid(2 * n_cu + 1), 64, 128, k=3)


@pytest.mark.parametrize("res_stride", [0, 1, 2])
@pytest.mark.parametrize("tile", [16, 13, 10, 11, 7, 8])
def test_t1_tail_split_of_a_pointwise_layer_on_every_128_column_tile(eng, n_cu, t1, tile, res_stride, monkeypatch):
    """fp16 (F16 fix-up: post-scale from the ranges) and bf16 tiles, 32 and 16 floats per K-step; no residual, one on the same grid, one
    subsampled from the 2x finer grid (res_stride 2)."""
    monkeypatch.setenv("DGP_FORCE_TILE", str(tile))
    slots = 2 * n_cu
    want = dict(tile=tile, mtiles=slots // 4 + 2, ntiles=4, tail_ksplit=4, n_main=slots, grid=slots + 32)
    _, err, _ = _run_fp32(eng, t1, SLAB_32MB, res_stride, want, ranged=tile >= 13, label="T1 res %d" % res_stride)
    assert err < _tol(tile), err


def test_t2_tail_split_two_ways_with_a_slab_that_just_fits(eng, n_cu):
    slots = 2 * n_cu
    rem_rows = slots * 50 // 512                        # rem = 4 rem_rows in (slots / 3, slots / 2]: ks = 2
    L = Layer(102, _grid(slots // 4 + rem_rows), 256, 512)
    want = dict(tile=16, tail_ksplit=2, n_main=slots, grid=slots + 8 * rem_rows)
    _, err, _ = _run_fp32(eng, L, R.tail_slab_bytes(4 * rem_rows, 2) // 4, 1, want, label="T2")
    assert err < 2e-5, err


@pytest.mark.parametrize("tile,ks", [(16, 3), (10, 4)])
def test_t3_tail_split_of_a_3x3_layer(eng, n_cu, t3, tile, ks, monkeypatch):
    """18 K-steps: the search drops 4 (18 % 4 != 0) and takes 3; 36 steps of 16 floats on tile 10: 4"""
    monkeypatch.setenv("DGP_FORCE_TILE", str(tile))
    slots = 2 * n_cu
    want = dict(tile=tile, mode=1, mtiles=slots + 1, ntiles=1, tail_ksplit=ks, n_main=slots, grid=slots + ks)
    _, err, _ = _run_fp32(eng, t3, SLAB_32MB, 1, want, ranged=tile >= 13, label="T3")
    assert err < _tol(tile), err


@pytest.mark.parametrize("case", ["shallow_k", "two_rounds", "ks_1", "slab_short"])
def test_t4_layers_that_do_not_split_with_the_slab_given(eng, n_cu, t1, case):
    """The slab is there and the rule says no: parts below 4 K-steps; two full rounds in front and < 48 K-steps; a tail of more than
    half a round (ks would be 1); a slab one float short (the layer-level entry point takes float32 tensors)."""
    slots = 2 * n_cu
    slab = SLAB_32MB
    if case == "shallow_k":
        L = Layer(104, _grid(slots // 4 + 2), 128, 512)
    elif case == "two_rounds":
        L = Layer(105, _grid(slots // 2 + 2), 512, 512)
    elif case == "ks_1":
        L = Layer(106, _grid(slots + slots // 2 + 1), 512, 128)
    else:
        L, slab = t1, R.tail_slab_bytes(8, 4) // 4 - 1
    tiles = -(-L.shape[0] * L.shape[1] * L.shape[2] // 128) * (L.w.shape[3] // 128)
    _, err, _ = _run_fp32(eng, L, slab, 1, dict(tile=16, tail_ksplit=0, n_main=tiles, grid=tiles), label="T4 " + case)
    assert err < 2e-5, err


def test_t4b_two_rounds_split_at_a_deep_k(eng, n_cu):
    slots = 2 * n_cu
    L = Layer(107, _grid(slots // 2 + 2), 2048, 512)
    _, err, _ = _run_fp32(eng, L, SLAB_32MB, 1, dict(tile=16, tail_ksplit=4, n_main=2 * slots, grid=2 * slots + 32), label="T4b")
    assert err < 2e-5, err


def test_t5_split_and_unsplit_agree_bit_for_bit_in_front_of_the_tail(eng, n_cu, t1):
    slots = 2 * n_cu
    y0, err0, pl0 = _run_fp32(eng, t1, 0, 1, dict(tile=16, tail_ksplit=0, grid=slots + 8), label="T5 unsplit")
    y1, err1, pl1 = _run_fp32(eng, t1, SLAB_32MB, 1, dict(tile=16, tail_ksplit=4, n_main=slots, grid=slots + 32), label="T5 split")
    M, Cout = y0.numel() // y0.shape[3], y0.shape[3]
    tile_id = (torch.arange(M, device="cuda")[:, None] // 128) * pl1["ntiles"] + torch.arange(Cout, device="cuda")[None, :] // 128      # row-major
    main = tile_id < pl1["n_main"]
    a, b = y0.reshape(M, Cout), y1.reshape(M, Cout)
    assert bool(main.any()) and bool((~main).any())
    assert torch.equal(a[main], b[main])
    assert err0 < 2e-5 and err1 < 2e-5                 # (the tail tiles are inside err1)
    assert not torch.equal(a[~main], b[~main])         # another summation order: the split ran


@pytest.mark.parametrize("ks", [4, 2])
def test_t6_tail_split_is_exact_on_integers(eng, n_cu, ks):
    """Integer activations below 2^13 (both fp16 parts are needed) times a 0 / 1 matrix with exactly one 1 per column in each quarter of
    K: every output is the sum of four integers, exact in every slice and in the fix-up.  A dropped, repeated or permuted slice and a
    wrong n_main change integers."""
    slots = 2 * n_cu
    cin = 512 if ks == 4 else 256
    mtiles = slots // 4 + (2 if ks == 4 else slots * 50 // 512)
    N, H, W = _grid(mtiles)
    M, cout = N * H * W, 512
    rng = np.random.default_rng(60 + ks)
    x = torch.from_numpy(rng.integers(0, 8192, (N, H, W, cin)).astype(np.float32)).cuda()
    q = cin // 4
    rows = np.stack([rng.integers(0, q, cout) + j * q for j in range(4)])          # [4, cout]: the row of the 1 in each quarter
    w = np.zeros((1, 1, cin, cout), np.float32)
    for j in range(4):
        w[0, 0, rows[j], np.arange(cout)] = 1.0
    bias = rng.integers(-20000, 100, cout).astype(np.float32)
    xi = x.reshape(M, cin).long()
    ref = torch.relu(sum(xi[:, torch.from_numpy(rows[j]).cuda()] for j in range(4)) + torch.from_numpy(bias).long().cuda())
    rem = mtiles * 4 - slots
    pl = eng.conv2d_plan((N, H, W, cin), w.shape, slab_bytes=4 * SLAB_32MB)
    assert (pl["tile"], pl["tail_ksplit"], pl["n_main"], pl["grid"]) == (16, ks, slots, slots + rem * ks), pl
    y = torch.full((N, H, W, cout), NAN, device="cuda")
    slab = torch.full((SLAB_32MB,), NAN, device="cuda")
    eng.conv2d(x, w, bias=bias, relu=True, ranged=True, tail_slab=slab, out=y)
    assert torch.equal(y.reshape(M, cout), ref.float())
    assert float(ref.max()) > 2 ** 14 and float((ref == 0).float().mean()) > 0.001


def test_t7_tail_split_on_the_cell_kernels_with_fp32_tensors(eng, n_cu, request):
    """DGP_CONV2D_CELLS=1: the compute-side-split / LDS-DMA kernels on fp32 tensors (T1 and T3), in a child process"""
    if not _respawn(request, DGP_CONV2D_CELLS="1"):
        return
    slots = 2 * n_cu
    L = Layer(101, _grid(slots // 4 + 2), 512, 512)
    _, err, _ = _run_fp32(eng, L, SLAB_32MB, 2, dict(tile=16, cs=1, dma=1, mode=2, tail_ksplit=4, n_main=slots, grid=slots + 32), cells=True, label="T7 T1")
    assert err < 2e-5, err
    L = Layer(103, _grid(slots + 1), 64, 128, k=3)
    _, err, _ = _run_fp32(eng, L, SLAB_32MB, 1, dict(tile=16, cs=1, dma=1, mode=1, tail_ksplit=3, n_main=slots, grid=slots + 3), cells=True, label="T7 T3")
    assert err < 2e-5, err


# ---------------------------------------------------------------- tail K-split on cells (forced: DGP_TAIL_SPLIT=2)
def test_tail_split_fixup_on_h2_tensors(eng, n_cu, request):
    """The K-split of the grid tail is off by default for H2 launches (measured slower); DGP_TAIL_SPLIT=2 forces it (a child process).
    H-T1: the batch-32 block3 conv1 (32, 30, 40, 1024 -> 256), 600 tiles: at 256 CUs 88 tail tiles split 4 ways + tail_fixup_h2_kernel,
    without a residual, with an H2 and with an fp32 one.  H-T2: H2 in, fp32 out on T1's geometry: tail_fixup_kernel<.., true> whose
    post-scale comes from the cells' scale.  H-T3: 512 -> 1024 on one round plus a tail, the H2 residual subsampled from the 2x finer grid."""
    if not _respawn(request, DGP_TAIL_SPLIT="2"):
        return
    slots = 2 * n_cu
    mt = slots // 2 + 44                                          # 300 row tiles of 2 column tiles at 256 CUs
    L = Layer(201, (32, 30, 40) if n_cu == 256 else _grid(mt), 1024, 256, cells=True, eng=eng)
    want = dict(tile=16, mtiles=mt, ntiles=2, tail_ksplit=4, n_main=slots, grid=slots + 88 * 4, ah2=1, oh2=1)
    for kind, rs in ((None, 0), ("h2", 1), ("f32", 1)):
        _, err, _ = _run_h2(eng, L, SLAB_32MB, kind, rs, True, want, label="H-T1 res %s" % kind)
        assert err < 2e-5, (kind, err)
    L = Layer(202, _grid(slots // 4 + 2), 512, 512, cells=True, eng=eng)
    want = dict(tile=16, tail_ksplit=4, n_main=slots, grid=slots + 32, ah2=1, oh2=0)
    for kind, rs in ((None, 0), ("f32", 1)):
        _, err, _ = _run_h2(eng, L, SLAB_32MB, kind, rs, False, want, label="H-T2 res %s" % kind)
        assert err < 2e-5, (kind, err)
    L = Layer(203, _grid(slots // 8 + 2), 512, 1024, cells=True, eng=eng)
    want = dict(tile=16, ntiles=8, tail_ksplit=4, n_main=slots, grid=slots + 64, st_gn=0)
    _, err, _ = _run_h2(eng, L, SLAB_32MB, "h2", 2, True, want, label="H-T3")
    assert err < 2e-5, err


# ---------------------------------------------------------------- supertile order and deep ring (H2 in and out, default switches)
def test_s1_supertile_order_with_a_padded_last_band(eng):
    """67 row tiles x 8 column tiles: bands of 9 row tiles, the last one 4 of 9 (its other blocks return early), a second row chunk of one"""
    L = Layer(301, (3, 49, 58), 1024, 1024, cells=True, eng=eng)                    # M = 67 x 128 - 50
    want = dict(mtiles=67, ntiles=8, st_gn=2, st_mc=8, st_mb=9, grid=576, tail_ksplit=0)
    _, err, _ = _run_h2(eng, L, 0, "h2", 1, True, want, label="S1")
    assert err < 2e-5, err


def test_s2_supertile_order_without_padding(eng):
    L = Layer(302, (2, 64, 64), 512, 2048, cells=True, eng=eng)
    _, err, _ = _run_h2(eng, L, 0, None, 0, True, dict(mtiles=64, ntiles=16, st_gn=4, st_mc=8, st_mb=8, grid=1024), label="S2")
    assert err < 2e-5, err


@pytest.mark.parametrize("case", ["63_row_tiles", "2MB_panel", "4_column_tiles"])
def test_s3_plain_order_beside_each_supertile_predicate(eng, case):
    nhw, cin, cout, grid = {"63_row_tiles": ((3, 49, 54), 1024, 1024, 63 * 8), "2MB_panel": ((3, 49, 58), 512, 1024, 67 * 8),
                            "4_column_tiles": ((3, 49, 58), 2048, 512, 67 * 4)}[case]
    L = Layer(303, nhw, cin, cout, cells=True, eng=eng)
    _, err, _ = _run_h2(eng, L, 0, "h2", 1, True, dict(st_gn=0, grid=grid, tail_ksplit=0), label="S3 " + case)
    assert err < 2e-5, err


def test_s4_supertile_order_writes_every_tile_once_exact(eng):
    """Selection matrix on S1's geometry: out[m][n] = x[m][n % Cin] with integers below 2^13 whose value names row and column"""
    N, H, W, C = 3, 49, 58, 1024
    M = N * H * W
    xi = (torch.arange(M, device="cuda")[:, None] * 131 + torch.arange(C, device="cuda")[None, :] * 17) % 8191
    x = xi.float().reshape(N, H, W, C)
    w = np.eye(C, dtype=np.float32).reshape(1, 1, C, C)
    e = eng.h2_exp_for(8190.0)
    xh = eng.f32_to_h2(x, e)
    assert torch.equal(eng.h2_to_f32(xh, e), x)
    pl = eng.conv2d_plan(x.shape, w.shape, in_fmt=1, out_fmt=1)
    assert (pl["st_gn"], pl["st_mc"], pl["st_mb"], pl["grid"]) == (2, 8, 9, 576), pl
    y = torch.full((N, H, W, C), NAN, device="cuda")
    eng.conv2d_h2(xh, e, w, relu=True, y_is_h2=True, y_exp=e, out=y)
    assert torch.equal(eng.h2_to_f32(y, e), x)


@pytest.mark.parametrize("extra_tiles,deep", [(0, 1), (4, 0)])
def test_deep_ring_on_each_side_of_one_tile_per_cu(eng, n_cu, extra_tiles, deep):
    mt = (n_cu + extra_tiles) // 4
    L = Layer(401, _grid(mt), 256, 512, cells=True, eng=eng)
    _, err, _ = _run_h2(eng, L, 0, "h2", 1, True, dict(mtiles=mt, ntiles=4, deep=deep, grid=4 * mt, dma=1), label="deep ring %d" % deep)
    assert err < 2e-5, err


# ---------------------------------------------------------------- the entry points with a slab are the ones without, bit for bit
@pytest.mark.parametrize("case", [(2, 17, 23, 64, 256, 1, 1), (1, 15, 20, 128, 128, 3, 2), (2, 19, 21, 64, 64, 3, 1), (1, 30, 40, 512, 512, 3, 2)])
def test_slab_entry_points_without_a_slab_are_the_old_ones_bit_for_bit(eng, case):
    """dgp_conv2d_ranged / dgp_conv2d_h2 forward to their _slab siblings with a null slab; called directly with an EMPTY slab (and, where
    the grid has no tail to split, with a real one) the siblings give the same bits -- on layers of tests/test_h2_gpu.py's table."""
    N, H, W, cin, cout, k, rate = case
    pad = rate * (k - 1) // 2
    g = torch.Generator(device="cuda").manual_seed(sum(case))
    rng = np.random.default_rng(sum(case))
    x = torch.relu(torch.randn((N, H, W, cin), device="cuda", generator=g)) * 3.0
    res = torch.randn((N, H, W, cout), device="cuda", generator=g)
    w = (rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    scale, bias = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32), (0.1 * rng.standard_normal(cout)).astype(np.float32)
    kw = dict(rate=rate, pad_t=pad, pad_l=pad, out_hw=(H, W), scale=scale, bias=bias, residual=res, res_stride=1, relu=True)
    empty, real = torch.empty(0, device="cuda"), torch.full((SLAB_32MB,), NAN, device="cuda")
    y0, r0 = eng.conv2d(x, w, ranged=True, return_range=True, **kw)
    for slab in (empty, real):
        y1, r1 = eng.conv2d(x, w, ranged=True, return_range=True, tail_slab=slab, **kw)
        assert torch.equal(y0, y1) and torch.equal(r0, r1)
    e = eng.h2_exp_for(float(x.abs().max()))
    xh = eng.f32_to_h2(x, e)
    y0, r0 = eng.conv2d_h2(xh, e, w, y_is_h2=True, y_exp=e - 2, **kw)
    for slab in (empty, real):
        y1, r1 = eng.conv2d_h2(xh, e, w, y_is_h2=True, y_exp=e - 2, tail_slab=slab, **kw)
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and torch.equal(r0, r1)
    assert bool(torch.isnan(real).all())               # nobody wrote the slab: these grids are smaller than one round
