"""dgp_conv2d_plan -- the host-side plan of a conv launch (csrc/dgp_kernels.hip, plan_conv; csrc/dgp_conv_split.hip, plan_split) -- against the independent restatement of
the grid rules in tests/_conv_plan_ref.py, for explicit numbers of CUs: no GPU is needed.  What a plan decides (the K-split of the
grid's tail, the supertile order, the deep ring) is otherwise reachable only at full-size grids; a refactor that sends a layer down
another, still correct kernel is caught here.  The GPU side (tests/test_conv_plan_gpu.py) asserts through the same query that each of
its launches takes the plan it is about.  The first sweep runs on 1 x M frames, which the halo ring never takes; a second one
(_halo_sweep) runs 3 x 3 layers on N x H x W frames around the ring's capacity bounds and holds the fourth rule, with a known-answer
table and the networks' own 3 x 3 layers at 256 CUs beside it (GPU side: tests/test_halo_walk_gpu.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import _conv_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# K-steps of 32 floats -> a kernel that has them: (KH, KW, Cin), nk = ceil(KH KW Cin / 32); Cin must be 4 * 2^k
KERNEL_OF_NK = {2: (1, 1, 64), 4: (1, 1, 128), 8: (1, 1, 256), 16: (1, 1, 512), 32: (1, 1, 1024), 64: (1, 1, 2048),
                9: (3, 3, 32), 18: (3, 3, 64), 36: (3, 3, 128), 72: (3, 3, 256), 47: (47, 1, 32), 48: (3, 1, 512)}
# tile id -> (K floats per step, columns, compute waves, needs ranges); the 128-row split tiles (TILES in dgp_conv.h)
SPLIT_TILES = {16: (32, 128, 4, True), 8: (32, 128, 4, False), 10: (16, 128, 4, False), 13: (16, 128, 4, True),
               12: (16, 128, 8, False), 15: (32, 64, 4, True)}
MB32 = 32 << 20


def _query(lib, mtiles, cout, nk, n_cu, slab=0, tile=-1, fmt=(0, 0, 0), ranged=1, cells=0, ragged=37):
    """plan of a layer with `mtiles` row tiles (ragged last one) and nk K-steps: one frame of 1 x M pixels"""
    from deepgraphpose_amd import _lib
    kh, kw, cin = KERNEL_OF_NK[nk]
    M = mtiles * 128 - ragged
    d = _lib.DgpConvDesc(1, 1, M, cin, cout, kh, kw, 1, 1, kh // 2, kw // 2, 1, M, 1, 1 if fmt[2] else 0, 1 if fmt[2] else 0, M if fmt[2] else 0)
    pl = _lib.DgpConvPlan()
    rc = lib.dgp_conv2d_plan(C.byref(d), fmt[0], fmt[1], fmt[2], ranged, cells, slab, tile, n_cu, C.byref(pl))
    return rc, pl


def _mtiles_around(n_cu, ntiles):
    """row-tile counts that put mtiles * ntiles on each side of every rule: the multiples of a round (2 n_cu), half a CU count beside
    them, the 3/4 boundary of the tail, one tile per CU"""
    slots = 2 * n_cu
    targets = {n_cu - 1, n_cu, n_cu + 1, n_cu + 4}
    for mult in (1, 2, 3):
        base = mult * slots
        for t in (base - n_cu // 2, base - 1, base, base + 1, base + 8, base + n_cu // 2, base + slots // 4, base + slots // 3, base + slots // 2,
                  base + 3 * slots // 4 - 1, base + 3 * slots // 4, base + 3 * slots // 4 + 1):
            targets.add(t)
    out = set()
    for t in targets:
        out.add(max(1, t // ntiles))
        out.add(-(-t // ntiles))
    return sorted(out)


def _sweep(lib, tail_env):
    """every mismatch between the query and the restatement, and the number of plans compared"""
    bad, n = [], 0

    def check(what, got, want):
        nonlocal n
        n += 1
        if got != want and len(bad) < 20:
            bad.append((what, got, want))

    for n_cu in (64, 104, 256, 304):
        for ntiles in (1, 2, 4, 8, 16):
            for mtiles in _mtiles_around(n_cu, ntiles):
                for nk in KERNEL_OF_NK:
                    # -- fp32 tensors on the split tiles, without and with weight cells
                    for tile, (bk, bn, cw, needs) in SPLIT_TILES.items():
                        nt_t = ntiles * (128 // bn)
                        nks = nk * (32 // bk)
                        ks_free, n_main, _ = R.tail_ksplit(mtiles, nt_t, nks, n_cu, 1 << 40, bn=bn, compute_waves=cw, tail_env=tail_env)
                        need = R.tail_slab_bytes(mtiles * nt_t - n_main, ks_free) if ks_free else 4 * R.TILE_FLOATS
                        for slab in (0, 4 * R.TILE_FLOATS, need, need - 1, MB32):
                            for cells in ((0, 1) if tile == 16 and slab in (0, MB32) else (0,)):
                                rc, pl = _query(lib, mtiles, 128 * ntiles, nk, n_cu, slab=slab, tile=tile, cells=cells)
                                want = R.tail_ksplit(mtiles, nt_t, nks, n_cu, slab, bn=bn, compute_waves=cw, tail_env=tail_env)
                                deep = R.deep_ring(mtiles, nt_t, nk, n_cu, dma=bool(pl.dma)) and tile == 16
                                check(("fp32", n_cu, mtiles, ntiles, nk, tile, slab, cells),
                                      (rc, pl.tile, pl.family, pl.mtiles, pl.ntiles, pl.tail_ksplit, pl.n_main, pl.grid, pl.st_gn, pl.cs, pl.dma, pl.deep),
                                      (0, tile, 2, mtiles, nt_t, *want, 0, cells, cells, int(deep)))
                    # -- H2 in and out (tile 16; a 1 x M frame is too wide for the halo ring, so 3 x 3 layers take the per-tap loaders)
                    for slab in (0, MB32):
                        rc, pl = _query(lib, mtiles, 128 * ntiles, nk, n_cu, slab=slab, fmt=(1, 1, 1))
                        ks, n_main, grid = R.tail_ksplit(mtiles, ntiles, nk, n_cu, slab, cells_in=True, halo=pl.mode == 3, tail_env=tail_env)
                        gn, mc, mb, st_grid = R.supertile(mtiles, ntiles, nk, 128 * ntiles, True, True, tail_ks=ks)
                        deep = R.deep_ring(mtiles, ntiles, nk, n_cu, dma=bool(pl.dma))
                        check(("H2", n_cu, mtiles, ntiles, nk, slab),
                              (rc, pl.tile, pl.mtiles, pl.ntiles, pl.tail_ksplit, pl.n_main, pl.grid, pl.st_gn, pl.st_mc, pl.st_mb, pl.ah2, pl.oh2, pl.h1, pl.cs, pl.dma, pl.deep),
                              (0, 16, mtiles, ntiles, ks, n_main, st_grid if gn else grid, gn, mc, mb, 1, 1, 0, 1, 1, int(deep)))
                    # -- H2 in, fp32 out: pointwise layers only
                    rc, pl = _query(lib, mtiles, 128 * ntiles, nk, n_cu, slab=MB32, fmt=(1, 0, 0))
                    if KERNEL_OF_NK[nk][:2] != (1, 1):
                        check(("H2 -> fp32 refused", n_cu, mtiles, ntiles, nk), rc, -2)
                    else:
                        want = R.tail_ksplit(mtiles, ntiles, nk, n_cu, MB32, cells_in=True, tail_env=tail_env)
                        check(("H2 -> fp32", n_cu, mtiles, ntiles, nk), (rc, pl.tail_ksplit, pl.n_main, pl.grid, pl.st_gn, pl.ah2, pl.oh2), (0, *want, 0, 1, 0))
                    # -- H1 in and out: never a split tail (the kernels see half the K-steps: two halves per 4-byte unit)
                    if KERNEL_OF_NK[nk][2] % 64 == 0 and nk % 2 == 0:
                        rc, pl = _query(lib, mtiles, 128 * ntiles, nk, n_cu, slab=MB32, fmt=(2, 2, 2))
                        check(("H1", n_cu, mtiles, ntiles, nk), (rc, pl.tail_ksplit, pl.n_main, pl.h1, pl.deep), (0, 0, mtiles * ntiles, 1, 0))
    return bad, n


def test_plan_query_matches_the_restated_grid_rules(lib_built):
    """The sweep of the module docstring with the switches at their defaults: cell inputs never split their tail."""
    from deepgraphpose_amd import _lib
    bad, n = _sweep(_lib.load(), tail_env=1)
    assert not bad and n > 100000, (n, bad[:5])


def test_plan_query_matches_the_restated_grid_rules_with_the_tail_split_forced_on_cells(lib_built):
    """DGP_TAIL_SPLIT=2 (read once per process: a child) lets cell inputs split; everything else as before."""
    env = dict(os.environ, DGP_TAIL_SPLIT="2", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "2"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sweep ok" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


# ---------------------------------------------------------------- the halo walk: 3 x 3 layers on real N x H x W frames
def _widths(d):
    """W = 1, 2, a small one, and the last fit / first miss of both capacity bounds at dilation d (worked out here, not read from the code):
    default S = 128 + 2 d (W + 1) <= 360 <=> W <= 116 // d - 1; hard d (W - 2) + 128 <= 352 <=> W <= 224 // d + 2"""
    w_def, w_hard = 116 // d - 1, 224 // d + 2
    assert 128 + 2 * d * (w_def + 1) <= 360 < 128 + 2 * d * (w_def + 2) and d * (w_hard - 2) + 128 <= 352 < d * (w_hard - 1) + 128
    return (1, 2, 9, w_def, w_def + 1, w_hard, w_hard + 1)


def _frames_for(mtiles, W):
    """(N, H) with ceil(N H W / 128) == mtiles where some H in 1 .. 40 allows it, else the nearest count from below"""
    for H in (7, 5, 3, 1, 2, 4, 6) + tuple(range(8, 41)):
        N = mtiles * 128 // (H * W)
        if N >= 1 and -(-N * H * W // 128) == mtiles:
            return N, H
    return max(1, mtiles * 128 // W), 1


def _halo_sweep(lib, halo_env, tail_env=1):
    """every mismatch between the query and the restatement on 3 x 3 layers, the number of plans compared, and how many took each path"""
    from deepgraphpose_amd import _lib
    bad, n, seen = [], 0, {"walk": 0, "deep": 0, "per_tap": 0}
    for n_cu in (64, 104, 256, 304):
        for fmt in (1, 2):
            for d in (1, 2, 3):
                for W in _widths(d):
                    for cin in ((32, 128, 512) if fmt == 1 else (64, 128, 512)):
                        for cout in (64, 128, 512):
                            bn = 128 if cout >= 128 else 64
                            ntiles = cout // bn
                            for mt in sorted({1, 3, n_cu // ntiles - 1, n_cu // ntiles, n_cu // ntiles + 1, 2 * n_cu // ntiles + 3, 5 * n_cu // ntiles + 1} - {0, -1}):
                                N, H = _frames_for(mt, W)
                                mtiles = -(-N * H * W // 128)
                                for pad_l, stride, slab in ((d, 1, 0), (d, 1, MB32), (d + 1, 1, 0), (d, 2, 0)):
                                    Ho = H if stride == 1 else (H - 1) // 2 + 1
                                    Wo = W + 2 * (pad_l - d) if stride == 1 else (W - 1) // 2 + 1
                                    dsc = _lib.DgpConvDesc(N, H, W, cin, cout, 3, 3, stride, d, d, pad_l, Ho, Wo, 1, 0, 0, 0)
                                    pl = _lib.DgpConvPlan()
                                    rc = lib.dgp_conv2d_plan(C.byref(dsc), fmt, fmt, 0, 1, 0, slab, -1, n_cu, C.byref(pl))
                                    mo = -(-N * Ho * Wo // 128)
                                    nk = 9 * cin // 32
                                    deep = bn == 128 and R.deep_ring(mo, ntiles, nk, n_cu, dma=True, h1=fmt == 2)
                                    halo = R.halo_walk(fmt, fmt, (3, 3), stride, d, d, pad_l, (H, W), (Ho, Wo), dma128=bn == 128, deep=deep, halo_env=halo_env)
                                    ks, n_main, grid = R.tail_ksplit(mo, ntiles, nk, n_cu, slab, cells_in=True, h1=fmt == 2, halo=halo, bn=bn, tail_env=tail_env)
                                    got = (rc, pl.tile, pl.mode, pl.deep, pl.lds, pl.mtiles, pl.ntiles, pl.tail_ksplit, pl.n_main, pl.grid, pl.st_gn, pl.dma, pl.h1)
                                    want = (0, 16 if bn == 128 else 15, 3 if halo else 1, int(deep), R.dma_lds_bytes(halo, deep, bn), mo, ntiles, ks, n_main, grid, 0, 1, int(fmt == 2))
                                    n += 1
                                    seen["walk" if halo else "deep" if deep else "per_tap"] += 1
                                    assert not (halo and (ks or deep))
                                    if got != want and len(bad) < 20:
                                        bad.append(((n_cu, fmt, d, N, H, W, cin, cout, pad_l, stride, slab), got, want))
    return bad, n, seen


def _halo_sweep_ok(bad, n, seen, halo_env):
    """nothing differs and the sweep reached every path it is about (no walk at all with the switch off)"""
    return not bad and n > 20000 and seen["deep"] > 500 and seen["per_tap"] > 5000 and (seen["walk"] > 3000 if halo_env else seen["walk"] == 0)


def test_plan_query_matches_the_restated_halo_rule(lib_built):
    """3 x 3 layers of both cell formats on N x H x W frames, dilation 1 / 2 / 3, widths 1, 2 and on each side of both capacity bounds,
    one and several channel chunks, 64 / 128 / 512 output channels, tile counts on each side of n_cu, with and without a slab, and beside
    each stride-1 layer one with another pad and a stride-2 one: mode, deep, lds, tail_ksplit, n_main and grid against the restatement."""
    from deepgraphpose_amd import _lib
    bad, n, seen = _halo_sweep(_lib.load(), halo_env=1)
    print("[conv-plan] halo sweep: %d plans, %r" % (n, seen))
    assert _halo_sweep_ok(bad, n, seen, 1), (n, seen, bad[:5])


@pytest.mark.parametrize("halo_env", [0, 2])
def test_plan_query_matches_the_restated_halo_rule_with_the_switch_set(lib_built, halo_env):
    """DGP_HALO=0 (no walk anywhere) and DGP_HALO=2 (the default capacity bound lifted, the hard one kept), read once per process: a child"""
    env = dict(os.environ, DGP_HALO=str(halo_env), PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "halo"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout[-500:])
    assert r.returncode == 0 and "halo sweep ok" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


def _plan(**kw):
    from deepgraphpose_amd import engine
    return engine.conv2d_plan(**kw)


def _c3(nhw, cin, cout, d, fmt, n_cu=256):
    return _plan(x_shape=tuple(nhw) + (cin,), w_shape=(3, 3, cin, cout), rate=d, pad_t=d, pad_l=d, in_fmt=fmt, out_fmt=fmt, n_cu=n_cu)


# 3 x 3, 128 -> 512 at 256 CUs, more than 256 tiles: (dilation, (N, H, W)) -> mode at the default switches, mode under DGP_HALO=2
HALO_KNOWN = [
    (1, (15, 5, 115), 3, 3), (1, (15, 5, 116), 1, 3),         # default capacity at d 1: S = 360 / 362
    (2, (30, 5, 57), 3, 3), (2, (30, 5, 58), 1, 3),           # ... at d 2: S = 360 / 364
    (1, (8, 5, 226), 1, 3), (1, (8, 5, 227), 1, 1),           # hard capacity at d 1: d (W - 2) + 128 = 352 / 353
    (2, (15, 5, 114), 1, 3), (2, (15, 5, 115), 1, 1),         # ... at d 2: 352 / 354
    (3, (6, 33, 47), 1, 3),                                   # S = 416, d (W - 2) + 128 = 263
    (1, (171, 25, 2), 3, 3), (1, (171, 50, 1), 1, 1),         # two pixels per row; one
    (1, (140, 7, 9), 3, 3),                                   # frames smaller than a tile
]


def _halo_known(halo_env):
    """the table above and the ResNet-101 layer through the query, both cell formats -> the rows that differ"""
    bad = []
    for fmt in (1, 2):
        rows = HALO_KNOWN + [(2, (16, 45, 80), 1, 3)]
        for d, nhw, m_def, m_forced in rows:
            cin, cout = (512, 512) if nhw[1:] == (45, 80) else (128, 512)
            pl = _c3(nhw, cin, cout, d, fmt)
            want = dict(mode=(1, m_def, m_forced)[halo_env], deep=0, tail_ksplit=0, st_gn=0, h1=int(fmt == 2), tile=16)
            if pl["mtiles"] * pl["ntiles"] <= 256 or {k: pl[k] for k in want} != want:
                bad.append((fmt, d, nhw, pl, want))
    return bad


def test_known_halo_plans_at_256_cus(lib_built):
    """Each side of both capacity bounds, dilation 3, narrow rows and tiny frames as literal answers, H2 and H1 alike.  With at most
    one tile per CU every H2 row is on the deep ring instead; H1 keeps the walk."""
    assert not _halo_known(1), _halo_known(1)[:3]
    for d, nhw, m_def, _ in HALO_KNOWN:
        small = (max(1, nhw[0] // 8),) + nhw[1:]
        _expect(_c3(small, 128, 512, d, 1), mode=1, deep=1, lds=147456, tail_ksplit=0)
        _expect(_c3(small, 128, 512, d, 2), mode=m_def, deep=0, lds=81920, tail_ksplit=0, h1=1)


def test_the_networks_3x3_layers_at_256_cus(lib_built):
    """ResNet-50 at 640 x 480: block2 / 3 / 4 conv2 (60 x 80 x 128, 30 x 40 x 256, 30 x 40 x 512 at dilation 2) walk the ring at batch 32 on
    both tiers; at batch 4 (150 / 76 / 152 tiles) the parity tier runs them on the deep ring with the per-tap loaders, the 16-bit tier
    still on the walk.  ResNet-101 at 1280 x 720 x 16: block4 conv2 (45 x 80 at dilation 2, S = 452) keeps the per-tap loaders."""
    layers = (((60, 80), 128, 1), ((30, 40), 256, 1), ((30, 40), 512, 2))
    for hw, c, d in layers:
        for fmt in (1, 2):
            _expect(_c3((32,) + hw, c, c, d, fmt), mode=3, deep=0, lds=81920, tail_ksplit=0, st_gn=0, grid=32 * hw[0] * hw[1] // 128 * (c // 128))
        _expect(_c3((4,) + hw, c, c, d, 1), mode=1, deep=1, lds=147456)
        _expect(_c3((4,) + hw, c, c, d, 2), mode=3, deep=0, h1=1)
    for fmt in (1, 2):
        _expect(_c3((16, 45, 80), 512, 512, 2, fmt), mode=1, deep=0, grid=1800)


def _expect(pl, **want):
    got = {k: pl[k] for k in want}
    assert got == want, (got, want)


def test_literal_plans_at_256_cus(lib_built):
    """The plans tests/test_conv_plan_gpu.py is about, as numbers (256 CUs, slots = 512), evaluated by hand from the rules:
    T1 130 x 4 = 520 tiles, rem 8, ks 4 -> grid 512 + 32; T2 178 x 4 = 712, rem 200, ks 2 -> 512 + 400; T3 513 x 1, nk 18: ks 3 (18 % 4 != 0),
    on the K16 tile 36 steps: ks 4; T4 the four ways not to split; T4b two rounds at K = 2048; S1 / S2 the supertile orders; the deep ring."""
    M1 = 13 * 31 * 41
    pw = lambda m, cin, cout: dict(x_shape=(1, 1, m, cin), w_shape=(1, 1, cin, cout), n_cu=256)
    for tile, name in ((16, "splith3_128x128_k32"), (13, "splith3_128x128_k16"), (10, "split6_128x128_k16"), (11, "split3_128x128_k16"),
                       (7, "split6_128x128_k32"), (8, "split3_128x128_k32")):
        _expect(_plan(**pw(M1, 512, 512), slab_bytes=MB32, tile=tile), tile=tile, family=2, mode=2, mtiles=130, ntiles=4, tail_ksplit=4,
                n_main=512, grid=544, st_gn=0, kernel_name=name)
    _expect(_plan(**pw(178 * 128 - 5, 256, 512), slab_bytes=MB32), tile=16, mtiles=178, tail_ksplit=2, n_main=512, grid=912)
    assert R.tail_slab_bytes(200, 2) == 26214400
    _expect(_plan(**pw(178 * 128 - 5, 256, 512), slab_bytes=26214400 - 1), tail_ksplit=0, n_main=712, grid=712)
    t3 = dict(x_shape=(1, 171, 384, 64), w_shape=(3, 3, 64, 128), pad_t=1, pad_l=1, n_cu=256, slab_bytes=MB32)      # M = 65664 = 513 x 128
    _expect(_plan(**t3), tile=16, mode=1, mtiles=513, ntiles=1, tail_ksplit=3, n_main=512, grid=515)
    _expect(_plan(**t3, tile=10), tile=10, mode=1, tail_ksplit=4, n_main=512, grid=516)
    # T4: no split although the slab is there
    _expect(_plan(**pw(M1, 128, 512), slab_bytes=MB32), tail_ksplit=0, n_main=520, grid=520)                      # 4 K-steps: parts below 4
    _expect(_plan(**pw(258 * 128 - 9, 512, 512), slab_bytes=MB32), mtiles=258, tail_ksplit=0, grid=1032)           # two rounds, 16 K-steps
    _expect(_plan(**pw(769 * 128 - 9, 512, 128), slab_bytes=MB32), mtiles=769, ntiles=1, tail_ksplit=0, grid=769)  # rem 257: ks would be 1
    _expect(_plan(**pw(M1, 512, 512), slab_bytes=R.tail_slab_bytes(8, 4) - 1), tail_ksplit=0, grid=520)
    _expect(_plan(**pw(M1, 512, 512), slab_bytes=R.tail_slab_bytes(8, 4)), tail_ksplit=4, grid=544)
    _expect(_plan(**pw(M1, 512, 512)), tail_ksplit=0, grid=520)                                                    # no slab: today's entry points
    # T4b: the same two rounds at K = 2048 (64 K-steps)
    _expect(_plan(**pw(258 * 128 - 9, 2048, 512), slab_bytes=MB32), tail_ksplit=4, n_main=1024, grid=1056)
    # cells: the split stays off unless forced
    h2 = dict(in_fmt=1, out_fmt=1)
    _expect(_plan(**pw(32 * 30 * 40, 1024, 256), **h2, slab_bytes=MB32), mtiles=300, ntiles=2, tail_ksplit=0, grid=600, cs=1, dma=1, ah2=1, oh2=1)
    # S1 / S2 / S3: supertile order and the plain order beside each predicate
    _expect(_plan(**pw(67 * 128 - 50, 1024, 1024), **h2, res_stride=1, res_hw=(1, 67 * 128 - 50), res_fmt=1), mtiles=67, ntiles=8, st_gn=2,
            st_mc=8, st_mb=9, grid=576, tail_ksplit=0)
    _expect(_plan(**pw(8192, 512, 2048), **h2), mtiles=64, ntiles=16, st_gn=4, st_mc=8, st_mb=8, grid=1024)
    _expect(_plan(**pw(63 * 128 - 50, 1024, 1024), **h2), mtiles=63, st_gn=0, grid=504)                 # 63 row tiles
    _expect(_plan(**pw(67 * 128 - 50, 512, 1024), **h2), st_gn=0, grid=536)                            # a 2-MiB panel
    _expect(_plan(**pw(67 * 128 - 50, 2048, 512), **h2), ntiles=4, st_gn=0, grid=268)                  # 4 column tiles
    _expect(_plan(**pw(67 * 128 - 50, 1024, 1024), in_fmt=1, out_fmt=0), st_gn=0, grid=536)            # fp32 out
    # deep ring: at most one tile per CU
    _expect(_plan(**pw(64 * 128 - 3, 256, 512), **h2), mtiles=64, ntiles=4, deep=1, lds=147456, grid=256)
    _expect(_plan(**pw(65 * 128 - 3, 256, 512), **h2), mtiles=65, deep=0, lds=81920, grid=260)
    _expect(_plan(**pw(8 * 128 - 3, 128, 512), **h2), deep=0)                                          # 4 K-steps: below 6
    # the halo walk (3 x 3, stride 1, cells) never splits
    _expect(_plan(x_shape=(2, 30, 40, 256), w_shape=(3, 3, 256, 256), pad_t=1, pad_l=1, n_cu=8, slab_bytes=MB32, **h2), mode=3, tail_ksplit=0)


def test_fallbacks_families_and_the_device_default(lib_built):
    pw = lambda m, cin, cout: dict(x_shape=(1, 1, m, cin), w_shape=(1, 1, cin, cout), n_cu=256)
    # Cin < 32: the per-lane tap kernel of the tile's fp32 stand-in
    _expect(_plan(**pw(1000, 16, 128), tile=16), tile=0, family=0, mtiles=8, ntiles=1, grid=8, kernel_name="f32")
    _expect(_plan(**pw(1000, 16, 64)), tile=1, family=0, ntiles=1, grid=8)
    _expect(_plan(**pw(1000, 16, 24)), tile=3, family=0, ntiles=1, grid=8)
    # the fp32 families report tile, family and grid
    _expect(_plan(**pw(1000, 64, 256), tile=6), tile=6, family=1, mtiles=8, ntiles=4, grid=32, tail_ksplit=0)
    _expect(_plan(**pw(1000, 64, 256), tile=4), tile=4, family=0, mtiles=8, ntiles=2, grid=16)
    _expect(_plan(**pw(1000, 64, 256), tile=99), tile=0, family=0, grid=16)                            # unknown id
    # pick_tile: ranges -> the fp16 tiles, none -> bf16
    _expect(_plan(**pw(1000, 64, 256)), tile=16)
    _expect(_plan(**pw(1000, 64, 64)), tile=15, ntiles=1)
    _expect(_plan(**pw(1000, 64, 256), ranged=False), tile=10)
    # n_cu = 0: the current device's count (256 where there is none to ask)
    assert _plan(x_shape=(1, 1, 1000, 64), w_shape=(1, 1, 64, 256))["n_cu"] > 0


def test_what_the_kernels_refuse_is_refused_by_the_query(lib_built):
    from deepgraphpose_amd import _lib
    pw = lambda m, cin, cout: dict(x_shape=(1, 1, m, cin), w_shape=(1, 1, cin, cout), n_cu=256)
    c3 = dict(x_shape=(1, 20, 24, 64), w_shape=(3, 3, 64, 128), pad_t=1, pad_l=1, n_cu=256)
    refused = [
        dict(**pw(1000, 64, 256), ranged=False, tile=16),             # fp16 split without the operand ranges
        dict(**pw(1000, 64, 256), in_fmt=1, out_fmt=1, tile=10),      # cells on a tile without the compute-side split
        dict(**pw(1000, 64, 64), tile=16),                            # a 64-column panel on a 128-column tile
        dict(**pw(1000, 64, 64), tile=5),                             # ... on the loader-specialised 128 x 128 tile
        dict(**c3, in_fmt=1, out_fmt=0),                              # fp32 out of cells: pointwise layers only
        dict(**c3, in_fmt=2, out_fmt=0),
    ]
    for kw in refused:
        with pytest.raises(_lib.DgpError, match=r"\(-2\).*invalid argument"):
            _plan(**kw)
    invalid = [
        dict(**pw(1000, 96, 256)),                                    # Cin not 4 * 2^k
        dict(**pw(1000, 64, 250)),                                    # Cout % 4
        dict(**pw(1000, 16, 256), in_fmt=1, out_fmt=1),               # cells: Cin >= 32
        dict(**pw(1000, 32, 256), in_fmt=2, out_fmt=2),               # H1: Cin % 64
        dict(**pw(1000, 64, 256), in_fmt=0, out_fmt=1),               # cells out of fp32
        dict(**pw(1000, 64, 256), in_fmt=1, out_fmt=2),               # two kinds of cells
        dict(**pw(1000, 64, 256), in_fmt=1, out_fmt=0, res_stride=1, res_hw=(1, 1000), res_fmt=1),      # H2 residual into an fp32 output
        dict(**pw(1000, 64, 256), slab_bytes=1 << 32),                # a slab beyond ConvArgs::slab_bytes
        dict(pw(1000, 64, 256), n_cu=-1),
    ]
    for kw in invalid:
        with pytest.raises(_lib.DgpError, match=r"\(-1\)"):
            _plan(**kw)


if __name__ == "__main__":
    from deepgraphpose_amd import _lib as _l
    if sys.argv[1] == "halo":          # the halo sweep and the known answers under this process's DGP_HALO
        henv = int(os.environ.get("DGP_HALO", "1"))
        bad_, n_, seen_ = _halo_sweep(_l.load(), halo_env=henv)
        known_ = _halo_known(henv)
        ok_ = _halo_sweep_ok(bad_, n_, seen_, henv) and not known_
        print("halo sweep ok: %d plans, %r" % (n_, seen_) if ok_ else "halo sweep FAILED: %d plans, %r, %r, %r" % (n_, seen_, bad_[:5], known_[:3]))
        sys.exit(0 if ok_ else 1)
    bad_, n_ = _sweep(_l.load(), tail_env=int(sys.argv[1]))
    print("sweep ok: %d plans" % n_ if not bad_ and n_ > 100000 else "sweep FAILED: %d plans, %r" % (n_, bad_[:5]))
    sys.exit(1 if bad_ else 0)
