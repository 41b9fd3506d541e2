"""The grid rules of the conv launch layer restated in plain Python, from the comments in the launchers (csrc/dgp_kernels.hip, the
launch layer; csrc/dgp_conv_split.hip, the split family's plan) and DESIGN.md ("How a conv launch picks its kernel", "XCD-aware launch order") -- not from the code: tests/test_conv_plan_cpu.py
holds dgp_conv2d_plan to these, tests/test_conv_plan_gpu.py and tests/test_halo_walk_gpu.py build their shapes with them.  Four rules, all on integers:

  grid tail      With two workgroups of a 128 x 128 split kernel per CU, `slots = 2 n_cu` run at once.  A grid of `tiles` leaves
                 `rem = tiles mod slots` tiles for a last, underfull round.  When there is a slab, at least one full round in front
                 and the tail fills at most 3/4 of a round, each tail tile is split over `ks` workgroups: the largest ks <= 4 with
                 rem ks <= slots that divides the K-steps into parts of at least 4.  With two or more full rounds in front, only
                 deep-K layers (>= 48 K-steps) split.  ks = 1 is no split, and so is a slab too small for rem ks raw 128 x 128 tiles.
                 Cell inputs split only when forced (DGP_TAIL_SPLIT=2), H1 cells and the halo walk never; 64-column tiles and the
                 8-wave tiles never.  The grid is then n_main + rem ks workgroups with n_main = tiles - rem.
  supertile      H2 in and out, 128 columns per tile, >= 8 column tiles, >= 64 row tiles, no split tail and a weight panel above
                 3 MiB: column tiles go in groups of gn, the largest power of two that divides the column tiles and keeps the group's
                 weight cells within 1.5 MiB; row tiles in chunks of 8 inside 8 bands of mb = ceil(row tiles / 8); the grid is padded
                 to 8 mb x column tiles.
  deep ring      LDS-DMA launches of the 128 x 128 fp16 tile whose whole grid is at most one tile per CU, with at least 6 K-steps,
                 not H1.
  halo walk      The K loop of a 3 x 3 / stride-1 conv of the cells engine (MODE 3 of conv_igemm_split_ls) streams each channel chunk's
                 strip of S = 128 + 2 d (W + 1) consecutive pixels of the flattened [N H W] list once through a ring of 360 pixels in
                 LDS, d the dilation.  It takes a launch whose cells in and out are of one kind (H2 or H1), 3 x 3, stride 1, pad = d on
                 both axes, output on the input grid, W >= 2, on the 128 x 128 LDS-DMA tile with weight cells, which is not on the deep
                 ring and has no predicted input scale, and whose rows fit the ring twice over: the largest jump between two consecutive
                 K-steps plus a 128-pixel window must leave one 8-pixel group free, d (W - 2) + 128 <= 360 - 8 (the other jump, from
                 one chunk to the next, is 128 plus the strip's padding to 8 pixels and always fits), and by default a whole strip fits
                 the ring, S <= 360 (a longer strip slides through the ring and measured slower: DGP_HALO=2 lifts this bound only).
                 DGP_HALO=0 switches the walk off.  Everything else 3 x 3 takes the per-tap loaders (mode 1).  The walk never splits
                 its tail.  LDS per workgroup: ring + 1 KiB of zeros + 2 KiB of address tables = 48 KiB, two 16-KiB stages of weight
                 cells behind them = 80 KiB; the plain LDS-DMA kernels 3 + 2 stages (80 KiB; 64 KiB on 64 columns), the deep ring
                 5 + 4 (144 KiB)."""

TILE_FLOATS = 128 * 128
MIB = 1 << 20


def tail_ksplit(mtiles, ntiles, nks, n_cu, slab_bytes, cells_in=False, h1=False, halo=False, bn=128, compute_waves=4, tail_env=1):
    """-> (tail_ksplit, n_main, grid).  nks: K-steps of the tile's own depth (32 floats, or 16 on the K16 tiles)"""
    tiles = mtiles * ntiles
    plain = (0, tiles, tiles)
    if tail_env == 0 or (cells_in and tail_env != 2) or h1 or halo or bn != 128 or compute_waves != 4 or slab_bytes <= 0:
        return plain
    slots = 2 * n_cu
    rounds, rem = divmod(tiles, slots)
    if rem == 0 or rounds == 0 or 4 * rem > 3 * slots:
        return plain
    fits = [ks for ks in (2, 3, 4) if rem * ks <= slots and nks % ks == 0 and nks // ks >= 4]
    if not fits or (rounds >= 2 and nks < 48):
        return plain
    ks = max(fits)
    if rem * ks * TILE_FLOATS * 4 > slab_bytes:
        return plain
    return ks, tiles - rem, tiles - rem + rem * ks


def tail_slab_bytes(rem, ks):
    """the smallest slab the split of `rem` tail tiles over ks workgroups needs"""
    return rem * ks * TILE_FLOATS * 4


def supertile(mtiles, ntiles, nk, coutp, cells_in, cells_out, tail_ks=0, bn=128):
    """-> (st_gn, st_mc, st_mb, grid); st_gn = 0 (and grid = None: the tail rule's) where the order stays plain.  nk: 32-float K-steps"""
    panel_bytes = nk * 32 * coutp * 4
    if not (cells_in and cells_out and bn == 128 and tail_ks <= 1 and ntiles >= 8 and mtiles >= 64 and panel_bytes > 3 * MIB):
        return 0, 0, 0, None
    group_bytes = nk * 32 * 128 * 4             # the weight cells one column tile reads
    gn = max(g for g in (1, 2, 4, 8, 16, 32, 64, 128) if g == 1 or (g <= ntiles and ntiles % g == 0 and g * group_bytes <= 3 * MIB // 2))
    mb = -(-mtiles // 8)
    return gn, 8, mb, 8 * mb * ntiles


def deep_ring(mtiles, ntiles, nk, n_cu, dma, h1=False):
    return bool(dma and not h1 and mtiles * ntiles <= n_cu and nk >= 6)


HALO_RING = 360     # pixels


def halo_walk(in_fmt, out_fmt, k, stride, d, pad_t, pad_l, hw, out_hw, dma128, deep, predicted_scale=False, halo_env=1):
    """in_fmt / out_fmt: 0 fp32, 1 H2, 2 H1; k: (KH, KW); d: dilation; dma128: the launch runs the 128 x 128 LDS-DMA tile on weight cells"""
    H, W = hw
    if halo_env == 0 or in_fmt == 0 or in_fmt != out_fmt or not dma128 or deep or predicted_scale:
        return False
    if tuple(k) != (3, 3) or stride != 1 or d < 1 or pad_t != d or pad_l != d or tuple(out_hw) != (H, W) or W < 2:
        return False
    if d * (W - 2) + 128 > HALO_RING - 8:
        return False
    return halo_env >= 2 or 128 + 2 * d * (W + 1) <= HALO_RING


def dma_lds_bytes(halo, deep, bn=128):
    """LDS bytes of an LDS-DMA launch on cells (the K loop's stages; the epilogue's staging tile is smaller)"""
    a_stage, b_stage = 128 * 8 * 16, 2 * 4 * bn * 16
    if halo:
        return HALO_RING * 128 + 1024 + 2048 + 2 * b_stage
    return 5 * a_stage + 4 * b_stage if deep else 3 * a_stage + 2 * b_stage
