"""Layer-level tests of the root block (conv 7x7 / 2 + BN + ReLU + max-pool 3x3 / 2): the pool's FIRST-MAXIMUM record and its consumers.

Three kernels write or read the record and none of them was compared with a reference as a layer: maxpool_fwd_idx_kernel and
maxpool_bwd_idx_kernel (the parity tier's training step) and stem_pool_fused_kernel (the root block of every 16-bit training step and of
both tiers' inference).  The whole-step tests dither their frames so that no pool window ties -- rightly, a tie between identical patches
cannot change a weight gradient -- so "strictly greater: the first maximum stays" was claimed in three places and checked in none.

  (a) maxpool_fwd_idx / maxpool_bwd_idx are EXACT: pool values, records, the H1 copy and the routed gradient bit for bit on hand-made maps
      (plateaus, plateaus across window borders, +0 / -0, all-negative, -inf, whole windows of -inf, subnormals; hand-made records, the
      all-zero record that names positions outside the map on padded grids).
  (b) the fused kernel's pool cells against tests/_h1_ref.root_forward (float64 on the cells the kernel holds) in its three reachable
      modes: H2 cells (parity tier inference, <false> instantiation), H1 cells at a fixed scale (16-bit inference, <true>), H1 cells at a
      predicted scale with the record (the training step).  Bounds, none tuned to the code under test, in scaled units:
        H1   |cell - ref| <= 2^-11 |ref| + 2^-25 + 1e-5 max |ref|          (_h1_excess of test_backward_layers_h1_gpu.py)
        H2   |cell - ref| <= max(2^-22 |ref|, 2^-33 max |ref|) + 1e-5 max |ref|   (test_h2_gpu.py's 22 bits + the accumulation bound)
      cells exactly 0 where the reference maximum is 0; tracked maximum within 1e-5.
  (c) the fused record, window by window, with b = (b)'s bound at the window's maximum: dead window -> 0; positive window -> a position
      inside the map whose reference value is within 2 b of the maximum; decisive window (the maximum leads by more than 2 b) -> the
      arg-max; exact tie (bitwise equal maximal set: identical patches, leading by more than 2 b) -> the FIRST of the set.  Windows that
      are neither decisive nor exact ties are capped at 2 % of the positive ones, asserted from the reference alone.
  (d) the unfused path (engine.conv2d + maxpool_fwd_idx) under the same rule with the fp32 bound, and the two dead-window conventions by
      name: the unfused kernel records the first VALID position, the fused kernel records 0.
Frames: uniform uint8 ("random") and constant 16 x 16 blocks, some forced to 0 and 255 ("blocky": asserted from the reference to give
>= 25 % exact ties among the positive windows, >= 10 % dead and >= 10 % positive windows).

Inputs are drawn on the host, so every machine tests the same frames and the preconditions above do not depend on the device's generator.

Measured on the MI355X (worst over the cases; every test prints its figures before it asserts; EXPERIMENTS.md RB has the table):
  (a) pool values, records, H1 copies, routed gradients    bit-identical
  (b) |err| / bound: H2 fixed 0.031, H1 fixed 0.959, H1 predicted + record 0.962 (the H1 bound's half ulp IS the cell's rounding);
      tracked maximum 2.0e-7 (H2) / 7.6e-8 (H1) relative (bound 1e-5); every cell exactly 0 where the reference maximum is 0
  (c) no violation; undecided windows 0.0017-0.0029 of the positive ones (cap 0.02), exact ties 0.66-0.71 on blocky frames, dead 0.35-0.57
  (d) unfused conv1 4.3e-7 of the range (bound 1e-5); no violation; undecided 0-0.0006
  persistent loop: 33 tiles per frame x 16 frames = 528 on a grid of 512 (16-bit kernel), 21 x 13 = 273 on 256 (parity kernel)
No kernel or launcher fault was found: all 92 cases passed on the first run of the code under test.
That the comparisons bite was checked once against builds with five value-only faults: `>=` for `>` in the fused record (every (c) case
fails: blocky by the ties, random by the dead windows), `>=` for `>` in maxpool_fwd_idx_kernel (every (a) forward case but "random", the
backward cases on the forward record, every (d) case), the fused record written to channel group 7 - cg and the record of the last pool
column not stored (every (c) case each), maxpool_bwd_idx_kernel walking window columns before rows (the "shared" record case on every
grid, bit-exactly: the fp32 sums of four windows differ).
"""
import ctypes

import numpy as np
import pytest
import torch

import _h1_ref as R

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
MEAN = (123.68, 116.779, 103.939)
# (H, W) -> conv1 17 x 33 (pool padding 1 / 1, ragged last tile row and column in both tilings), 32 x 48 (padding 0 / 0),
# 38 x 51 (padding 0 / 1), 16 x 16 (one partial tile)
FRAMES = [(33, 65), (64, 96), (75, 101), (32, 32)]
GRIDS = [((H + 1) // 2, (W + 1) // 2) for H, W in FRAMES]
KINDS = ["random", "blocky"]
BIG = (128, 160)          # the persistent-loop case: conv1 64 x 80, pool 32 x 40
DEV = "cuda"
_WORST = {}
_MEMO = {}


def _note(group, value):
    _WORST[group] = max(_WORST.get(group, 0.0), value)
    print("measured %s: %.3g (worst so far %.3g)" % (group, value, _WORST[group]))


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _frames(kind, B, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * H + W + 7 * B + seed)          # drawn on the host: the same frames on every machine
    if kind == "random":
        return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    bh, bw = (H + 15) // 16, (W + 15) // 16
    col = torch.randint(0, 256, (B, bh, bw, 3), generator=g)
    u = torch.rand((B, bh, bw, 1), generator=g)
    col = torch.where(u < 0.15, torch.zeros_like(col), torch.where(u > 0.85, torch.full_like(col, 255), col))
    return col.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].to(torch.uint8).contiguous().to(DEV)


def _weights():
    """Random weights; BN biases spread over the range of the conv1 values so that whole channels are mostly dead and others mostly alive."""
    def make():
        g = torch.Generator().manual_seed(4711)
        w = torch.randn((7, 7, 3, 64), generator=g) * 0.05
        sc = torch.rand(64, generator=g) + 0.5
        bi = torch.randn(64, generator=g) * 60.0 - 30.0
        return w.to(DEV), sc.to(DEV), bi.to(DEV)
    return _memo("weights", make)


def _case(frame, kind, B=2):
    return _memo(("frames", frame, kind, B), lambda: _frames(kind, B, *frame))


def _ref(frame, kind, cells, B=2):
    """(conv1 map, pool maxima) of the float64 root block, unscaled; computed once per case and never modified."""
    w, sc, bi = _weights()
    return _memo(("ref", frame, kind, cells, B), lambda: R.root_forward(_case(frame, kind, B), w, sc, bi, MEAN, cells))


def _h1_bound(ref_scaled, top):
    return 2.0 ** -11 * ref_scaled.abs() + 2.0 ** -25 + REL_TOL * top


def _h2_bound(ref_scaled, top):
    return torch.clamp(2.0 ** -22 * ref_scaled.abs(), min=2.0 ** -33 * top) + REL_TOL * top


def _f32_bound(ref_scaled, top):
    return torch.zeros_like(ref_scaled) + REL_TOL * top


def _h2_values(cells):
    """H2 cells (fp32-typed [..., 64]) -> high + low in scaled units, float64."""
    h = cells.contiguous().view(torch.float16).reshape(cells.shape[:-1] + (8, 2, 8)).double()
    return (h[..., 0, :] + h[..., 1, :]).reshape(cells.shape)


def _window_classes(c1_scaled, bound):
    """From the reference alone: per window and channel (values [9, ...] with -inf outside the map, maximum, first arg-max, classes).
    decisive: the maximum leads every other element by more than 2 b; tie: the maximal set is bitwise equal, has more than one member and
    leads the rest by more than 2 b; positive / dead by the sign of the maximum."""
    r = torch.stack(R.pool_windows(c1_scaled))
    top = r.amax(0)
    b2 = 2.0 * bound(top, float(c1_scaled.max()))
    is_max = r == top
    first = is_max.to(torch.uint8).argmax(0).to(torch.uint8)
    rest = torch.where(is_max, torch.full_like(r, -float("inf")), r).amax(0)
    lead = rest < top - b2
    n_max = is_max.sum(0)
    positive = top > 0
    return dict(r=r, top=top, first=first, b2=b2, positive=positive, dead=~positive, decisive=positive & lead & (n_max == 1),
                tie=positive & lead & (n_max > 1))


def _shares(cls, kind, what):
    """The preconditions, from the reference alone; prints them."""
    n, npos = cls["top"].numel(), int(cls["positive"].sum())
    dead, tie = int(cls["dead"].sum()) / n, int(cls["tie"].sum()) / max(npos, 1)
    undecided = 1.0 - (int(cls["decisive"].sum()) + int(cls["tie"].sum())) / max(npos, 1)
    print("%s (%s): %d windows, positive %.3f, dead %.3f, exact ties %.3f and undecided %.5f of the positive ones"
          % (what, kind, n, npos / n, dead, tie, undecided))
    _note("undecided share, %s frames" % kind, undecided)
    assert undecided <= 0.02, (what, undecided)
    assert npos / n >= 0.10 and dead > 0.0, (what, npos / n, dead)
    if kind == "blocky":
        assert tie >= 0.25 and dead >= 0.10, (what, tie, dead)
    return undecided


def _check_record(rec, gpu_positive, cls, H1, W1, what):
    """(c)'s rule.  gpu_positive: the GPU's own pool value is > 0."""
    valid = R.pool_valid(H1, W1, rec.device)[:, None, :, :, None].expand_as(cls["r"])
    k = rec.long()
    assert int(k.max()) <= 8, what
    r_k = torch.gather(cls["r"], 0, k[None])[0]
    inside = torch.gather(valid, 0, k[None])[0]
    pos = gpu_positive
    assert bool((inside | ~pos).all()), "%s: %d positive windows name a position outside the map" % (what, int((pos & ~inside).sum()))
    weak = r_k >= cls["top"] - cls["b2"]
    assert bool((weak | ~pos).all()), "%s: %d positive windows name an element that is not a maximum" % (what, int((pos & ~weak).sum()))
    for name in ("decisive", "tie"):
        m = cls[name]
        assert bool(pos[m].all()), "%s: a %s window's pool value is not positive" % (what, name)
        bad = int((k != cls["first"].long())[m].sum())
        assert bad == 0, "%s: %d of %d %s windows do not name the first maximum" % (what, bad, int(m.sum()), name)


# ---- (a) the unfused pool and its backward: exact ------------------------------------------------------------------------------
MAPS = ["random", "plateau", "straddle", "zeros", "negative", "neginf", "subnormal"]


def _map(kind, B, H1, W1):
    g = torch.Generator().manual_seed(31 * H1 + W1 + len(kind))
    x = torch.randn((B, H1, W1, 64), generator=g)
    if kind == "plateau":                     # all equal: every window ties on all of its elements
        x = torch.full_like(x, 1.5)
        x[1] = -2.25
    elif kind == "straddle":                  # 5 x 5 plateaus at offsets that put their edges inside, on and across window borders
        lvl = torch.randint(0, 3, (B, (H1 + 4) // 5, (W1 + 4) // 5, 64), generator=g).float()
        x = lvl.repeat_interleave(5, 1).repeat_interleave(5, 2)[:, 1:H1 + 1, 2:W1 + 2].contiguous()
        x[1] = torch.roll(x[1], (1, 1), (0, 1))
    elif kind == "zeros":                     # +0.0 / -0.0 mixtures, some negative values between them
        u = torch.rand(x.shape, generator=g)
        x = torch.where(u < 0.45, torch.zeros_like(x), torch.where(u < 0.9, -torch.zeros_like(x), -x.abs()))
    elif kind == "negative":
        x = -x.abs() - 0.5
        x[1] = torch.round(x[1])              # ... with ties
    elif kind == "neginf":                    # single -inf entries, and whole windows (8 x 8 patches) of -inf
        x[torch.rand(x.shape, generator=g) < 0.3] = -float("inf")
        x[:, :8, :8] = -float("inf")
        x[:, H1 - 7:, W1 - 9:] = -float("inf")
    elif kind == "subnormal":                 # positive subnormals against +0.0 and each other
        n = torch.randint(0, 4, x.shape, generator=g).float()
        x = n * 2.0 ** -149
        x[1] = n[1] * 2.0 ** -140 - 2.0 ** -139
    return x.contiguous().to(DEV)


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("grid", GRIDS)
def test_maxpool_fwd_idx_is_the_first_maximum_bit_for_bit(lib_built, grid, kind):
    from deepgraphpose_amd import engine
    H1, W1 = grid
    x = _map(kind, 2, H1, W1)
    ref, rec_ref = R.pool_first_max(x, first_valid=True)
    if kind in ("plateau", "straddle", "zeros"):          # the case is about ties: most windows must have one
        wins = torch.stack(R.pool_windows(x))
        assert float(((wins == wins.amax(0)).sum(0) > 1).float().mean()) > 0.5
    if kind == "neginf":
        assert int((ref == -float("inf")).sum()) >= 64     # whole windows of -inf
        if R.pool_geometry(H1)[1]:
            assert int(rec_ref[:, 0, 0].min()) == 4        # ... whose first VALID position is not position 0 in the padded corner
    fin = x[torch.isfinite(x)].abs()
    prev = float(fin.max()) * 0.7 if float(fin.max()) > 2.0 ** -100 else 1.0
    for pm in (None, prev):
        pool, rec, cells = engine.maxpool_fwd_idx(x, pm)
        assert torch.equal(_bits32(pool), _bits32(ref)), (grid, kind, int((_bits32(pool) != _bits32(ref)).sum()))
        assert torch.equal(rec, rec_ref), (grid, kind, int((rec != rec_ref).sum()))
        if pm is None:
            assert cells is None
        else:
            s = R.pred_scale(pm)
            assert s > 0
            exp = R.h1(ref, s)
            assert torch.equal(cells.view(torch.int16), exp.view(torch.int16)), (grid, kind, int((cells.view(torch.int16) != exp.view(torch.int16)).sum()))


def _hand_record(kind, B, H1, W1, dev):
    """shared: every window names the pixel it shares with its neighbours, so one conv1 pixel collects four windows; corner: every window
    names its own top-left valid pixel; zero: position 0 everywhere (outside the map in the border windows of a padded grid)."""
    HP, pt = R.pool_geometry(H1)
    WP, pl = R.pool_geometry(W1)
    qy, qx = torch.arange(HP, device=dev), torch.arange(WP, device=dev)
    if kind == "shared":
        a = torch.where((qy % 2 == 1) | (qy == HP - 1), 0, 2)
        b = torch.where((qx % 2 == 1) | (qx == WP - 1), 0, 2)
    elif kind == "corner":
        a, b = torch.clamp(pt - 2 * qy, min=0), torch.clamp(pl - 2 * qx, min=0)
    else:
        a, b = torch.zeros_like(qy), torch.zeros_like(qx)
    rec = (a[:, None] * 3 + b[None, :]).to(torch.uint8)
    return rec[None, :, :, None].expand(B, HP, WP, 64).contiguous()


@pytest.mark.parametrize("record", ["forward", "shared", "corner", "zero"])
@pytest.mark.parametrize("grid", GRIDS)
def test_maxpool_bwd_idx_routes_by_the_record_bit_for_bit(lib_built, grid, record):
    from deepgraphpose_amd import engine
    B, (H1, W1) = 2, grid
    HP, pt = R.pool_geometry(H1)
    WP, pl = R.pool_geometry(W1)
    g = torch.Generator().manual_seed(17 * H1 + W1)          # drawn on the host
    # the gate map: positive values, positive subnormals (open), +0.0, -0.0 and negative values (closed)
    u = torch.randint(0, 5, (B, H1, W1, 64), generator=g)
    c1 = torch.randn((B, H1, W1, 64), generator=g).abs() + 0.1
    c1 = torch.where(u == 1, torch.full_like(c1, 2.0 ** -149), c1)
    c1 = torch.where(u == 2, torch.zeros_like(c1), c1)
    c1 = torch.where(u == 3, -torch.zeros_like(c1), c1)
    c1 = torch.where(u == 4, -c1, c1).contiguous().to(DEV)
    u = u.to(DEV)
    dpool = (torch.randn((B, HP, WP, 64), generator=g) * 1e-3).to(DEV)
    if record == "forward":
        pool, rec, _ = engine.maxpool_fwd_idx(c1)
        assert torch.equal(rec, R.pool_first_max(c1, first_valid=True)[1])
    else:
        rec = _hand_record(record, B, H1, W1, DEV)
    routed = R.pool_backward(dpool, rec, H1, W1, dtype=torch.float32)           # fp32, a pixel's windows in ascending (ho, wo) order
    if record == "shared":
        assert float(R.pool_backward(torch.ones_like(dpool), rec, H1, W1).max()) == 4.0
    inside = torch.gather(R.pool_valid(H1, W1, DEV)[:, None, :, :, None].expand(9, B, HP, WP, 64), 0, rec.long()[None])[0]
    if record == "zero" and (pt or pl):
        assert not bool(inside.all())                                             # the border windows point outside the map
    else:
        assert bool(inside.all())
    kept = float((dpool.double() * inside).sum())
    slack = 4 * 2.0 ** -24 * float(dpool.double().abs().sum())
    # ungated (the 16-bit tier's form)
    got = engine.maxpool_bwd_idx(None, dpool, rec, hw=(H1, W1))
    assert torch.equal(_bits32(got), _bits32(routed)), (grid, record, int((_bits32(got) != _bits32(routed)).sum()))
    assert abs(float(got.double().sum()) - kept) <= slack                         # what points outside the map is dropped, nothing else
    # gated by c1 > 0: a positive subnormal opens the gate, -0.0, 0.0 and negative values close it
    got = engine.maxpool_bwd_idx(c1, dpool, rec)
    exp = torch.where(c1 > 0, routed, torch.zeros_like(routed))
    assert torch.equal(_bits32(got), _bits32(exp)), (grid, record, int((_bits32(got) != _bits32(exp)).sum()))
    sub = (u == 1) & (routed != 0)
    assert int(sub.sum()) > 0 and bool((got[sub] == routed[sub]).all())
    for closed in (2, 3, 4):                                                      # +0.0, -0.0, negative
        m = (u == closed) & (routed != 0)
        # (in the forward pass's own record such a pixel is a first maximum only where a whole window is closed: not on every grid)
        assert int(m.sum()) > 0 or record == "forward", (grid, record, closed)
        assert float(got[m].abs().sum()) == 0.0, (grid, record, closed)
    assert int(((u >= 2) & (routed != 0)).sum()) > 0


# ---- (b) the fused kernel's pool cells against float64 -------------------------------------------------------------------------
MODES = ["h2 fixed", "h1 fixed", "h1 predicted + record"]


def _run(frame, kind, mode, B=2, frames=None):
    """One launch of the fused root block in `mode` -> (cells in scaled units float64, record or None, tracked maximum, scale)."""
    from deepgraphpose_amd import engine
    w, sc, bi = _weights()
    cells = "h2" if mode.startswith("h2") else "h1"
    top = float(_ref(frame, kind, cells, B)[0].max())
    fr = _case(frame, kind, B) if frames is None else frames
    if mode.endswith("record"):
        prev = 0.8 * top                        # "last step's" range of conv1: the scale is predicted from it
        s = R.pred_scale(prev)
        assert R.usable(s, top)
        out, rec, amax = engine.root_block(fr, w, sc, bi, MEAN, cells="h1", prev_max=prev, record=True)
    else:
        e = engine.h2_exp_for(top)
        s = 2.0 ** e
        out, rec, amax = engine.root_block(fr, w, sc, bi, MEAN, cells=cells, out_exp=e)
        assert rec is None
    vals = _h2_values(out) if cells == "h2" else out.double()
    return vals, rec, amax, s


def _check_cells(frame, kind, mode, B=2):
    cells = "h2" if mode.startswith("h2") else "h1"
    c1, pool = _ref(frame, kind, cells, B)
    vals, rec, amax, s = _memo(("run", frame, kind, mode, B), lambda: _run(frame, kind, mode, B))
    ref = pool * s
    top = float(c1.max()) * s
    bound = (_h2_bound if cells == "h2" else _h1_bound)(ref, top)
    assert float(ref.max()) == top and float((ref == 0).float().mean()) > 0.02      # every conv1 pixel lies in a window; dead windows exist
    excess = float(((vals - ref).abs() / bound).max())
    _note("root_block %s |err| / bound" % mode, excess)
    _note("root_block %s tracked maximum, relative error" % mode, abs(amax - float(c1.max())) / float(c1.max()))
    assert excess <= 1.0, (frame, kind, mode, excess)
    assert float(vals[ref == 0].abs().max()) == 0.0, (frame, kind, mode)
    assert abs(amax - float(c1.max())) <= REL_TOL * float(c1.max()), (frame, kind, mode, amax, float(c1.max()))
    # the last pool row and column are compared like the rest; they must hold something to compare
    assert float(ref[:, -1].max()) > 0 and float(ref[:, :, -1].max()) > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_root_block_pool_cells_match_float64(lib_built, frame, kind, mode):
    _check_cells(frame, kind, mode)


def _persistent_batch(mode):
    """The smallest batch of BIG frames whose tiles outnumber the persistent grid (3 x 16 tiles and 2 workgroups per CU for the 16-bit
    tier's kernel, 5 x 16 and 1 for the parity tier's)."""
    ph, per_cu = (5, 1) if mode.startswith("h2") else (3, 2)
    HP, WP = (BIG[0] + 3) // 4, (BIG[1] + 3) // 4
    per_frame = ((HP + ph - 1) // ph) * ((WP + 15) // 16)
    grid = per_cu * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    B = grid // per_frame + 1
    assert B * per_frame > grid                  # a workgroup walks more than one tile: fetch(tile + gridDim.x) runs
    print("persistent loop, %s: %d tiles per frame, batch %d, %d tiles on a grid of %d" % (mode, per_frame, B, B * per_frame, grid))
    return B


@pytest.mark.parametrize("mode", ["h2 fixed", "h1 predicted + record"])
@pytest.mark.parametrize("kind", KINDS)
def test_root_block_persistent_tile_loop(lib_built, kind, mode):
    B = _persistent_batch(mode)
    _check_cells(BIG, kind, mode, B)
    if mode.endswith("record"):
        _check_fused_record(BIG, kind, B)


# ---- (c) the fused record ---------------------------------------------------------------------------------------------------
def _check_fused_record(frame, kind, B=2):
    mode = "h1 predicted + record"
    c1, pool = _ref(frame, kind, "h1", B)
    s = R.pred_scale(0.8 * float(c1.max()))
    cls = _window_classes(c1 * s, _h1_bound)
    _shares(cls, kind, "fused record %s B=%d" % (frame, B))          # from the reference alone, before the GPU is looked at
    vals, rec, _, s2 = _memo(("run", frame, kind, mode, B), lambda: _run(frame, kind, mode, B))
    assert s2 == s
    dead = vals == 0
    assert int(dead.sum()) > 0 and int(rec[dead].max()) == 0, "fused convention: a dead window records position 0"
    _check_record(rec, ~dead, cls, c1.shape[1], c1.shape[2], "fused record %s %s" % (frame, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_fused_record_names_the_first_maximum(lib_built, frame, kind):
    _check_fused_record(frame, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_record_does_not_depend_on_the_batch(lib_built, kind):
    """The same two frames first and last in a batch of 5: the same cells and record."""
    frame, mode = (33, 65), "h1 predicted + record"
    two = _case(frame, kind)
    five = _frames(kind, 5, *frame, seed=99)
    five[0], five[4] = two[0], two[1]
    vals2, rec2, _, _ = _memo(("run", frame, kind, mode, 2), lambda: _run(frame, kind, mode))
    vals5, rec5, _, _ = _run(frame, kind, mode, frames=five.contiguous())
    assert torch.equal(rec5[[0, 4]], rec2)
    assert torch.equal(vals5[[0, 4]], vals2)


def test_root_block_reads_frames_at_any_byte_alignment(lib_built):
    """The batch 1, 2 and 3 bytes into a larger buffer (the fr_delta path; the byte loads at the batch's last bytes): every mode's cells
    and the record are bit-identical to the aligned run."""
    frame, kind = (33, 65), "random"
    fr = _case(frame, kind)
    n = fr.numel()
    for mode in MODES:
        base = _run(frame, kind, mode)
        for off in (1, 2, 3):
            buf = torch.zeros(n + off, dtype=torch.uint8, device=DEV)      # the batch ends with the allocation
            view = buf[off:off + n].view(fr.shape)
            view.copy_(fr)
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            got = _run(frame, kind, mode, frames=view)
            assert torch.equal(got[0], base[0]), (mode, off)
            assert got[2] == base[2], (mode, off)
            if base[1] is not None:
                assert torch.equal(got[1], base[1]), (mode, off)


# ---- (d) the unfused path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_unfused_pool_record_agrees_where_it_must(lib_built, frame, kind):
    from deepgraphpose_amd import engine
    w, sc, bi = _weights()
    fr = _case(frame, kind)
    c1_ref, _ = _ref(frame, kind, "f32")
    H1, W1 = c1_ref.shape[1], c1_ref.shape[2]
    w4 = np.zeros((7, 7, 4, 64), dtype=np.float32)
    w4[:, :, :3] = w.cpu().numpy()
    x = engine.preprocess_u8(fr, MEAN)
    c1 = engine.conv2d(x, w4, stride=2, pad_t=3, pad_l=3, out_hw=(H1, W1), scale=sc, bias=bi, relu=True)
    err = float((c1.double() - c1_ref).abs().max() / c1_ref.max())
    _note("unfused conv1, relative error", err)
    assert err < REL_TOL, (frame, kind, err)
    cls = _window_classes(c1_ref, _f32_bound)
    _shares(cls, kind, "unfused record %s" % (frame,))
    pool, rec, _ = engine.maxpool_fwd_idx(c1)
    assert torch.equal(_bits32(pool), _bits32(R.pool_first_max(c1, first_valid=True)[0]))
    assert torch.equal(rec, R.pool_first_max(c1, first_valid=True)[1])          # exact on its own input
    dead = pool == 0
    corner = _hand_record("corner", fr.shape[0], H1, W1, DEV)
    assert int(dead.sum()) > 0
    assert torch.equal(rec[dead], corner[dead]), "unfused convention: a dead window records its first valid position"
    if R.pool_geometry(H1)[1] or R.pool_geometry(W1)[1]:
        assert int(rec[dead].max()) > 0                                          # ... which is not the fused kernel's 0 on a padded grid
    _check_record(rec, ~dead, cls, H1, W1, "unfused record %s %s" % (frame, kind))


# ---- what the entry points refuse ----------------------------------------------------------------------------------------------
def test_root_block_entry_points_refuse_what_the_trainer_refuses(lib_built):
    from deepgraphpose_amd import _lib, engine
    lib = _lib.load()
    w, sc, bi = _weights()
    fr = _case((32, 32), "random")
    with pytest.raises(_lib.DgpError, match=r"\(-4\).*no predicted range"):      # DGP_ERR_STATE, the trainer's own message
        engine.root_block(fr, w, sc, bi, MEAN, cells="h1", record=True)
    with pytest.raises(_lib.DgpError, match=r"\(-1\)"):                           # the record belongs to the 16-bit tier
        engine.root_block(fr, w, sc, bi, MEAN, cells="h2", prev_max=100.0, record=True)
    t = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    m = (ctypes.c_float * 3)(*MEAN)
    # a frame batch of 2^31 bytes: refused before anything is launched
    assert lib.dgp_root_block(p, 2 ** 15, 256, 256, p, p, p, m, 2, 0, None, None, p, p, p, None) == -1
    assert lib.dgp_root_block(p, 1, 8, 8, None, p, p, m, 2, 0, None, None, p, p, p, None) == -1                  # (null weights)
    # maps that are not those of the root block's pool
    assert lib.dgp_maxpool_fwd_idx(p, 1, 4, 4, 3, 2, None, p, p, None, None) == -1
    assert lib.dgp_maxpool_bwd_idx(None, p, p, 1, 4, 4, 2, 3, p, None) == -1
    assert lib.dgp_maxpool_fwd_idx(p, 1, 4, 4, 2, 2, p, p, p, None, None) == -1          # predicted range without a place for the copy
