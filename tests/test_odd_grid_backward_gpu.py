"""The training step's backward pass on grids that are odd at the stride-2 stages, tensor by tensor against the float64 autograd oracle.

Each frame size runs the chain H -> h1 -> hp -> h2 -> fh (stem, pool, block1, block2: ceil at every halving):
  33 x 65    rows 33 -> 17 -> 9 -> 5 -> 3          columns 65 -> 33 -> 17 -> 9 -> 5      (odd everywhere)
  75 x 101   rows 75 -> 38 -> 19 -> 10 -> 5        columns 101 -> 51 -> 26 -> 13 -> 7    (odd and even mixed)
  747 x 832  rows 747 -> 374 -> 187 -> 94 -> 47    columns all even                      (the Reaching demo's training geometry)
  64 x 96    all even                                                                    (control)
  32 x 32    the smallest frame dgp_net_create accepts (fh = 2)
What depends on that parity lives in the backward pass: the max-pool's SAME padding (1 on top when h1 is odd), the subsample shortcut's
coarse (H + 1) / 2 grid, the zero-stuffed stride-2 data gradient (one row longer than the data on an odd grid), the stem's fused 16-bit
weight gradient (bands of 4 rows, chunks of 32 columns) and the heads' transposed conv on odd feature maps.

With ordinary weights a ReLU whose input is ~1e-7 can land on the other side of zero in fp32 than in float64, and everything upstream of
it then moves by ~1e-3 (test_train_gpu.test_full_backward_matches_autograd): that tolerance would hide a lost boundary row.  The
open-gate weights below have every gated value a clear margin above zero, so no gate can flip and every tensor is held to one tight
bound.  The 747 x 832 cases are the slow ones: their ids contain "747x832".
"""
import numpy as np
import pytest
import torch

from test_train_gpu import _train_case, _oracle_grads, _grad_agreement, _dlc_targets

pytestmark = pytest.mark.gpu

# Per-tensor relative L2 error of every trainable tensor against float64, open-gate weights, parity tier.  Measured worst tensor:
# 64 x 96 (control) 1.9e-6, 33 x 65 2.4e-6, 75 x 101 2.7e-6, 747 x 832 3.9e-6 (stem weights), last-row labels <= 3.2e-6, DLC loss
# <= 3.8e-6; 32 x 32 6.2e-5 (the locref bias: a sum over 2 x 4 x 4 cells that mostly cancels).  A boundary row lost is percents.
BOUND = 1e-4
# 16-bit pass on the same weights: per-tensor relative L2 error, measured worst 1.3e-2 (stem weights at 747 x 832)
BOUND_F16 = 3e-2
MARGIN = 0.05           # every gated value sits at least this far above zero (channel spreads are ~1)
N_TRAINABLE = 53 * 3 + 2 * 2

# (H, W, frames), ids name the frame size
STEP_SHAPES = [pytest.param((33, 65, 3), id="33x65"), pytest.param((75, 101, 3), id="75x101"),
               pytest.param((64, 96, 3), id="64x96"), pytest.param((32, 32, 2), id="32x32"),
               pytest.param((747, 832, 2), id="747x832")]


def _threads():
    torch.set_num_threads(16)


def _net_forward64(w, frames, depth=50, margin=None):
    """The oracle's network (oracle/dgp_train_oracle.network: same ops, same order) in float64 on the float32 weights of `w`.

    margin given: on the way, every BatchNorm's gamma / beta in `w` is rewritten (float32) so that each channel of each gated value
    (the ReLU inputs: stem, conv1, conv2, shortcut + conv3) spans [margin, margin + ~1] over the batch, the shortcut conv's output
    spans [0, 1], and the heads give logits around -4 (spread ~1.5) and locref maps around 0 (spread ~1).
    Returns the smallest gated value, the number of gated tensors and the smallest gap between the two largest values of a pool window."""
    import torch.nn.functional as F
    from oracle import dgp_oracle as O
    from oracle import dgp_train_oracle as T
    from oracle.resnet_plan import units
    t = lambda k: torch.from_numpy(np.asarray(w[k])).double()
    gated = []

    def bn(z, scope, lo=None, base=0.0):
        """BatchNorm of the conv output z; lo given: rescale gamma to a unit spread per channel, then pick beta so that the channel's
        minimum of base + BN(z) over the batch is lo"""
        def scaled():
            inv = t(scope + "/BatchNorm/gamma") * torch.rsqrt(t(scope + "/BatchNorm/moving_variance") + O.BN_EPS)
            return (z - t(scope + "/BatchNorm/moving_mean")[None, :, None, None]) * inv[None, :, None, None]
        y = scaled()
        if lo is not None:
            spread = (y.amax((0, 2, 3)) - y.amin((0, 2, 3))).clamp_min(1e-6)
            w[scope + "/BatchNorm/gamma"] = (t(scope + "/BatchNorm/gamma") / spread).numpy().astype(np.float32)
            y = scaled()
            w[scope + "/BatchNorm/beta"] = (lo - (base + y).amin((0, 2, 3))).numpy().astype(np.float32)
        return y + t(scope + "/BatchNorm/beta")[None, :, None, None]

    def gate(pre):
        gated.append(float(pre.amin()))
        return F.relu(pre)

    adj = margin is not None
    name = "resnet_v1_%d" % depth
    x = torch.from_numpy(frames.astype(np.float32) - np.asarray(O.MEAN_PIXEL, np.float32)).double().permute(0, 3, 1, 2)
    net = gate(bn(T._conv_same(x, t(name + "/conv1/weights"), 2), name + "/conv1", margin))
    _, pt, pb = O.tf_same_pads(net.shape[2], 3, 2)
    _, pl, pr = O.tf_same_pads(net.shape[3], 3, 2)
    padded = F.pad(net, (pl, pr, pt, pb), value=float("-inf"))
    win = F.unfold(padded, 3, stride=2).reshape(net.shape[0], net.shape[1], 9, -1)
    top2 = win.topk(2, dim=2).values
    pool_gap = float((top2[:, :, 0] - top2[:, :, 1]).min())
    net = F.max_pool2d(padded, 3, 2)
    for u in units(depth):
        if u.has_shortcut_conv:
            sc = bn(T._conv(net, t(u.scope + "/shortcut/weights"), u.stride), u.scope + "/shortcut", 0.0 if adj else None)
        else:
            sc = net if u.stride == 1 else net[:, :, ::u.stride, ::u.stride]
        r = gate(bn(T._conv(net, t(u.scope + "/conv1/weights"), 1), u.scope + "/conv1", margin))
        r = gate(bn(T._conv_same(r, t(u.scope + "/conv2/weights"), u.stride, u.rate), u.scope + "/conv2", margin))
        net = gate(sc + bn(T._conv(r, t(u.scope + "/conv3/weights"), 1), u.scope + "/conv3", margin, base=sc))
    if adj:
        for head, spread, centre in (("part_pred", 1.5, -4.0), ("locref_pred", 1.0, 0.0)):
            kw, kb = "pose/%s/block4/weights" % head, "pose/%s/block4/biases" % head
            y = T._deconv(net, t(kw), torch.zeros(w[kb].shape, dtype=torch.float64))
            s = spread / y.std((0, 2, 3))
            w[kw] = (t(kw) * s[None, None, :, None]).numpy().astype(np.float32)
            w[kb] = (centre - y.mean((0, 2, 3)) * s).numpy().astype(np.float32)
    return min(gated), len(gated), pool_gap


def _open_gate_weights(wts, frames, depth=50, margin=MARGIN):
    """make_weights' weights with every BatchNorm shifted so that no ReLU of the network is near its kink on these frames (see
    _net_forward64); checked in a fresh float64 forward on the final float32 weights: no gated value within `margin` of zero (up to
    the float32 rounding of beta) and no exact tie in a pool window."""
    w = {k: np.array(v, copy=True) for k, v in wts.items()}
    _net_forward64(w, frames, depth, margin)
    lo, n, gap = _net_forward64(w, frames, depth)
    assert n == 1 + 3 * 16, n
    assert lo > (1 - 1e-4) * margin, lo
    assert gap > 0.0, gap
    return w


def _per_tensor(g, P):
    """{trainable name: relative L2 error} of a gradient dict against the oracle's, all 163 tensors present"""
    _, _, per = _grad_agreement(g, P)
    assert len(per) == N_TRAINABLE, len(per)
    return {k: v[1] for k, v in per.items()}


def _worst(rel, n=3):
    return sorted(rel.items(), key=lambda kv: -kv[1])[:n]


def _dithered(frames, seed):
    """make_frames clips its blobs at 255: flat patches there give exactly equal stem outputs, i.e. tied pool windows.  Noise added
    after the clip breaks the ties."""
    rng = np.random.default_rng(seed)
    return np.clip(frames.astype(np.int16) - rng.integers(0, 8, frames.shape), 0, 255).astype(np.uint8)


def _open_gate_case(shape, seed):
    H, W, nt = shape
    batch, S0, wts, frames, ws, ws_max = _train_case(seed, hw=(H, W), nt=nt, nj=3)
    frames = _dithered(frames, seed)
    return batch, S0, _open_gate_weights(wts, frames), frames, ws, ws_max


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_open_gate_step_gradients_per_tensor(lib_built, shape):
    """Trainer.forward_backward (DGP loss, gm2 = 1, gm3 = 3) on the parity tier, every trainable tensor within BOUND of float64."""
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    _threads()
    H, W, nt = shape
    batch, S0, wts, frames, ws, ws_max = _open_gate_case(shape, 31)
    hy = DGPHyper(gm2=1, gm3=3)
    P, L = _oracle_grads(wts, frames, batch, S0, ws, ws_max, hy, 300.0, 25.0, dtype=torch.float64)
    tr = Trainer(50, 3, H, W, max_frames=nt)
    tr.load_weights(wts)
    losses = tr.forward_backward(torch.from_numpy(frames).cuda(), batch, hy, S0, ws, ws_max, 300.0, 25.0)
    ref = float(L["total_loss"].detach())
    assert abs(losses["total_loss"] - ref) < 1e-5 * max(1.0, abs(ref)), (losses["total_loss"], ref)
    rel = _per_tensor(tr.get_grads(), P)
    print("open gates %dx%d parity: worst %s" % (H, W, _worst(rel)))
    assert max(rel.values()) < BOUND, _worst(rel)


def _edge_batch(nt, H, W, nj, seed):
    """Every frame visible, every label on the scoremap's last row or last column (alternating), no skeleton."""
    from deepgraphpose_amd import dataset as D
    rng = np.random.default_rng(seed)
    jl = np.empty((nt, nj, 2))
    for n in range(nt):
        for j in range(nj):
            jl[n, j] = (H - 1, rng.uniform(0, W - 1)) if (n + j) % 2 else (rng.uniform(0, H - 1), W - 1)
    vm, hm, vt = D.gen_idx_chunk(np.arange(nt), np.zeros(0, dtype=int), jl)
    assert len(vm) == nt * nj and len(hm) == 0
    lmap, lmask = D.coord2map(jl, H, W, nj, 8)
    batch = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt, nt=nt)
    return batch, np.zeros((0, nj)), np.zeros(0), np.zeros(0)


@pytest.mark.parametrize("shape", [STEP_SHAPES[0], STEP_SHAPES[1], STEP_SHAPES[4]])
def test_open_gate_step_with_the_loss_on_the_last_row_and_column(lib_built, shape):
    """The same weights with a loss whose gradient sits on the scoremap's last row and column (the logits are ~-4 elsewhere, so the
    visible cross-entropy's gradient is small off the labels, and the locref mask covers only the labels' neighbourhoods): a row or
    column lost at a boundary is not diluted in the whole tensor's norm here."""
    from deepgraphpose_amd.arch import scoremap_hw
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    _threads()
    H, W, nt = shape
    _, _, wts, frames, _, _ = _open_gate_case(shape, 31)
    batch, S0, ws, ws_max = _edge_batch(nt, *scoremap_hw(H, W), 3, seed=H)
    hy = DGPHyper(gm2=1, gm3=3)
    P, L = _oracle_grads(wts, frames, batch, S0, ws, ws_max, hy, 300.0, 25.0, dtype=torch.float64)
    tr = Trainer(50, 3, H, W, max_frames=nt)
    tr.load_weights(wts)
    losses = tr.forward_backward(torch.from_numpy(frames).cuda(), batch, hy, S0, ws, ws_max, 300.0, 25.0)
    ref = float(L["total_loss"].detach())
    assert abs(losses["total_loss"] - ref) < 1e-5 * max(1.0, abs(ref)), (losses["total_loss"], ref)
    rel = _per_tensor(tr.get_grads(), P)
    print("edge labels %dx%d parity: worst %s" % (H, W, _worst(rel)))
    assert max(rel.values()) < BOUND, _worst(rel)


@pytest.mark.parametrize("shape", [pytest.param((33, 65), id="33x65"), pytest.param((75, 101), id="75x101")])
def test_open_gate_dlc_step_gradients_per_tensor(lib_built, shape):
    """Trainer.forward_backward_dlc (sigmoid cross-entropy on the part disks + locref Huber), every tensor within BOUND of float64."""
    from deepgraphpose_amd import synthetic
    from deepgraphpose_amd.train import Trainer
    from oracle import dgp_train_oracle as T
    _threads()
    H, W = shape
    nj = 3
    frames = _dithered(synthetic.make_frames(1, H, W, nj, seed=H), H)
    wts = _open_gate_weights(synthetic.make_weights(50, nj, True, seed=17, head_std=0.05), frames)
    sc, lmap, lmask = _dlc_targets(np.random.default_rng(W), H, W, nj)
    tr = Trainer(50, nj, H, W, max_frames=1)
    tr.load_weights(wts)
    losses = tr.forward_backward_dlc(torch.from_numpy(frames).cuda(), sc, lmap, lmask, locref_loss_weight=0.05)
    P = T.make_params(wts, torch.float64)
    pred, loc = T.network(frames, P, 50, torch.float64)
    d = lambda a: torch.from_numpy(a).double()
    L = T.dlc_loss(pred, loc, d(sc), d(lmap), d(lmask), None, 0.05)
    L["total_loss"].backward()
    ref = float(L["total_loss"].detach())
    assert abs(losses["total_loss"] - ref) < 1e-5 * max(1.0, abs(ref)), (losses["total_loss"], ref)
    rel = _per_tensor(tr.get_grads(), P)
    print("open gates DLC %dx%d: worst %s" % (H, W, _worst(rel)))
    assert max(rel.values()) < BOUND, _worst(rel)


@pytest.mark.parametrize("shape", [STEP_SHAPES[0], STEP_SHAPES[1], STEP_SHAPES[4]])
def test_open_gate_step_on_the_16_bit_tier(lib_built, shape):
    """Trainer(tier="f16") on the open-gate weights.  Pass 1 of the shape runs the parity path: the parity tolerances, and every tensor
    within BOUND.  Pass 2 is the 16-bit pass: the bounds of test_train_gpu.test_trainer_tier_f16_gradients_against_the_fp64_oracle, and
    with no gate to flip every tensor within BOUND_F16."""
    import ctypes
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    _threads()
    H, W, nt = shape
    batch, S0, wts, frames, ws, ws_max = _open_gate_case(shape, 31)
    hy = DGPHyper(gm2=1, gm3=3)
    P, L = _oracle_grads(wts, frames, batch, S0, ws, ws_max, hy, 300.0, 25.0, dtype=torch.float64)
    ref = float(L["total_loss"].detach())
    tr = Trainer(50, 3, H, W, max_frames=nt, tier="f16")
    tr.load_weights(wts)
    ft = torch.from_numpy(frames).cuda()
    was, failed = ctypes.c_int32(), ctypes.c_int32()
    l0 = tr.forward_backward(ft, batch, hy, S0, ws, ws_max, 300.0, 25.0)
    tr.lib.dgp_trainer_fast_status(tr._t, was, failed)
    assert was.value == 0 and abs(l0["total_loss"] - ref) < 1e-4 * max(1, abs(ref))
    g0 = tr.get_grads()
    cos0, rel0, _ = _grad_agreement(g0, P)
    assert cos0 > 0.99999 and rel0 < 3e-3
    rel = _per_tensor(g0, P)
    assert max(rel.values()) < BOUND, _worst(rel)
    l1 = tr.forward_backward(ft, batch, hy, S0, ws, ws_max, 300.0, 25.0)
    tr.lib.dgp_trainer_fast_status(tr._t, was, failed)
    assert was.value == 1 and failed.value == 0 and tr.fast_redos == 0 and tr.fast_passes == 1
    g1 = tr.get_grads()
    cos1, rel1, per = _grad_agreement(g1, P)
    worst = sorted(per.items(), key=lambda kv: kv[1][0])[:3]
    rel16 = {k: v[1] for k, v in per.items()}
    print("open gates %dx%d f16: parity pass worst %s | 16-bit pass loss %.6f (fp64 %.6f) cosine %.6f rel L2 %.4f worst %s"
          % (H, W, _worst(rel, 1), l1["total_loss"], ref, cos1, rel1, _worst(rel16)))
    assert abs(l1["total_loss"] - ref) < 2e-3 * max(1, abs(ref))
    assert cos1 >= 0.999 and rel1 <= 0.05
    assert min(v[0] for v in per.values()) >= 0.98, worst
    assert max(rel16.values()) < BOUND_F16, _worst(rel16)
    assert all(np.isfinite(v).all() for v in g1.values())


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [STEP_SHAPES[0], STEP_SHAPES[1], STEP_SHAPES[4]])
def test_realistic_weights_step_on_odd_grids(lib_built, shape):
    """Ordinary make_weights (ReLU masks that really cut) on the parity tier against float64: block4 + heads to 2e-5, every other tensor
    to 1e-2 (test_train_gpu.test_full_backward_matches_autograd), the whole gradient to 1e-3.  At 747 x 832 block4's own gates can flip
    (47 x 52 pixels per frame; measured 1.5e-4 in block4/unit_2): there block4 + heads are held to test_full_size_config4_step_matches_autograd's
    5e-4 (measured global 5.8e-5)."""
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    _threads()
    H, W, nt = shape
    batch, S0, wts, frames, ws, ws_max = _train_case(37, hw=(H, W), nt=nt, nj=3)
    hy = DGPHyper(gm2=1, gm3=3)
    P, L = _oracle_grads(wts, frames, batch, S0, ws, ws_max, hy, 300.0, 25.0, dtype=torch.float64)
    tr = Trainer(50, 3, H, W, max_frames=nt)
    tr.load_weights(wts)
    losses = tr.forward_backward(torch.from_numpy(frames).cuda(), batch, hy, S0, ws, ws_max, 300.0, 25.0)
    ref = float(L["total_loss"].detach())
    assert abs(losses["total_loss"] - ref) < 1e-4 * max(1.0, abs(ref)), (losses["total_loss"], ref)
    g = tr.get_grads()
    _, glob, _ = _grad_agreement(g, P)
    rel = _per_tensor(g, P)
    strict = {k: v for k, v in rel.items() if "block4" in k or k.startswith("pose/")}
    print("make_weights %dx%d parity: strict worst %s | all worst %s | global %.3g" % (H, W, _worst(strict, 2), _worst(rel, 2), glob))
    assert len(strict) == 3 * 10 + 4 and max(strict.values()) < (5e-4 if H * W > 480 * 640 else 2e-5), _worst(strict)
    assert max(rel.values()) < 1e-2, _worst(rel)
    assert glob < 1e-3, glob


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [pytest.param((32, 32), id="32x32"), pytest.param((33, 65), id="33x65")])
def test_inference_on_the_smallest_frames(lib_built, hw):
    """dgp_net_create takes frames down to 32 x 32 (a 2 x 2 feature map).  Parity tier: coordinates within 1e-3 px of the oracle, window
    indices bit-exact; 16-bit tier: inside the band of test_h1_gpu.test_tier_f16_network_stays_within_its_measured_band."""
    from test_h1_gpu import _tier_errors
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    from oracle import dgp_oracle as O
    h, w = hw
    nj, B = 4, 3
    wts = make_weights(50, nj, False, seed=5, head_std=0.05)
    frames = make_frames(B, h, w, nj, seed=h + w)
    ref = O.infer(frames, wts, 50, 8.0, 1.0, 1)
    net = engine.DGPNet(50, nj, h, w, max_batch=B, with_locref=False)
    net16 = engine.DGPNet(50, nj, h, w, max_batch=B, with_locref=False, tier="f16")
    net.load_weights(wts)
    net16.load_weights(wts)
    e32 = _tier_errors(net, frames, ref)
    e16 = _tier_errors(net16, frames, ref)
    print("%dx%d: parity %s | f16 %s" % (h, w, e32, e16))
    assert e32["px_max"] < 1e-3 and e32["idx_agree"] == 1.0 and e32["sc_rel"] < 1e-4
    assert e16["px_max"] < 0.1 and e16["px_rmse"] < 0.05 and e16["sc_rel"] < 1e-2 and e16["idx_agree"] >= 0.9 and e16["conf_max"] < 1e-2
