"""GPU tests of the Adam optimiser: global-norm clip + TF-1's dense ApplyAdam (sumsq_kernel + adam_kernel behind dgp_adam_clip) on gradients
written straight into the trainer's flat buffers, against the float64 restatement and the hand-derived answers of tests/_adam_ref.py; the
skip protocol of the 16-bit tier, Trainer.step end to end, the optimiser's state by name and the fit driver.

Tolerances (tests/_adam_ref.py, tolerances): ulps x 2^-23 x magnitude + the smallest fp32 subnormal; 4 ulps for m and v against the float64
slots, 8 for the parameters against the float64 move computed from the slots the kernel stored (adam_step's `stored`).  The library is built without fast-math flags and hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt holds, so the
kernel's divide and sqrt are correctly rounded and nothing is widened for them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _adam_ref as A

pytestmark = pytest.mark.gpu

EPS32 = A.EPS32
B1, B2 = np.float32(0.9), np.float32(0.999)


def _put(view, a):
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(view.device))


def _get(view):
    torch.cuda.synchronize()
    return view.cpu().numpy()


def _set_powers(tr, b1p, b2p):
    a = np.array([b1p, b2p], dtype=np.float32)
    rc = tr.lib.dgp_trainer_upload(tr._t, 7, 0, a.ctypes.data_as(C.c_void_p), 2)       # (allocates Adam's slots when they do not exist yet)
    assert rc == 0


def _get_powers(tr):
    a = np.empty(2, dtype=np.float32)
    assert tr.lib.dgp_trainer_download(tr._t, 7, 0, a.ctypes.data_as(C.c_void_p), 2) == 0
    return a


def _views(tr):
    """(params, gradients, m, v) as device views of the trainer's flat buffers (Adam's slots must exist)"""
    from deepgraphpose_amd import train
    n = tr.n_trainable
    ptrs = [tr.lib.dgp_trainer_buffer(tr._t, w) for w in (0, 1, 5, 6)]
    assert all(ptrs)
    return tuple(train._view(p, (n,), tr.device) for p in ptrs)


@pytest.fixture(scope="module")
def opt(lib_built):
    """One trainer for the module (ResNet-50 with 3 joints: 23.7 M trainables); every test writes the parameters, slots, powers and
    gradients it starts from.  -> (trainer, params, gradients, m, v)"""
    from deepgraphpose_amd import train
    from deepgraphpose_amd.synthetic import make_weights
    tr = train.Trainer(50, 3, 64, 96, max_frames=3)
    tr.load_weights(make_weights(50, 3, True, seed=4, head_std=0.05))
    assert not tr.lib.dgp_trainer_buffer(tr._t, 5) and not tr.lib.dgp_trainer_buffer(tr._t, 7)      # nothing of Adam's before its first use
    assert tr.get_optimizer_state() == {}
    _set_powers(tr, B1, B2)
    yield (tr,) + _views(tr)
    del tr


def _reset(opt, p=None):
    tr, P, G, M, V = opt
    if p is not None:
        _put(P, p)
    M.zero_()
    V.zero_()
    _set_powers(tr, B1, B2)


def _check_state(ref, p0, m0, v0, p1, m1, v1):
    tol_m, tol_v, tol_p = A.tolerances(ref, p0, m0, v0)
    assert not (np.isnan(p1).any() or np.isnan(m1).any() or np.isnan(v1).any())
    for name, got, want, tol in (("m", m1, ref["m"], tol_m), ("v", v1, ref["v"], tol_v), ("params", p1, ref["var"], tol_p)):
        inf = np.isinf(want)
        if inf.any():
            assert np.array_equal(got[inf], want[inf].astype(np.float32)), name
        err = np.where(inf, 0.0, np.abs(got - np.where(inf, 0.0, want)))
        k = int(np.argmax(err - tol))
        assert err[k] <= tol[k], (name, k, got[k], want[k], err[k], tol[k])


def _step_and_check(opt, g, lr, clip, beta1=0.9, beta2=0.999, eps=1e-8):
    """Writes g, runs one Adam step, asserts m, v and the parameters against the reference from the state before, the powers to be the
    fp32 products power * beta exactly, and the reported norm to 1 ulp of float32(sqrt(fp64 sum of squares)).  -> (params, m, v, reference)"""
    tr, P, G, M, V = opt
    p0, m0, v0, pw0 = _get(P), _get(M), _get(V), _get_powers(tr)
    _put(G, g)
    gn_dev = tr.apply_gradients(lr, 0.9, clip, optimizer="adam", beta1=beta1, beta2=beta2, eps=eps)
    p1, m1, v1, pw1 = _get(P), _get(M), _get(V), _get_powers(tr)
    ref = A.adam_step(p0, m0, v0, g, pw0[0], pw0[1], lr, beta1, beta2, eps, clip, stored=(m1, v1))
    gn32 = np.float32(ref["gn"])
    assert abs(np.float32(gn_dev) - gn32) <= np.spacing(gn32), (gn_dev, ref["gn"])
    assert pw1[0] == pw0[0] * np.float32(beta1) and pw1[1] == pw0[1] * np.float32(beta2), (pw0, pw1)
    _check_state(ref, p0, m0, v0, p1, m1, v1)
    return p1, m1, v1, ref


def test_the_flat_buffer_is_a_whole_number_of_float4(opt):
    """adam_kernel reads float4s and then the last n % 4 elements one by one.  The trainer pads EVERY tensor to a multiple of 4 floats
    (dgp_trainer_create keeps each 16-byte aligned), so n_trainable % 4 is 0 for every joint count -- 1 to 6 joints are checked here on
    the table's own arithmetic -- and no trainer reaches the scalar tail; the ends of the float4 loop are tested below instead."""
    tr = opt[0]
    assert tr.n_trainable % 4 == 0
    assert all(off % 4 == 0 for off, _, st in tr.table.values() if not st)
    body = sum((size + 3) // 4 * 4 for k, (_, size, st) in tr.table.items() if not st and not k.startswith("pose/"))
    cin = tr.table["pose/part_pred/block4/weights"][1] // (9 * 3)
    for nj in range(1, 7):
        heads = sum((s + 3) // 4 * 4 for s in (9 * nj * cin, nj, 9 * 2 * nj * cin, 2 * nj))
        assert (body + heads) % 4 == 0


def test_known_answers_in_a_bn_gamma_and_a_head_bias(opt):
    """adam_test.py testBasic (tests/_adam_ref.py): var0 [1, 2] with gradient 0.1 in the stem's BN gamma, var1 [3, 4] with 0.01 in the part
    head's biases, lr 0.001, three steps from zero slots; every other gradient is zero.  Each step meets the reference; the end meets the
    closed form to the three steps' bounds (8 ulps each, + 1e-8 for the powers' own fp32 rounding); the powers are beta^4; parameters
    with zero gradient and zero slots are bit-unchanged (0 / (0 + eps) = 0)."""
    tr, P, G, M, V = opt
    o0 = tr.table["resnet_v1_50/conv1/BatchNorm/gamma"][0]
    o1 = tr.table["pose/part_pred/block4/biases"][0]
    assert not tr.table["resnet_v1_50/conv1/BatchNorm/gamma"][2] and not tr.table["pose/part_pred/block4/biases"][2]
    p = _get(P).copy()
    p[o0:o0 + 2], p[o1:o1 + 2] = A.BASIC_VAR0, A.BASIC_VAR1
    _reset(opt, p)
    g = np.zeros(tr.n_trainable, np.float32)
    g[o0:o0 + 2], g[o1:o1 + 2] = A.BASIC_G0, A.BASIC_G1
    for _ in range(A.BASIC_STEPS):
        p1, m1, v1, _ = _step_and_check(opt, g, A.BASIC_LR, 10.0)
    rest = np.ones(p1.size, bool)
    rest[o0:o0 + 2] = rest[o1:o1 + 2] = False
    assert np.array_equal(p1[rest], p[rest]) and not m1[rest].any() and not v1[rest].any()
    for o, var, gg, rough in ((o0, A.BASIC_VAR0, A.BASIC_G0, A.BASIC_ROUGH[0]), (o1, A.BASIC_VAR1, A.BASIC_G1, A.BASIC_ROUGH[1])):
        want, m, v, _, _ = A.basic_expected(var, gg)
        np.testing.assert_allclose(p1[o:o + 2], want, rtol=3 * 8 * EPS32, atol=1e-8)
        np.testing.assert_allclose(p1[o:o + 2], rough, atol=1e-6)
        np.testing.assert_allclose(m1[o:o + 2], m, rtol=3 * 4 * EPS32)
        np.testing.assert_allclose(v1[o:o + 2], v, rtol=3 * 4 * EPS32)
    pw = _get_powers(tr)
    assert pw[0] == B1 * B1 * B1 * B1 and pw[1] == B2 * B2 * B2 * B2
    np.testing.assert_allclose(pw, [0.9 ** 4, 0.999 ** 4], rtol=4 * EPS32)


def test_clip_then_adam_known_answers(opt):
    """The norm-5 vectors of tf.clip_by_global_norm's test at clip 4, in the stem's first six weights and the locref head's biases, from
    var 0: the reported norm is 5 exactly, m = 0.8 (1 - beta1) g, and the move is lr sign(g) / (1 + eps / (0.8 |g| s_1))."""
    import _tf_kat as K
    tr, P, G, M, V = opt
    o0 = tr.table["resnet_v1_50/conv1/weights"][0]
    o1 = tr.table["pose/locref_pred/block4/biases"][0]
    idx = np.concatenate([np.arange(o0, o0 + 6), np.arange(o1, o1 + 2)])
    p = _get(P).copy()
    p[idx] = 0.0
    _reset(opt, p)
    g = np.zeros(tr.n_trainable, np.float32)
    g[idx] = A.CLIP_G
    _put(G, g)
    p1, m1, v1, ref = _step_and_check(opt, g, A.BASIC_LR, A.CLIP_AT)
    assert ref["gn"] == K.CLIP_NORM
    move, m = A.clip_expected(A.CLIP_G)
    np.testing.assert_allclose(-p1[idx], move, rtol=8 * EPS32, atol=0)
    np.testing.assert_allclose(m1[idx], m, rtol=4 * EPS32, atol=0)
    nz = A.CLIP_G != 0
    np.testing.assert_allclose(-p1[idx][nz], A.f32(A.BASIC_LR) * np.sign(A.CLIP_G[nz]), rtol=1e-5)     # eps / (0.8 * 1 * 0.0316) = 4e-7
    rest = np.ones(p1.size, bool)
    rest[idx] = False
    assert np.array_equal(p1[rest], p[rest]) and not p1[idx][~nz].any()


def test_dense_gradient_three_steps_toggle_the_clip(opt):
    """Three consecutive steps on dense random gradients over every trainable, the clip active (norm ~49 against 10), off (0) and active
    again: m, v, parameters, powers and the reported norm after every step, each from the state the step before left."""
    tr, P, G, M, V = opt
    rng = np.random.default_rng(4)
    _reset(opt)
    for s, clip in ((0.01, 10.0), (0.001, 0.0), (0.02, 10.0)):          # a standard normal times s over 23.7 M elements has norm ~4 866 s
        g = rng.standard_normal(tr.n_trainable, dtype=np.float32) * np.float32(s)
        _, _, _, ref = _step_and_check(opt, g, 0.001, clip)
        assert clip == 0.0 or ref["gn"] > 2 * clip
    pw = _get_powers(tr)
    assert pw[0] == B1 * B1 * B1 * B1 and pw[1] == B2 * B2 * B2 * B2


def test_gradient_only_at_the_ends_of_the_buffer(opt):
    """A gradient only at element 0 (the first float4's first lane) and only at element n - 1 (the last float4's last lane, or the scalar
    tail should n % 4 ever be non-zero): both reach the norm (3, clip 2 scales by 2 / 3) and the update; nothing else moves."""
    tr, P, G, M, V = opt
    n = tr.n_trainable
    for where in (0, n - 1):
        _reset(opt)
        p0 = _get(P).copy()
        g = np.zeros(n, np.float32)
        g[where] = 3.0
        p1, m1, v1, ref = _step_and_check(opt, g, 0.5, 2.0)
        assert ref["gn"] == 3.0
        np.testing.assert_allclose(m1[where], 2.0 * (1.0 - float(B1)), rtol=4 * EPS32)
        assert abs((p0[where] - p1[where]) - 0.5) < 1e-5 * 0.5 + 8 * EPS32 * max(abs(p0[where]), 0.5)      # eps / (2 s_1) = 1.6e-7
        rest = np.ones(n, bool)
        rest[where] = False
        assert np.array_equal(p1[rest], p0[rest]) and not m1[rest].any() and not v1[rest].any()


def test_underflowing_square_moves_by_alpha_m_over_eps(opt):
    """g = 1e-25: g g = 1e-50 is below the smallest fp32 subnormal, so v stays exactly 0 and the move is alpha m / eps."""
    tr, P, G, M, V = opt
    rng = np.random.default_rng(5)
    idx = rng.choice(tr.n_trainable, 1000, replace=False)
    p = _get(P).copy()
    p[idx] = 0.0
    _reset(opt, p)
    g = np.zeros(tr.n_trainable, np.float32)
    g[idx] = 1e-25
    p1, m1, v1, _ = _step_and_check(opt, g, 0.001, 0.0)
    assert not v1.any()
    alpha = A.f32(0.001) * np.sqrt(1.0 - float(B2)) / (1.0 - float(B1))
    want = alpha * ((1.0 - float(B1)) * float(np.float32(1e-25))) / A.f32(1e-8)
    np.testing.assert_allclose(-p1[idx], want, rtol=8 * EPS32)
    assert want > 1e-23                                               # (a move fp32 resolves: 3.2e-22)


def test_overflowing_square_stops_the_parameter_and_stays_infinite(opt):
    """g = 1e20: g g is beyond fp32, v becomes +inf, the parameter does not move (m alpha / inf = 0) and nothing is NaN; on the next step
    with g = 0, v stays +inf and the parameter still does not move."""
    tr, P, G, M, V = opt
    rng = np.random.default_rng(6)
    idx = rng.choice(tr.n_trainable, 1000, replace=False)
    _reset(opt)
    p0 = _get(P).copy()
    g = np.zeros(tr.n_trainable, np.float32)
    g[idx] = 1e20
    p1, m1, v1, _ = _step_and_check(opt, g, 0.001, 0.0)
    assert np.all(v1[idx] == np.inf) and np.isfinite(m1).all() and np.array_equal(p1, p0)
    p2, m2, v2, _ = _step_and_check(opt, np.zeros(tr.n_trainable, np.float32), 0.001, 0.0)
    assert np.all(v2[idx] == np.inf) and np.isfinite(m2).all() and np.array_equal(p2, p0)
    assert np.count_nonzero(v2) == idx.size


def test_large_eps_makes_the_move_alpha_m(opt):
    """eps = 1: the move is alpha m / (sqrt(v) + 1) = alpha m (1 - O(sqrt v)), sqrt(v) <= |g| sqrt(1 - beta2) here.  From var 0, lr 1."""
    tr, P, G, M, V = opt
    rng = np.random.default_rng(7)
    _reset(opt, np.zeros(tr.n_trainable, np.float32))
    g = rng.standard_normal(tr.n_trainable, dtype=np.float32) * np.float32(0.01)
    p1, m1, v1, ref = _step_and_check(opt, g, 1.0, 0.0, eps=1.0)
    alpha = np.sqrt(1.0 - float(B2)) / (1.0 - float(B1))
    am = alpha * ref["m"]
    assert np.all(np.abs(-p1 - am) <= np.abs(am) * np.sqrt(ref["v"]) + 8 * EPS32 * np.abs(am) + A.TINY32)


def test_beta1_zero_makes_m_the_clipped_gradient(opt):
    """beta1 = 0: m += (g' - m) * 1, so m = g' whatever it was before (to the bound of m: 4 ulps of max(|m_0|, |g'|))."""
    tr, P, G, M, V = opt
    rng = np.random.default_rng(8)
    _reset(opt)
    m0 = (rng.standard_normal(tr.n_trainable) * 0.01).astype(np.float32)
    _put(M, m0)
    _set_powers(tr, 0.0, B2)                                          # beta1_power starts at beta1
    g = rng.standard_normal(tr.n_trainable, dtype=np.float32) * np.float32(0.01)
    _, m1, _, ref = _step_and_check(opt, g, 0.001, 10.0, beta1=0.0)
    assert ref["gn"] > 20.0
    assert np.all(np.abs(m1 - ref["gs"]) <= 4 * EPS32 * np.maximum(np.abs(m0), np.abs(ref["gs"])) + A.TINY32)


def test_a_momentum_step_and_an_adam_step_keep_to_their_own_slots(opt):
    """One trainer, a momentum step and then an Adam step: the Adam step leaves the momentum slot bit-unchanged, the momentum step left
    Adam's slots and powers alone, and both shared the two norm accumulators in turn."""
    from deepgraphpose_amd import train
    tr, P, G, M, V = opt
    rng = np.random.default_rng(9)
    _reset(opt)
    mom = train._view(tr.lib.dgp_trainer_buffer(tr._t, 2), (tr.n_trainable,), tr.device)
    g = rng.standard_normal(tr.n_trainable, dtype=np.float32) * np.float32(0.01)
    _put(G, g)
    gn = tr.apply_gradients(0.005, 0.9, 10.0)
    slot = _get(mom).copy()
    assert slot.any() and not _get(M).any() and not _get(V).any() and np.array_equal(_get_powers(tr), [B1, B2])
    _, _, _, ref = _step_and_check(opt, g, 0.001, 10.0)
    assert abs(np.float32(gn) - np.float32(ref["gn"])) <= np.spacing(np.float32(ref["gn"]))
    assert np.array_equal(_get(mom), slot)


# ---- Trainer.step ---------------------------------------------------------------------------------------------------------------------
def _step_case(seed, nvf=1):
    import test_train_gpu as TT
    return TT._train_case(seed, nvf=nvf)


def _flat_state(tr):
    """(params, m, v, powers) on the host; zero slots and powers at the betas before Adam's state exists"""
    from deepgraphpose_amd import train
    n = tr.n_trainable
    p = _get(train._view(tr.lib.dgp_trainer_buffer(tr._t, 0), (n,), tr.device))
    if not tr.lib.dgp_trainer_buffer(tr._t, 5):
        return p, np.zeros(n, np.float32), np.zeros(n, np.float32), np.array([B1, B2])
    _, _, M, V = _views(tr)
    return p, _get(M), _get(V), _get_powers(tr)


def _check_applied_step(tr, before, hy, gn_reported):
    """The state after a Trainer.step against the helper applied to the gradients the step left in the buffer, from the state before"""
    p0, m0, v0, pw0 = before
    g = _get(tr.grads_tensor())
    p1, m1, v1, pw1 = _flat_state(tr)
    ref = A.adam_step(p0, m0, v0, g, pw0[0], pw0[1], hy.lr, hy.beta1, hy.beta2, hy.adam_eps, hy.clip_norm, stored=(m1, v1))
    assert pw1[0] == np.float32(pw0[0]) * np.float32(hy.beta1) and pw1[1] == np.float32(pw0[1]) * np.float32(hy.beta2), (pw0, pw1)
    gn32 = np.float32(ref["gn"])
    assert abs(np.float32(gn_reported) - gn32) <= np.spacing(gn32)
    _check_state(ref, p0, m0, v0, p1, m1, v1)
    return p1, m1, v1, pw1


def test_step_with_adam_matches_the_oracle_loss_and_the_helper(lib_built):
    """Two Trainer.step calls with hyper.optimizer = "adam" on the parity tier.  The losses and the gradient norm are compared to
    oracle.dgp_train_oracle evaluated at the trainer's own parameters before each step; the parameters, m, v and the powers to the helper
    applied to the trainer's OWN gradient buffer from the state before.  The parameters are deliberately not compared to an Adam run on
    the oracle's gradients: Adam's first step is lr sign(g), so a parameter whose gradient is rounding noise may legitimately move by
    2 lr in the opposite direction -- that comparison is ill-conditioned by construction."""
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    from oracle import dgp_train_oracle as T
    batch, S0, wts, frames, ws, ws_max = _step_case(5, nvf=2)
    hy = DGPHyper(gm2=0, gm3=0, lr=0.001, optimizer="adam")
    n_tot, n_vis = 300.0, 25.0
    tr = Trainer(50, 3, 64, 96, max_frames=3)
    tr.load_weights(wts)
    ft = torch.from_numpy(frames).cuda()
    cfg = dict(nj=3, S0=S0, ws=ws, ws_max=ws_max, stride=8.0, gamma=1.0, gauss_len=1, lengthscale=1.0, gm2=0, gm3=0,
               wn_visible=5.0, wn_hidden=3.0, locref_loss_weight=0.05, locref_huber_loss=True, n_frames_total=n_tot,
               n_visible_frames_total=n_vis)
    for it in range(2):
        P = T.make_params(tr.get_weights(), torch.float32)
        before = _flat_state(tr)
        losses = tr.step(ft, batch, hy, S0, ws, ws_max, n_tot, n_vis)
        pred, loc = T.network(frames, P, 50, torch.float32)
        L = T.dgp_loss(pred, loc, batch, cfg)
        L["total_loss"].backward()
        gn = float(np.sqrt(sum(float((t.grad.double() ** 2).sum()) for t in P.values() if t.requires_grad and t.grad is not None)))
        ref_loss = float(L["total_loss"].detach())
        assert abs(losses["total_loss"] - ref_loss) < 2e-4 * max(1.0, abs(ref_loss))
        assert abs(losses["grad_norm"] - gn) < 2e-3 * gn
        _, _, _, pw = _check_applied_step(tr, before, hy, losses["grad_norm"])
    assert pw[0] == B1 * B1 * B1 and pw[1] == B2 * B2 * B2
    assert sorted(k for k in tr.get_optimizer_state() if "/" not in k) == ["beta1_power", "beta2_power"]


def test_a_skipped_16_bit_step_leaves_adam_state_and_powers_alone(lib_built):
    """The 16-bit tier, three Trainer.step calls with Adam.  Before the third, a 64-fold stem scale is smuggled in behind the wrapper's back:
    the 16-bit pass fails its range check, its update is skipped ON THE DEVICE (parameters, m, v and the powers untouched, no read-back)
    and the step is repeated on the parity path.  Afterwards the powers are beta^4 -- advanced exactly three times -- and m, v and the
    parameters are the helper's result of ONE step from the state before, on the gradients the repeated pass left in the buffer."""
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    batch, S0, wts, frames, ws, ws_max = _step_case(3)
    hy = DGPHyper(gm2=1, gm3=3, lr=1e-5, optimizer="adam")
    tr = Trainer(50, 3, 64, 96, max_frames=3, tier="f16")
    tr.load_weights(wts)
    ft = torch.from_numpy(frames).cuda()
    _set_powers(tr, B1, B2)
    for it in range(3):
        if it == 2:
            w2 = tr.get_weights()
            w2["resnet_v1_50/conv1/BatchNorm/gamma"] = w2["resnet_v1_50/conv1/BatchNorm/gamma"] * 64.0
            w2["resnet_v1_50/conv1/BatchNorm/beta"] = w2["resnet_v1_50/conv1/BatchNorm/beta"] * 64.0
            key = tr._fast_key
            tr.load_weights(w2)
            tr._fast_key = key                                       # pretend nothing happened: the next pass is requested as a 16-bit one
        before = _flat_state(tr)
        losses = tr.step(ft, batch, hy, S0, ws, ws_max, 300.0, 25.0)
        assert np.isfinite(losses["total_loss"])
        assert tr.fast_redos == (1 if it == 2 else 0) and tr.fast_passes == it, (it, tr.fast_passes, tr.fast_redos)
        _, _, _, pw = _check_applied_step(tr, before, hy, losses["grad_norm"])
    assert tr.fast_redos == 1
    assert pw[0] == B1 * B1 * B1 * B1 and pw[1] == B2 * B2 * B2 * B2
    np.testing.assert_allclose(pw, [0.9 ** 4, 0.999 ** 4], rtol=4 * EPS32)


# ---- state by name --------------------------------------------------------------------------------------------------------------------
def test_optimizer_state_round_trips_by_name_and_resumes_bit_identically(lib_built, tmp_path):
    """get_optimizer_state -> Saver.save -> weights_io.load_optimizer_state -> load_optimizer_state of a fresh trainer: one further
    identical step (injected gradient) is bit-identical in parameters, m, v and powers to the uninterrupted trainer's."""
    from deepgraphpose_amd import _lib, train, weights_io
    from deepgraphpose_amd.synthetic import make_weights
    wts = make_weights(50, 3, True, seed=4, head_std=0.05)
    rng = np.random.default_rng(11)

    def fresh():
        t = train.Trainer(50, 3, 64, 96, max_frames=3)
        t.load_weights(wts)
        return t
    a = fresh()
    n = a.n_trainable
    assert a.get_optimizer_state() == {}
    g = [rng.standard_normal(n, dtype=np.float32) * np.float32(0.01) for _ in range(3)]
    _put(a.grads_tensor(), g[0])
    a.apply_gradients(0.005, 0.9, 10.0)                               # a momentum step: its slots are reported too
    for k in (0, 1):
        _put(a.grads_tensor(), g[k])
        a.apply_gradients(0.001, 0.9, 10.0, optimizer="adam")
    state = a.get_optimizer_state()
    w = a.get_weights()
    trainables = [k for k, (_, _, st) in a.table.items() if not st]
    assert sorted(state) == sorted([k + s for k in trainables for s in ("/Momentum", "/Adam", "/Adam_1")] + ["beta1_power", "beta2_power"])
    assert all(state[k + s].shape == w[k].shape for k in trainables for s in ("/Momentum", "/Adam", "/Adam_1"))
    assert state["beta1_power"].shape == () and state["beta1_power"] == B1 * B1 * B1 and state["beta2_power"] == B2 * B2 * B2
    prefix = weights_io.Saver(fmt="tf").save({**w, **state}, str(tmp_path / "snapshot-step1-"), global_step=2)
    assert sorted(weights_io.load_weights(prefix)) == sorted(w)       # the default reader still returns the model variables alone
    loaded = weights_io.load_optimizer_state(prefix)
    assert sorted(loaded) == sorted(state)
    b = train.Trainer(50, 3, 64, 96, max_frames=3)
    b.load_weights(weights_io.load_weights(prefix))
    bad = dict(loaded)
    del bad["pose/part_pred/block4/biases/Adam_1"]
    with pytest.raises(_lib.DgpError, match="pose/part_pred/block4/biases/Adam_1"):
        b.load_optimizer_state(bad)
    bad = dict(loaded, **{"resnet_v1_50/conv1/weights/Adam": np.zeros(5, np.float32)})
    with pytest.raises(_lib.DgpError, match="resnet_v1_50/conv1/weights/Adam"):
        b.load_optimizer_state(bad)
    assert b.get_optimizer_state() == {}                              # (nothing was uploaded by the refused calls)
    b.load_optimizer_state(loaded)
    for t in (a, b):
        _put(t.grads_tensor(), g[2])
        t.apply_gradients(0.001, 0.9, 10.0, optimizer="adam")
    named = np.zeros(n, bool)               # (the floats that pad a tensor to a multiple of 4 belong to no variable: the injected gradient
    for k in trainables:                    #  reaches them in the flat buffer, no name carries them over)
        named[a.table[k][0]:a.table[k][0] + a.table[k][1]] = True
    assert n - 16 < np.count_nonzero(named) < n
    sa, sb = _flat_state(a), _flat_state(b)
    for x, y in zip(sa[:3], sb[:3]):
        assert np.array_equal(x[named], y[named])
    assert np.array_equal(sa[3], sb[3]) and sa[3][0] == B1 * B1 * B1 * B1
    mom = [_get(train._view(t.lib.dgp_trainer_buffer(t._t, 2), (n,), t.device)) for t in (a, b)]
    assert np.array_equal(mom[0][named], mom[1][named]) and mom[0].any()


# ---- driver ---------------------------------------------------------------------------------------------------------------------------
def _reaching_fit_dlc_project(root, monkeypatch):
    """The Reaching demo project from the files under tests/golden (tests/test_reaching_cpu.py), its configs rewritten by the demo script,
    with a seeded 5-joint snapshot `snapshot-start` in its train folder for fit_dlc to start from."""
    import sys
    import test_reaching_cpu as R
    sys.path.insert(0, os.path.join(os.path.dirname(R.HERE), "demo"))
    import run_dgp_demo as demo
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.models.fitdgp_util import get_snapshot_path
    from deepgraphpose_amd.synthetic import make_weights
    dst = os.path.join(str(root), demo.DEMO_PROJECT)
    R._reaching_project(dst)
    monkeypatch.chdir(str(root))
    proj = demo.update_config_files(demo.DEMO_PROJECT, need_init_weights=False)
    snap0, _ = get_snapshot_path("snapshot-step0-final--0", proj, shuffle=1)
    weights_io.save_weights(os.path.join(os.path.dirname(snap0), "snapshot-start"), make_weights(50, 5, True, seed=2, head_std=0.05), fmt="tf")
    return proj, snap0


def test_fit_dlc_with_adam_keeps_its_state_in_the_snapshots_on_request(lib_built, tmp_path, capsys, monkeypatch):
    """fit_dlc(optimizer="adam", maxiters=3, keep_optimizer_state=True) on the Reaching project writes a final snapshot whose bundle holds
    the `/Adam`, `/Adam_1` slots of every trainable and the two powers (beta^5: iterations 0 .. 3 are four steps); the same call with the
    default arguments writes the model variables alone; a run that starts from the snapshot with state says that it restored it."""
    import random
    from deepgraphpose_amd import tf_checkpoint
    from deepgraphpose_amd.models import fitdgp
    proj, snap0 = _reaching_fit_dlc_project(tmp_path, monkeypatch)
    train_dir = os.path.dirname(snap0)

    def run(**kw):
        np.random.seed(0)
        random.seed(0)
        fitdgp.fit_dlc(kw.pop("start", "snapshot-start"), proj, maxiters=3, displayiters=1, saveiters=1000, **kw)
        t = tf_checkpoint.load_checkpoint(snap0, slots=True)
        return t

    t = run()
    model = sorted(t)
    assert not any(tf_checkpoint.is_optimizer_entry(k) for k in t)
    for f in os.listdir(train_dir):
        if f.startswith("snapshot-step0"):
            os.remove(os.path.join(train_dir, f))
    capsys.readouterr()
    t = run(optimizer="adam", keep_optimizer_state=True)
    assert "Restored" not in capsys.readouterr().out                  # (snapshot-start holds no state)
    trainables = [k for k in model if "moving_" not in k]
    assert sorted(t) == sorted(model + [k + s for k in trainables for s in ("/Adam", "/Adam_1")] + ["beta1_power", "beta2_power"])
    assert all(t[k + "/Adam"].shape == t[k].shape and np.isfinite(t[k + "/Adam_1"]).all() for k in trainables)
    assert t["beta1_power"].shape == () and t["beta1_power"] == B1 * B1 * B1 * B1 * B1 and t["beta2_power"] == B2 * B2 * B2 * B2 * B2
    assert t["pose/part_pred/block4/weights/Adam_1"].any()
    for ext in (".index", ".data-00000-of-00001"):
        os.rename(snap0 + ext, os.path.join(train_dir, "snapshot-resume") + ext)
    for f in os.listdir(train_dir):
        if f.startswith("snapshot-step0"):
            os.remove(os.path.join(train_dir, f))
    t2 = run(start="snapshot-resume", optimizer="adam", keep_optimizer_state=True)
    assert capsys.readouterr().out.count("Restored the adam optimizer state") == 1
    assert t2["beta1_power"] == np.float32(t["beta1_power"]) * B1 * B1 * B1 * B1            # four more steps on the restored powers
