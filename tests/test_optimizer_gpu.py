"""GPU tests of the optimiser on its own: global-norm clip + momentum SGD (sumsq_kernel + momentum_kernel behind dgp_sgd_momentum_clip)
on gradients written straight into the trainer's flat buffer, against an fp64 numpy restatement of tf.clip_by_global_norm and
tf.train.MomentumOptimizer: scale = clip / max(gn, clip) (clip <= 0: 1), accum = m accum + g scale, var -= lr accum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23          # one fp32 ulp, relative to the value's magnitude (an upper bound)


@pytest.fixture(scope="module")
def opt(lib_built):
    """One trainer for the module (the flat buffers of ResNet-50 with 3 joints: 23.7 M trainables); every test writes the parameters,
    momentum and gradients it starts from.  -> (trainer, params, gradients, momentum) as device views of the trainer's buffers."""
    from deepgraphpose_amd import _lib, train
    from deepgraphpose_amd.synthetic import make_weights
    tr = train.Trainer(50, 3, 64, 96, max_frames=3)
    tr.load_weights(make_weights(50, 3, True, seed=4, head_std=0.05))
    lib = _lib.load()
    n = tr.n_trainable
    p = train._view(lib.dgp_trainer_buffer(tr._t, 0), (n,), tr.device)
    v = train._view(lib.dgp_trainer_buffer(tr._t, 2), (n,), tr.device)
    yield tr, p, tr.grads_tensor(), v
    del tr


def _put(view, a):
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(view.device))


def _get(view):
    torch.cuda.synchronize()
    return view.cpu().numpy()


def _reference(p0, v0, g, lr, m, clip):
    """fp64 restatement of one step from the fp32 state the kernel starts from; lr / m / clip as the fp32 values the kernel receives"""
    lr, m, clip = (float(np.float32(x)) for x in (lr, m, clip))
    p0, v0, g = (np.asarray(x, np.float64) for x in (p0, v0, g))
    gn = float(np.sqrt(np.dot(g, g)))
    scale = clip / max(gn, clip) if clip > 0 else 1.0
    gs = g * scale
    a = m * v0 + gs
    return p0 - lr * a, a, gn, np.maximum(np.maximum(np.abs(a), m * np.abs(v0)), np.abs(gs))


def _step_and_check(opt, g, lr, m, clip, ulps=4):
    """Writes g, runs one step, asserts parameters and momentum against the reference to `ulps` fp32 ulps of their magnitude (the
    momentum's: max(|accum|, m |accum_0|, |g scale|); the parameters': max(|var|, lr of that)) and the reported norm to 1 ulp of
    float32(sqrt(fp64 sum of squares)).  -> (params, momentum, reported norm, reference norm)"""
    tr, P, G, V = opt
    p0, v0 = _get(P), _get(V)
    _put(G, g)
    gn_dev = tr.apply_gradients(lr, m, clip)
    p1, v1 = _get(P), _get(V)
    p_ref, a_ref, gn_ref, mag_a = _reference(p0, v0, g, lr, m, clip)
    gn32 = np.float32(gn_ref)
    assert abs(np.float32(gn_dev) - gn32) <= np.spacing(gn32), (gn_dev, gn_ref)
    err_a = np.abs(v1 - a_ref)
    tol_a = ulps * EPS32 * mag_a
    k = int(np.argmax(err_a - tol_a))
    assert err_a[k] <= tol_a[k], ("momentum", k, v1[k], a_ref[k])
    err_p = np.abs(p1 - p_ref)
    tol_p = ulps * EPS32 * np.maximum(np.abs(p_ref), float(np.float32(lr)) * mag_a)
    k = int(np.argmax(err_p - tol_p))
    assert err_p[k] <= tol_p[k], ("params", k, p1[k], p_ref[k])
    return p1, v1, gn_dev, gn_ref


def _zero_state(opt, p=None):
    tr, P, G, V = opt
    if p is not None:
        _put(P, p)
    V.zero_()


def test_momentum_known_answer_in_a_trainable_tensor(opt):
    """tf.train.MomentumOptimizer testBasic (tests/_tf_kat.py): var0 [1, 2] with gradient 0.1 and var1 [3, 4] with 0.01, lr 2, momentum
    0.9, placed in the part head's biases and the first two weights of the stem; the rest of the gradient is zero (norm 0.14, far below
    the clip).  Two steps: [0.8, 1.8] / [2.98, 3.98], then [0.42, 1.42] / [2.942, 3.942]; nothing else moves."""
    import _tf_kat as K
    tr, P, G, V = opt
    o0 = tr.table["pose/part_pred/block4/biases"][0]
    o1 = tr.table["resnet_v1_50/conv1/weights"][0]
    assert not tr.table["pose/part_pred/block4/biases"][2] and not tr.table["resnet_v1_50/conv1/weights"][2]
    p = _get(P).copy()
    p[o0:o0 + 2], p[o1:o1 + 2] = K.MOMENTUM_VAR0, K.MOMENTUM_VAR1
    _zero_state(opt, p)
    g = np.zeros(tr.n_trainable, np.float32)
    g[o0:o0 + 2], g[o1:o1 + 2] = K.MOMENTUM_G0, K.MOMENTUM_G1
    for want0, want1 in K.MOMENTUM_STEPS:
        p1, _, _, _ = _step_and_check(opt, g, K.MOMENTUM_LR, K.MOMENTUM_M, 10.0)
        np.testing.assert_allclose(p1[o0:o0 + 2], want0, rtol=4 * EPS32)
        np.testing.assert_allclose(p1[o1:o1 + 2], want1, rtol=4 * EPS32)
        rest = np.ones(p1.size, bool)
        rest[o0:o0 + 2] = rest[o1:o1 + 2] = False
        np.testing.assert_array_equal(p1[rest], p[rest])


@pytest.mark.parametrize("clip,scale", [(4.0, 0.8), (6.0, 1.0)])
def test_clip_by_global_norm_known_answers(opt, clip, scale):
    """tf.clip_by_global_norm testClipByGlobalNorm / ...NotClipped: t0 [[-2, 0, 0], [4, 0, 0]] and t1 [1, -2] (norm 5) as the stem's
    first six weights and the locref head's biases.  lr 1, momentum 0 from var 0: -var is the clipped gradient -- x 0.8 at clip 4,
    unchanged at clip 6; the reported norm is 5 exactly."""
    import _tf_kat as K
    tr, P, G, V = opt
    o0 = tr.table["resnet_v1_50/conv1/weights"][0]
    o1 = tr.table["pose/locref_pred/block4/biases"][0]
    _zero_state(opt, np.zeros(tr.n_trainable, np.float32))
    g = np.zeros(tr.n_trainable, np.float32)
    g[o0:o0 + 6], g[o1:o1 + 2] = K.CLIP_T0.ravel(), K.CLIP_T1
    p1, _, gn, _ = _step_and_check(opt, g, 1.0, 0.0, clip)
    assert gn == K.CLIP_NORM
    want = K.CLIP_AT_4 if clip == 4.0 else K.CLIP_AT_6
    np.testing.assert_allclose(-p1[o0:o0 + 6], want[0].ravel(), rtol=2 * EPS32)
    np.testing.assert_allclose(-p1[o1:o1 + 2], want[1], rtol=2 * EPS32)
    assert np.count_nonzero(p1) == np.count_nonzero(g)
    np.testing.assert_allclose(-p1[g != 0], g[g != 0] * scale, rtol=2 * EPS32)


def test_clip_at_exactly_the_norm_is_bit_identical_to_no_clip(opt):
    """gn == clip: gradient entries 3 and 4 (norm 5 exactly) with clip 5 scale by 5 / max(5, 5) = 1, so the step must equal, bit for
    bit, the same step with clip 0 (no clipping) from the same parameters and momentum."""
    tr, P, G, V = opt
    rng = np.random.default_rng(1)
    p0 = _get(P).copy()
    v0 = (rng.standard_normal(tr.n_trainable) * 0.01).astype(np.float32)
    g = np.zeros(tr.n_trainable, np.float32)
    g[[17, tr.n_trainable // 2]] = 3.0, 4.0
    res = []
    for clip in (5.0, 0.0):
        _put(P, p0)
        _put(V, v0)
        p1, v1, gn, _ = _step_and_check(opt, g, 0.005, 0.9, clip)
        assert gn == 5.0
        res.append((p1, v1))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_no_clip_when_clip_is_not_positive(opt):
    """clip <= 0 (fit_dlc's plain MomentumOptimizer): a gradient of norm 1e6 is applied unscaled, and the norm is still reported."""
    tr, P, G, V = opt
    rng = np.random.default_rng(2)
    _zero_state(opt)
    g = np.zeros(tr.n_trainable, np.float32)
    idx = rng.choice(tr.n_trainable, 1000, replace=False)
    g[idx] = rng.standard_normal(1000)
    g *= np.float32(1e6 / np.linalg.norm(g.astype(np.float64)))
    for clip in (0.0, -1.0):
        _zero_state(opt)
        _, v1, gn, gn_ref = _step_and_check(opt, g, 1e-9, 0.9, clip)
        assert gn_ref > 0.999e6
        np.testing.assert_array_equal(v1, g)              # momentum 0 before: accum = g * 1 exactly


def test_gradient_only_at_the_ends_of_the_buffer(opt):
    """sumsq_kernel reads float4s, then the last n % 4 elements one by one; the trainer pads every tensor to a multiple of 4 floats, so
    n % 4 is 0 today and the whole buffer goes through the float4 loop.  A gradient only at the end (the last float4's last lane,
    or the scalar tail should n % 4 ever be non-zero), and one only at element 0 (the first float4's first lane), must both reach
    the norm -- 3 here, clip 2 scales by 2 / 3; a lost element would leave the norm 0 and the step unclipped."""
    tr, P, G, V = opt
    n = tr.n_trainable
    last = np.arange(n - n % 4, n) if n % 4 else np.array([n - 1])
    for where in (last, np.array([0])):
        _zero_state(opt)
        g = np.zeros(n, np.float32)
        g[where] = np.float32(3.0 / np.sqrt(where.size))
        p0 = _get(P).copy()
        p1, v1, gn, gn_ref = _step_and_check(opt, g, 0.5, 0.9, 2.0)
        assert abs(gn_ref - 3.0) < 1e-6
        np.testing.assert_allclose(v1[where], g[where] * (2.0 / 3.0), rtol=4 * EPS32)
        rest = np.ones(n, bool)
        rest[where] = False
        np.testing.assert_array_equal(p1[rest], p0[rest])


def test_reported_norm_of_a_dense_gradient(opt):
    """A dense random gradient over every trainable: the reported norm is float32(sqrt(fp64 sum of squares)) to 1 ulp, and the
    clipped step (norm ~250 against clip 10) matches the reference everywhere."""
    tr, P, G, V = opt
    rng = np.random.default_rng(3)
    _zero_state(opt)
    g = (rng.standard_normal(tr.n_trainable, dtype=np.float32) * 0.05)
    _, _, gn, gn_ref = _step_and_check(opt, g, 0.005, 0.9, 10.0)
    assert gn_ref > 100.0


def test_consecutive_steps_toggle_the_clip(opt):
    """Seven steps in a row with changing dense gradients, the clip active, inactive, off (0) and active again: parameters, momentum and
    norm after every step.  The sum of squares alternates between two fp64 accumulators, each zeroed by the step before the one that
    uses it: the third step is the first to reuse one, so a stale accumulator shows from there on."""
    tr, P, G, V = opt
    rng = np.random.default_rng(4)
    _zero_state(opt)
    # (gradient scale, clip): a standard normal times s over 23.7 M elements has norm ~4 866 s
    plan = [(0.01, 10.0), (0.001, 10.0), (0.02, 10.0), (0.0005, 10.0), (0.01, 0.0), (0.003, 10.0), (0.004, 5.0)]
    for it, (s, clip) in enumerate(plan):
        g = rng.standard_normal(tr.n_trainable, dtype=np.float32) * np.float32(s)
        _, _, gn, gn_ref = _step_and_check(opt, g, 0.005, 0.9, clip)
        if clip > 0:
            assert abs(gn_ref - clip) > 0.1 * clip, (it, gn_ref, clip)      # each step clearly on one side of its clip
