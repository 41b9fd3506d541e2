"""tf.clip_by_global_norm + TF-1's dense ApplyAdam restated in float64 numpy, and the known answers the Adam tests hold the helper
(tests/test_adam_cpu.py) and the kernel (tests/test_adam_gpu.py) to.  The definition, per step:

    scale = clip / max(gn, clip) if clip > 0 else 1                 g' = g scale
    alpha = lr sqrt(1 - beta2_power) / (1 - beta1_power)
    m += (g' - m)(1 - beta1)          v += (g' g' - v)(1 - beta2)
    var -= alpha m / (sqrt(v) + eps)
    then beta1_power *= beta1, beta2_power *= beta2                (they start at beta1, beta2: after t applied steps beta^(t + 1))

Every known answer below is derived by hand beside it, in the manner of tests/_tf_kat.py."""
import numpy as np

import _tf_kat as K

EPS32 = 2.0 ** -23                      # one fp32 ulp, relative to the value's magnitude (an upper bound)
TINY32 = 2.0 ** -149                    # the smallest fp32 subnormal: the absolute floor where g' g' underflows (or is flushed)
FLT_MAX = float(np.finfo(np.float32).max)


def f32(x):
    return float(np.float32(x))


def adam_step(var, m, v, g, b1p, b2p, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=0.0, stored=None):
    """One step in float64 from the fp32 state the kernel starts from (var, m, v, the two powers); lr, beta1, beta2, eps and clip as the
    fp32 values the kernel receives.  g' g' goes through fp32's range: a square beyond it is +inf, as in TF's float kernel, and a second
    moment that is +inf stays +inf (the limit of the convex combination beta2 v + (1 - beta2) g' g'; the incremental form would read
    inf - inf).  -> dict: var, m, v, b1p, b2p (the state after), gn (the norm before clipping), gs (g'), upd (what var moved by).
    stored = (m, v) as the kernel stored them in fp32: var and upd are then computed from THOSE.  The parameters' bound counts the roundings
    between the stored slots and var; the slots' own error is held to the slots' bounds, relative to max(|m_0|, |g'|) -- where m_0 and g'
    cancel, m is small against that magnitude and its admissible error, carried into the move, is many ulps of the move."""
    lr, beta1, beta2, eps, clip = (f32(x) for x in (lr, beta1, beta2, eps, clip))
    b1p, b2p = float(b1p), float(b2p)        # (as given: the fp32 values read from the device, or exact powers when the recursion is checked)
    var, m, v, g = (np.asarray(x, np.float64) for x in (var, m, v, g))
    gn = float(np.sqrt(np.dot(g.ravel(), g.ravel())))
    scale = clip / max(gn, clip) if clip > 0 else 1.0
    gs = g * scale
    g2 = gs * gs
    g2 = np.where(g2 > FLT_MAX, np.inf, g2)
    alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    m1 = m + (gs - m) * (1.0 - beta1)
    with np.errstate(invalid="ignore"):
        v1 = np.where(np.isinf(v), v, v + (g2 - v) * (1.0 - beta2))
    ms, vs = (m1, v1) if stored is None else (np.asarray(x, np.float64) for x in stored)
    upd = alpha * ms / (np.sqrt(vs) + eps)
    return dict(var=var - upd, m=m1, v=v1, b1p=b1p * beta1, b2p=b2p * beta2, gn=gn, gs=gs, upd=upd)


def tolerances(ref, var0, m0, v0, ulps_m=4, ulps_v=4, ulps_var=8):
    """The bounds of tests/test_adam_gpu.py for one step `ref` = adam_step(...) from (var0, m0, v0): ulps x 2^-23 x magnitude + the smallest
    fp32 subnormal, the magnitudes max(|m1|, |m0|, |g'|), max(|v1|, |v0|, g' g') and max(|var|, |alpha m / (sqrt v + eps)|).  The 8 of the
    parameters counts the roundings on their path: alpha 3 (sqrt, multiply, divide), sqrt v 1, + eps 1, divide 1, multiply 1, subtract 1."""
    a = np.abs
    g2 = np.minimum(ref["gs"] * ref["gs"], FLT_MAX)
    fin = lambda x: np.where(np.isfinite(x), x, 0.0)          # (an infinite v is compared exactly, not to a bound)
    tol_m = ulps_m * EPS32 * np.maximum(np.maximum(a(ref["m"]), a(np.asarray(m0, np.float64))), a(ref["gs"])) + TINY32
    tol_v = ulps_v * EPS32 * np.maximum(np.maximum(fin(ref["v"]), fin(np.asarray(v0, np.float64))), g2) + TINY32
    tol_p = ulps_var * EPS32 * np.maximum(a(ref["var"]), a(ref["upd"])) + TINY32
    return tol_m, tol_v, tol_p


# ---- constant gradient from zero slots (TF's adam_test.py testBasic: var0 [1, 2] with g 0.1, var1 [3, 4] with g 0.01, lr 0.001, the default
# beta1 0.9, beta2 0.999, eps 1e-8; three steps).
# With m_0 = v_0 = 0 and the same g every step, m_t = g (1 - beta1^t) and v_t = g^2 (1 - beta2^t) (geometric sums), and the powers the step
# reads are beta^t, so alpha_t = lr sqrt(1 - beta2^t) / (1 - beta1^t).  With s_t = sqrt(1 - beta2^t):
#     move_t = alpha_t m_t / (sqrt(v_t) + eps) = lr s_t g / (|g| s_t + eps) = lr sign(g) / (1 + eps / (|g| s_t))
# i.e. lr sign(g) to within eps / (|g| s_t): s_1 = sqrt(0.001) = 0.0316, so for g = 0.1 the relative shortfall is 1e-8 / 3.16e-3 = 3.2e-6
# (3e-9 of a move of 1e-3) and for g = 0.01 it is 3.2e-5.  Three steps: var0 = [1, 2] - 0.003 (1 - O(3e-6)) ~ [0.997, 1.997] and
# var1 = [3, 4] - 0.003 (1 - O(3e-5)) ~ [2.997, 3.997], the values adam_test.py asserts; afterwards the powers are beta^4.
BASIC_LR, BASIC_BETA1, BASIC_BETA2, BASIC_EPS, BASIC_STEPS = 0.001, 0.9, 0.999, 1e-8, 3
BASIC_VAR0, BASIC_G0 = np.array([1.0, 2.0]), 0.1
BASIC_VAR1, BASIC_G1 = np.array([3.0, 4.0]), 0.01
BASIC_ROUGH = (np.array([0.997, 1.997]), np.array([2.997, 3.997]))


def basic_move(g, t, lr=BASIC_LR, beta2=BASIC_BETA2, eps=BASIC_EPS):
    """move_t of the closed form above, the eps term written out (lr, beta2, eps as the fp32 values the kernel receives)"""
    lr, beta2, eps = f32(lr), f32(beta2), f32(eps)
    s_t = np.sqrt(1.0 - beta2 ** t)
    return lr * np.sign(g) / (1.0 + eps / (abs(g) * s_t))


def basic_expected(var, g, steps=BASIC_STEPS):
    """var after `steps` steps, m and v after them, and the two powers: the closed forms, not the recursion"""
    b1, b2 = f32(BASIC_BETA1), f32(BASIC_BETA2)
    out = np.asarray(var, np.float64) - sum(basic_move(g, t) for t in range(1, steps + 1))
    return out, g * (1.0 - b1 ** steps), g * g * (1.0 - b2 ** steps), b1 ** (steps + 1), b2 ** (steps + 1)


# ---- clipping, then Adam: tf.clip_by_global_norm's vectors (_tf_kat.CLIP_T0 / CLIP_T1, global norm 5) at clip 4 scale by 0.8.  From zero
# slots the first step has m_1 = (1 - beta1) g' = 0.8 (1 - beta1) g, v_1 = (1 - beta2) g'^2 and alpha_1 = lr sqrt(1 - beta2) / (1 - beta1),
# so the move is lr g' / (|g'| + eps / sqrt(1 - beta2)) = lr sign(g) / (1 + eps / (0.8 |g| s_1)): still lr sign(g), whatever the scale; a
# zero gradient does not move (0 / (0 + eps)).
CLIP_AT, CLIP_SCALE = 4.0, 0.8


def clip_expected(g, lr=BASIC_LR):
    """(move, m) of the first step for gradient entries g of the norm-5 vectors clipped at 4"""
    g = np.asarray(g, np.float64)
    b1, b2, eps, lr = f32(BASIC_BETA1), f32(BASIC_BETA2), f32(BASIC_EPS), f32(lr)
    gs = CLIP_SCALE * g
    with np.errstate(divide="ignore", invalid="ignore"):
        move = np.where(g != 0, lr * np.sign(g) / (1.0 + eps / (np.abs(gs) * np.sqrt(1.0 - b2))), 0.0)
    return move, CLIP_SCALE * (1.0 - b1) * g


CLIP_G = np.concatenate([K.CLIP_T0.ravel(), K.CLIP_T1])
