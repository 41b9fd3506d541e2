"""Known answers TensorFlow's own unit tests assert for conv2d (tensorflow/python/kernel_tests/conv_ops_test.py, class Conv2DTest), restated
as data: the test's name, input shape (NHWC), filter shape (HWIO), stride, padding and the expected output (row-major NHWC).  As in
`_SetupValuesForDevice`, both tensors are filled with 1, 2, 3, ... in row-major order.  Used by tests/test_oracle_cpu.py (the oracle) and
tests/test_parity_gpu.py (the product's conv kernel through the C-ABI)."""
import numpy as np

TF_CONV2D_KNOWN_ANSWERS = [
    ("testConv2D1x1Filter", (1, 2, 3, 3), (1, 1, 3, 3), 1, "VALID",
     [30.0, 36.0, 42.0, 66.0, 81.0, 96.0, 102.0, 126.0, 150.0, 138.0, 171.0, 204.0, 174.0, 216.0, 258.0, 210.0, 261.0, 312.0]),
    ("testConv2D2x2Filter", (1, 2, 3, 3), (2, 2, 3, 3), 1, "VALID", [2271.0, 2367.0, 2463.0, 2901.0, 3033.0, 3165.0]),
    ("testConv2D2x2FilterStride2", (1, 2, 3, 3), (2, 2, 3, 3), 2, "VALID", [2271.0, 2367.0, 2463.0]),
    ("testConv2D2x2FilterStride2Same", (1, 2, 3, 3), (2, 2, 3, 3), 2, "SAME", [2271.0, 2367.0, 2463.0, 1230.0, 1305.0, 1380.0]),
    ("testConv2D1x2Filter", (1, 2, 3, 3), (1, 2, 3, 3), 1, "VALID",
     [231.0, 252.0, 273.0, 384.0, 423.0, 462.0, 690.0, 765.0, 840.0, 843.0, 936.0, 1029.0]),
    ("testConv2DKernelSmallerThanStrideValid (3x3)", (1, 3, 3, 1), (1, 1, 1, 1), 2, "VALID", [1, 3, 7, 9]),
    ("testConv2DKernelSmallerThanStrideValid (7x7)", (1, 7, 7, 1), (2, 2, 1, 1), 3, "VALID", [65, 95, 275, 305]),
    ("testConv2DKernelSmallerThanStrideSame (3x3)", (1, 3, 3, 1), (1, 1, 1, 1), 2, "SAME", [1, 3, 7, 9]),
    ("testConv2DKernelSmallerThanStrideSame (4x4)", (1, 4, 4, 1), (1, 1, 1, 1), 2, "SAME", [1, 3, 9, 11]),
    ("testConv2DKernelSizeMatchesInputSize", (1, 2, 2, 1), (2, 2, 1, 2), 1, "VALID", [50.0, 60.0]),
]


def tf_test_values(shape):
    """_SetupValuesForDevice: 1, 2, 3, ... in row-major order"""
    return np.arange(1, int(np.prod(shape)) + 1, dtype=np.float32).reshape(shape)


def tf_out_and_pads(size, k, stride, padding):
    """TF's output size and (before, after) padding of one spatial axis (common_shape_fns / the SAME rule: the extra pixel goes AFTER)"""
    if padding == "VALID":
        return (size - k) // stride + 1, 0, 0
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2, total - total // 2


def brute_force(in_shape, f_shape, stride, padding):
    """the definition, in float64 loops: what the published vectors are re-derived from before anything is held to them"""
    x, w = tf_test_values(in_shape).astype(np.float64), tf_test_values(f_shape).astype(np.float64)
    n, h, wd, _ = in_shape
    kh, kw, _, co = f_shape
    oh, pt, _ = tf_out_and_pads(h, kh, stride, padding)
    ow, pl, _ = tf_out_and_pads(wd, kw, stride, padding)
    y = np.zeros((n, oh, ow, co))
    for i in range(oh):
        for j in range(ow):
            for a in range(kh):
                for b in range(kw):
                    r, c = i * stride + a - pt, j * stride + b - pl
                    if 0 <= r < h and 0 <= c < wd:
                        y[:, i, j] += x[:, r, c] @ w[a, b]
    return y


# ---- the training step's tail: losses and optimiser -------------------------------------------------------------------------
# Closed forms of the TF ops fit_dgp / pose_net.train build their loss and update from.  Every number is derived by hand beside it,
# so they pin the oracle (tests/test_oracle_cpu.py) and the kernels (tests/test_optimizer_gpu.py, tests/test_loss_edges_gpu.py) to
# the definitions instead of to each other.

# tf.losses.sigmoid_cross_entropy, reduction SUM_BY_NONZERO_WEIGHTS (losses_test.py SigmoidCrossEntropyLossTest).
# Per element ce = max(x, 0) - x z + log1p(exp(-|x|)); at |x| = 100 the log1p term is 4e-44, so a right element costs 0 and a
# wrong one costs 100.
CE_LOGITS = np.array([[100.0, -100.0, -100.0], [-100.0, 100.0, -100.0], [-100.0, -100.0, 100.0]])
CE_LABELS_RIGHT = np.eye(3)
CE_LABELS_WRONG = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
CE_KNOWN_ANSWERS = [
    # (name, labels, weights or None, expected loss)
    ("all right", CE_LABELS_RIGHT, None, 0.0),                               # every element right: 0 / 9
    ("all wrong", CE_LABELS_WRONG, None, 600.0 / 9.0),                       # two wrong elements per row, 100 each: 600 / 9
    # per-element weights: wrong elements (0,0) (0,2) (1,0) (1,1) (2,1) (2,2) weigh 3+5+2+6+0+1 = 17 -> 1700; 7 weights are non-zero
    ("all wrong, element weights", CE_LABELS_WRONG, np.array([[3.0, 4.0, 5.0], [2.0, 6.0, 0.0], [8.0, 0.0, 1.0]]), 1700.0 / 7.0),
    ("all wrong, all weights zero", CE_LABELS_WRONG, np.zeros((3, 3)), 0.0),  # no non-zero weight: 0, not 0 / 0
]
# One weight per marker, broadcast over its H x W map ([n, 1, 1]): two markers (the 3 x 3 map above, all wrong, 600 each) weighing 3
# and 0.  Sum 3 * 600 = 1800; the denominator counts the BROADCAST weights, H * W = 9 per non-zero marker: 1800 / 9 = 200.
CE_MARKER_WEIGHTS = np.array([3.0, 0.0])
CE_MARKER_WEIGHTS_LOSS = 200.0

# tf.losses.huber_loss, delta 1: 0.5 d^2 for |d| <= 1, |d| - 0.5 beyond (both give 0.5 at |d| = 1)
HUBER_D = np.array([0.0, 0.5, 1.0, 3.0, -2.0])
HUBER_EL = np.array([0.0, 0.125, 0.5, 2.5, 1.5])                           # 0; .5 * .25; .5 * 1; 3 - .5; 2 - .5
HUBER_MASK = np.array([1.0, 1.0, 0.0, 1.0, 0.0])
HUBER_MEAN = 4.625 / 5.0                                                   # mask all ones: (0 + .125 + .5 + 2.5 + 1.5) / 5
HUBER_MASKED = 2.625 / 3.0                                                 # mask above: (0 + .125 + 2.5) / 3 non-zero
# tf.losses.mean_squared_error with the same mask (the locref_huber_loss=False branch): (0 + .25 + 9) / 3
MSE_MASKED = 9.25 / 3.0

# tf.clip_by_global_norm (clip_ops_test.py testClipByGlobalNorm / ...NotClipped): global norm sqrt(4 + 16 + 1 + 4) = 5
CLIP_T0 = np.array([[-2.0, 0.0, 0.0], [4.0, 0.0, 0.0]])
CLIP_T1 = np.array([1.0, -2.0])
CLIP_NORM = 5.0
CLIP_AT_4 = (np.array([[-1.6, 0.0, 0.0], [3.2, 0.0, 0.0]]), np.array([0.8, -1.6]))     # scale 4 / 5
CLIP_AT_6 = (CLIP_T0, CLIP_T1)                                                           # 5 <= 6: unchanged

# tf.train.MomentumOptimizer (momentum_test.py testBasic): lr 2, momentum 0.9, accum = m accum + g, var -= lr accum.
# var0 [1, 2] with g 0.1: accum 0.1 -> var 1 - 0.2; accum 0.9 * 0.1 + 0.1 = 0.19 -> var 0.8 - 0.38
# var1 [3, 4] with g 0.01: accum 0.01 -> var 3 - 0.02; accum 0.019 -> var 2.98 - 0.038
MOMENTUM_LR, MOMENTUM_M = 2.0, 0.9
MOMENTUM_VAR0, MOMENTUM_G0 = np.array([1.0, 2.0]), 0.1
MOMENTUM_VAR1, MOMENTUM_G1 = np.array([3.0, 4.0]), 0.01
MOMENTUM_STEPS = [(np.array([0.8, 1.8]), np.array([2.98, 3.98])), (np.array([0.42, 1.42]), np.array([2.942, 3.942]))]
