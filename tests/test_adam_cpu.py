"""The Adam optimiser without a GPU: the float64 restatement against its hand-derived answers (tests/_adam_ref.py), optimiser slots through
the checkpoint reader, the C-ABI's declaration and export, and the names the Python layers accept."""
import os
import re
import subprocess

import numpy as np
import pytest

import _adam_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(var, g, steps, clip=0.0, lr=A.BASIC_LR):
    st = dict(var=np.asarray(var, np.float64), m=np.zeros_like(var, dtype=np.float64), v=np.zeros_like(var, dtype=np.float64),
              b1p=A.f32(A.BASIC_BETA1), b2p=A.f32(A.BASIC_BETA2))         # the powers start at the fp32 betas
    for _ in range(steps):
        st = A.adam_step(st["var"], st["m"], st["v"], g, st["b1p"], st["b2p"], lr, A.BASIC_BETA1, A.BASIC_BETA2, A.BASIC_EPS, clip)
    return st


def test_helper_reproduces_the_constant_gradient_closed_form():
    """adam_test.py testBasic: three steps of the recursion equal the closed forms (moves with the eps term written out, m, v, powers) and
    land on the values TensorFlow's test asserts."""
    for var, g, rough in ((A.BASIC_VAR0, A.BASIC_G0, A.BASIC_ROUGH[0]), (A.BASIC_VAR1, A.BASIC_G1, A.BASIC_ROUGH[1])):
        st = _run(var, np.full(2, g), A.BASIC_STEPS)
        want, m, v, b1p, b2p = A.basic_expected(var, g)
        np.testing.assert_allclose(st["var"], want, rtol=1e-13)
        np.testing.assert_allclose(st["m"], m, rtol=1e-13)
        np.testing.assert_allclose(st["v"], v, rtol=1e-12)
        np.testing.assert_allclose([st["b1p"], st["b2p"]], [b1p, b2p], rtol=1e-13)
        np.testing.assert_allclose(st["var"], rough, atol=1e-6)            # 0.003 short by eps / (|g| s_t): < 3 * 1e-3 * 3.2e-5 = 1e-7
        # each move is lr sign(g) to within eps / (|g| s_t), s_1 = sqrt(1 - beta2) being the smallest s_t
        short = A.f32(A.BASIC_EPS) / (g * np.sqrt(1.0 - A.f32(A.BASIC_BETA2)))
        for t in range(1, 4):
            assert 0 <= 1.0 - A.basic_move(g, t) / A.f32(A.BASIC_LR) <= short
    assert abs(st["b1p"] - 0.9 ** 4) < 1e-7 and abs(st["b2p"] - 0.999 ** 4) < 1e-7        # (fp32 0.9 / 0.999 against the decimals)


def test_helper_clips_then_applies_adam():
    """The norm-5 vectors at clip 4: the norm is 5, g' = 0.8 g, the first move is still lr sign(g) and m = 0.8 (1 - beta1) g."""
    st = _run(np.zeros(8), A.CLIP_G, 1, clip=A.CLIP_AT)
    move, m = A.clip_expected(A.CLIP_G)
    assert st["gn"] == 5.0
    np.testing.assert_allclose(st["gs"], 0.8 * A.CLIP_G, rtol=1e-15)
    np.testing.assert_allclose(-st["var"], move, rtol=1e-13, atol=0)
    np.testing.assert_allclose(st["m"], m, rtol=1e-13, atol=0)
    nz = A.CLIP_G != 0
    np.testing.assert_allclose(-st["var"][nz], A.f32(A.BASIC_LR) * np.sign(A.CLIP_G[nz]), rtol=1e-6)
    assert not st["var"][~nz].any()


def test_helper_squares_through_fp32_range():
    st = A.adam_step([1.0], [0.0], [0.0], [1e20], 0.9, 0.999, 0.001)
    assert st["v"][0] == np.inf and st["var"][0] == 1.0 and st["upd"][0] == 0.0
    st = A.adam_step(st["var"], st["m"], st["v"], [0.0], st["b1p"], st["b2p"], 0.001)
    assert st["v"][0] == np.inf and st["var"][0] == 1.0 and np.isfinite(st["m"][0])


def test_checkpoint_slots_are_kept_on_request_only(tmp_path):
    """A bundle holding x, its three slots and the two powers: load_checkpoint(slots=True) returns all six, weights_io.load_optimizer_state
    the five optimiser entries, and the default load_checkpoint x alone."""
    from deepgraphpose_amd import tf_checkpoint, weights_io
    rng = np.random.RandomState(0)
    t = {"x": rng.randn(3, 4).astype(np.float32)}
    for sfx in ("/Adam", "/Adam_1", "/Momentum"):
        t["x" + sfx] = rng.randn(3, 4).astype(np.float32)
    t["beta1_power"] = np.float32(0.9 ** 4).reshape(())
    t["beta2_power"] = np.float32(0.999 ** 4).reshape(())
    prefix = str(tmp_path / "snapshot-5")
    tf_checkpoint.write_v2(prefix, t)
    full = tf_checkpoint.load_checkpoint(prefix, slots=True)
    assert sorted(full) == sorted(t)
    for k, a in t.items():
        assert full[k].shape == a.shape and np.array_equal(full[k], a), k
    state = weights_io.load_optimizer_state(prefix)
    assert sorted(state) == sorted(k for k in t if k != "x")
    assert state["beta1_power"].shape == () and state["beta1_power"] == t["beta1_power"]
    assert all(np.array_equal(state[k], t[k]) for k in state)
    assert list(tf_checkpoint.load_checkpoint(prefix)) == ["x"]
    assert list(weights_io.load_weights(prefix)) == ["x"]


def test_header_declares_and_library_exports_dgp_adam_clip(lib_built):
    with open(os.path.join(ROOT, "include", "dgp_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+dgp_adam_clip\s*\(\s*dgp_trainer\s*\*\s*tr\s*,\s*float lr\s*,\s*float beta1\s*,\s*float beta2\s*,\s*float eps\s*,"
                     r"\s*float clip_norm\s*,\s*float\s*\*\s*gnorm_host_or_null\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    from deepgraphpose_amd import _lib
    assert "dgp_adam_clip" in _lib.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", lib_built], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT dgp_adam_clip$", out, re.M)


def test_unknown_optimizer_names_are_refused():
    from deepgraphpose_amd.loss import DGPHyper
    from deepgraphpose_amd.models.fitdgp import resolve_optimizer
    from deepgraphpose_amd.models.session import LossGraph
    assert DGPHyper().optimizer == "sgd"
    assert (DGPHyper().beta1, DGPHyper().beta2, DGPHyper().adam_eps) == (0.9, 0.999, 1e-8)
    graph = LossGraph(DGPHyper(), np.zeros((0, 3)), np.zeros(0), np.zeros(0), 10.0, 2.0, 3)
    with pytest.raises(ValueError, match="unknown optimizer nope"):
        graph.minimize(graph.total_loss, 0.005, optimizer="nope")
    assert graph.minimize(graph.total_loss, 0.005).optimizer == "sgd"
    assert graph.minimize(graph.total_loss_visible, 0.005, optimizer="adam").optimizer == "adam"
    with pytest.raises(ValueError, match="unknown optimizer nope"):
        resolve_optimizer("nope")
    with pytest.raises(ValueError, match="unknown optimizer rmsprop"):
        resolve_optimizer(None, "rmsprop")                               # pose_cfg.yaml's key, when the argument is None
    assert resolve_optimizer(None, "adam") == "adam" and resolve_optimizer("sgd", "adam") == "sgd" and resolve_optimizer() == "sgd"
