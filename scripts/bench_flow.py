#!/usr/bin/env python3
"""Farneback flow (csrc/dgp_flow.hip, engine.optical_flow) on BASELINE configs[3]'s batch: 11 frames of 640x480, the reference's
parameters (0.5, 3, 15, 3, 5, 1.2), magnitude only.  Median of >= 50 hipEvent-timed calls after warm-up; algorithmic bytes from the
shapes (every kernel's compulsory reads and writes once) and their share of the HBM roof.  `bench_flow.py [calls] [train_steps]`:
with train_steps > 0 the Trainer step of scripts/bench_train.py is also timed with wt = 0 and with wt = 50 (flow computed on the
device every step, as fit_dgp does).  One JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np, torch
from deepgraphpose_amd import engine, _lib

T, H, W = 11, 480, 640
PARAMS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
train_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 0


def frames_moving(T, H, W, seed=0):
    """A smooth texture moved by a few pixels per frame (uint8 BGR)."""
    rng = np.random.default_rng(seed)
    ky, kx = np.fft.fftfreq(H + 64)[:, None], np.fft.fftfreq(W + 64)[None, :]
    tex = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((H + 64, W + 64))) * np.exp(-2 * (np.pi * 3) ** 2 * (kx ** 2 + ky ** 2))))
    tex = np.clip(128 + 60 * tex / tex.std(), 0, 255).astype(np.uint8)
    off = np.cumsum(rng.integers(-3, 4, (T, 2)), 0) + 32
    return np.stack([np.repeat(tex[oy:oy + H, ox:ox + W, None], 3, -1) for ox, oy in np.clip(off, 0, 64)])


def algorithmic_bytes(T, H, W, levels_used, iterations):
    P, b = T - 1, T * H * W * (3 + 4)                        # gray: uint8 BGR in, fp32 out
    prev = 0
    for k in range(levels_used, -1, -1):
        s = PARAMS["pyr_scale"] ** k
        n = int(np.rint(W * s)) * int(np.rint(H * s))
        b += T * H * W * 4 + T * n * 4                       # blur + resize: full-resolution gray in, level image out
        b += T * n * 4 + T * n * 5 * 4                       # polynomial expansion: level image in, 5 planes out
        b += P * (prev * 8 + n * (5 + 5) * 4 + n * (8 + 20))  # first M: coarse flow, R0, R1 in; flow, M out
        b += P * n * (iterations - 1) * (20 + 40 + 8 + 20)  # passes with an M update: M, R0, R1 in; flow, M out
        b += P * n * (20 + 8 + (4 if k == 0 else 0))        # last pass: M in, flow (+ magnitude at level 0) out
        prev = n
    return b


lib = _lib.load()
prm = _lib.DgpFlowParams(PARAMS["pyr_scale"], PARAMS["levels"], PARAMS["winsize"], PARAMS["iterations"], PARAMS["poly_n"],
                         PARAMS["poly_sigma"], 0)
nb, used = C.c_size_t(), C.c_int32()
_lib.check(lib.dgp_optical_flow_scratch_bytes(T, H, W, C.byref(prm), C.byref(nb), C.byref(used)))
dev = torch.from_numpy(frames_moving(T, H, W)).cuda()
for _ in range(5):
    mag = engine.optical_flow(dev, **PARAMS)
torch.cuda.synchronize()
ms = []
for _ in range(max(calls, 50)):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    mag = engine.optical_flow(dev, **PARAMS)
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
med = float(np.median(ms))
nbytes = algorithmic_bytes(T, H, W, used.value, PARAMS["iterations"])
out = {"kernel": "optical_flow", "frames": T, "H": H, "W": W, "params": PARAMS, "levels_used": used.value,
       "launches": 1 + (used.value + 1) * (3 + PARAMS["iterations"]), "calls": len(ms), "ms_median": round(med, 4),
       "ms_p10": round(float(np.percentile(ms, 10)), 4), "ms_p90": round(float(np.percentile(ms, 90)), 4),
       "algorithmic_MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med / 1e6, 1), "hbm_peak_GB_per_s": 8000,
       "frac_hbm_roof": round(nbytes / med / 1e6 / 8000, 3), "scratch_MB": round(nb.value / 1e6, 1),
       "includes": "scratch allocation from torch's cache + every flow kernel; magnitude only",
       "mean_magnitude": round(float(mag.mean()), 4)}

if train_steps > 0:                                          # Trainer step, wt = 0 vs wt = 50 (flow on the device every step)
    import time
    from deepgraphpose_amd.train import Trainer
    from deepgraphpose_amd.loss import DGPHyper
    from deepgraphpose_amd import dataset as D
    from deepgraphpose_amd.synthetic import make_weights
    NJ = 4
    rng = np.random.default_rng(0)
    wts = make_weights(50, NJ, True, seed=0, head_std=0.05)
    jl = np.stack([rng.uniform(5, 55, (1, NJ)), rng.uniform(5, 75, (1, NJ))], -1)
    vm, hm, vt = D.gen_idx_chunk(np.array([5]), np.setdiff1d(np.arange(T), [5]), jl)
    lt, lm = D.coord2map(jl, 60, 80, NJ, 17)
    lmap, lmask = np.zeros((T, 60, 80, 2 * NJ), np.float32), np.zeros((T, 60, 80, 2 * NJ), np.float32)
    lmap[5], lmask[5] = lt[0], lm[0]
    S0 = np.zeros((3, NJ)); [S0.__setitem__((i, i), 1) or S0.__setitem__((i, i + 1), -1) for i in range(3)]
    ws, ws_max = np.full(3, 10.0), np.full(3, 200.0)
    tr = Trainer(50, NJ, H, W, max_frames=T)
    tr.load_weights(wts)
    res = {}
    for wt in (0.0, 50.0, 0.0, 50.0):                        # alternated; the second of each is reported
        hy = DGPHyper(gm2=1, gm3=3, wt=wt)
        base = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt)

        def step():
            b = dict(base, vector_field=engine.optical_flow(dev, **PARAMS)) if wt > 0 else base
            return tr.step(dev, b, hy, S0, ws, ws_max, 2000.0, 50.0)
        for _ in range(3):
            losses = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(train_steps):
            losses = step()
        torch.cuda.synchronize()
        res["wt%g" % wt] = dict(ms_per_step=round((time.perf_counter() - t0) / train_steps * 1e3, 3),
                                wt_loss=round(losses.get("wt_loss", 0.0), 5), total_loss=round(losses["total_loss"], 5))
    out["train_step"] = dict(res, steps=train_steps, tier="parity", note="Trainer.step at configs[3]; wt = 50 includes engine.optical_flow")
print(json.dumps(out))
