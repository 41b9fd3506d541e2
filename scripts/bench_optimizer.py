#!/usr/bin/env python3
"""Optimiser benchmark: dgp_sgd_momentum_clip against dgp_adam_clip on ONE trainer, called alternately and timed with hipEvents (the
norm pass and the update kernel of each call; no weight re-packing), median of `calls` calls after warm-up, for ResNet-50 / 4 joints and
ResNet-101 / 20 joints.  Achieved GB/s counts 24 B per parameter for momentum (norm pass 4; w, g, accum read, w, accum written 20) and
32 B for Adam (norm pass 4; w, g, m, v read, w, m, v written 28).  The momentum update is the yardstick: Adam's GB/s over momentum's in
the same run is reported per block of `calls` (`blocks` of them: the spread).  Then the 11-frame Trainer.step of scripts/bench_train.py
with hyper.optimizer "sgd" against "adam" on both tiers.

The stand-alone and the in-step figures differ by construction: behind the backward pass a gradient buffer of ~100 MB may still sit in
the 256 MiB Infinity Cache, while the alternating stand-alone calls stream 285 / 380 MB each and find little of it there.

`bench_optimizer.py [calls] [blocks] [steps] [--out PATH]` -> one JSON line, also written to profiles/optimizer_bench_line.json."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from deepgraphpose_amd import _lib, dataset as D
from deepgraphpose_amd.engine import _stream
from deepgraphpose_amd.loss import DGPHyper
from deepgraphpose_amd.synthetic import make_frames, make_weights
from deepgraphpose_amd.train import Trainer, _view

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "optimizer_bench_line.json")
if "--out" in sys.argv:
    args.remove(out_path)
calls = max(50, int(args[0])) if len(args) > 0 else 100
blocks = int(args[1]) if len(args) > 1 else 5
steps = int(args[2]) if len(args) > 2 else 20
WARM = 10
B_SGD, B_ADAM = 24, 32


def kernels(depth, nj):
    tr = Trainer(depth, nj, 64, 64, max_frames=1)
    tr.load_weights(make_weights(depth, nj, True, seed=0, head_std=0.05))
    lib, st, n = tr.lib, _stream(tr.device), tr.n_trainable
    tr.grads_tensor().normal_(0.0, 0.01)
    sgd = lambda: _lib.check(lib.dgp_sgd_momentum_clip(tr._t, 1e-6, 0.9, 10.0, None, st))
    adam = lambda: _lib.check(lib.dgp_adam_clip(tr._t, 1e-6, 0.9, 0.999, 1e-8, 10.0, None, st))
    for _ in range(WARM):
        sgd(); adam()
    per_block = []
    for _ in range(blocks):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(calls)]
        for e in ev:
            e[0].record(); sgd(); e[1].record(); adam(); e[2].record()
        torch.cuda.synchronize()
        ms_s = float(np.median([e[0].elapsed_time(e[1]) for e in ev]))
        ms_a = float(np.median([e[1].elapsed_time(e[2]) for e in ev]))
        per_block.append((ms_s, ms_a))
    ms_s, ms_a = (float(np.median([b[k] for b in per_block])) for k in (0, 1))
    gbs = lambda ms, b: b * n / (ms * 1e-3) / 1e9
    ratios = [gbs(a, B_ADAM) / gbs(s, B_SGD) for s, a in per_block]
    return {"net": "resnet_%d" % depth, "joints": nj, "n_trainable": n,
            "momentum": {"ms": round(ms_s, 4), "bytes_per_param": B_SGD, "GBps": round(gbs(ms_s, B_SGD), 1)},
            "adam": {"ms": round(ms_a, 4), "bytes_per_param": B_ADAM, "GBps": round(gbs(ms_a, B_ADAM), 1)},
            "adam_over_momentum_GBps": round(gbs(ms_a, B_ADAM) / gbs(ms_s, B_SGD), 3),
            "ratio_per_block": [round(r, 3) for r in ratios], "ratio_min_max": [round(min(ratios), 3), round(max(ratios), 3)],
            "blocks_ms": [[round(s, 4), round(a, 4)] for s, a in per_block]}


def step_ms(tier, optimizer):
    """scripts/bench_train.py's case and method: wall clock over `steps` Trainer.step calls between two synchronisations"""
    H, W, NJ, NT = 480, 640, 4, 11
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(make_frames(NT, H, W, NJ, seed=0)).cuda()
    jl = np.stack([rng.uniform(5, 55, (1, NJ)), rng.uniform(5, 75, (1, NJ))], -1)
    vm, hm, vt = D.gen_idx_chunk(np.array([5]), np.setdiff1d(np.arange(NT), [5]), jl)
    lt, lm = D.coord2map(jl, 60, 80, NJ, 17)
    lmap, lmask = np.zeros((NT, 60, 80, 2 * NJ), np.float32), np.zeros((NT, 60, 80, 2 * NJ), np.float32)
    lmap[5], lmask[5] = lt[0], lm[0]
    batch = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt)
    S0 = np.zeros((3, NJ))
    for i in range(3):
        S0[i, i], S0[i, i + 1] = 1, -1
    # (Adam moves every parameter by ~lr per step whatever its gradient: the learning rate TF's AdamOptimizer defaults to, not momentum's 0.005)
    hy = DGPHyper(gm2=1, gm3=3, optimizer=optimizer, lr=0.005 if optimizer == "sgd" else 0.001)
    tr = Trainer(50, NJ, H, W, max_frames=NT, tier=tier)
    tr.load_weights(make_weights(50, NJ, True, seed=0, head_std=0.05))
    ws, ws_max = np.full(3, 10.0), np.full(3, 200.0)
    for _ in range(3):
        tr.step(frames, batch, hy, S0, ws, ws_max, 2000.0, 50.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = tr.step(frames, batch, hy, S0, ws, ws_max, 2000.0, 50.0)
    torch.cuda.synchronize()
    return {"ms_per_step": round((time.perf_counter() - t0) / steps * 1e3, 3), "fast_passes": tr.fast_passes, "fast_redos": tr.fast_redos,
            "total_loss": round(losses["total_loss"], 4)}


res = {"metric": "optimizer_update", "calls_per_block": calls, "blocks": blocks, "timer": "hipEvents around each call, calls alternating",
       "kernels": [kernels(50, 4), kernels(101, 20)],
       "train_step_11_frames": {t: {o: step_ms(t, o) for o in ("sgd", "adam")} for t in ("parity", "f16")}, "steps": steps,
       "note": "stand-alone calls stream 285 / 380 MB (ResNet-50) and find little in the 256 MiB Infinity Cache; in the step the ~100 MB "
               "gradient buffer may still sit there right behind the backward pass, so the two figures differ"}
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
