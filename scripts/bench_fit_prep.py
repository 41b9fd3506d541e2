#!/usr/bin/env python3
"""Sample preparation of the fit drivers, host against device (prep_backend "host" | "hip"), on one box in alternation:

  fit_dlc        iterations per second of the real driver on the golden Reaching project (52 labeled 832 x 747 images, ResNet-50,
                 5 joints): the intervals between consecutive optimiser updates, median over >= 200 iterations after a warm-up
  fit_dgp step   Trainer.step on 11 synthetic frames (scripts/bench_train.py's batch) with the locref maps built as the driver builds
                 them -- _locref_targets on the host, _device_locref on the device -- at nj = 4 / 640 x 480 / ResNet-50 and at
                 nj = 20 / 1280 x 720 / ResNet-101; the preparation is timed inside the step (inline: what the prefetch thread would hide
                 only if it kept up) and on its own
  kernels        engine.target_maps and engine.window_resize alone, hipEvent-timed (the call's small table / entry upload included)

`bench_fit_prep.py [dlc_iters] [dgp_steps] [out.json]` -> one JSON line, also written to profiles/fit_prep_bench_line.json."""
import contextlib
import io
import json
import os
import random
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import yaml

from deepgraphpose_amd import dataset as D
from deepgraphpose_amd import engine, weights_io
from deepgraphpose_amd.loss import DGPHyper
from deepgraphpose_amd.models import fitdgp
from deepgraphpose_amd.staged import _device_locref
from deepgraphpose_amd.synthetic import make_frames, make_weights
from deepgraphpose_amd.train import Trainer

GOLDEN = os.path.join(ROOT, "tests", "golden")
dlc_iters = int(sys.argv[1]) if len(sys.argv) > 1 else 110
dgp_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "fit_prep_bench_line.json")
WARM = 20


def reaching_project(root):
    """The Reaching demo project from the files under tests/golden, its paths made absolute, with a seeded ResNet-50 start snapshot"""
    proj = os.path.join(root, "Reaching-Mackenzie-2018-08-30")
    shutil.copytree(os.path.join(GOLDEN, "reaching_project"), proj)
    shutil.copytree(os.path.join(GOLDEN, "reaching_frames"), os.path.join(proj, "labeled-data", "reachingvideo1"))
    ts = os.path.join(proj, "training-datasets", "iteration-0", "UnaugmentedDataSet_ReachingAug30")
    os.makedirs(ts)
    shutil.copy(os.path.join(GOLDEN, "Reaching_Mackenzie95shuffle1.mat"), ts)
    train = os.path.join(proj, "dlc-models", "iteration-0", "ReachingAug30-trainset95shuffle1", "train")
    for path in (os.path.join(proj, "config.yaml"), os.path.join(train, "pose_cfg.yaml")):
        with open(path) as f:
            cfg = yaml.safe_load(f)
        cfg["project_path"] = proj
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
    weights_io.save_weights(os.path.join(train, "snapshot-start"), make_weights(50, 5, True, seed=0, head_std=0.05))
    return proj, train


def time_fit_dlc(proj, train, backend, iters):
    """one fit_dlc run of WARM + iters iterations -> the seconds between consecutive optimiser updates after the warm-up"""
    stamps = []
    apply = Trainer.apply_gradients

    def stamped(self, *a, **k):
        r = apply(self, *a, **k)                 # (reads the gradient norm back: the step is over when it returns)
        stamps.append(time.perf_counter())
        return r
    Trainer.apply_gradients = stamped
    np.random.seed(0)
    random.seed(0)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fitdgp.fit_dlc("snapshot-start", proj, maxiters=WARM + iters, displayiters=10 ** 9, saveiters=10 ** 9, prep_backend=backend)
    finally:
        Trainer.apply_gradients = apply
    assert fitdgp.PREP_STATS["backend"] == backend
    for f in os.listdir(train):
        if f.startswith("snapshot-step0") or f == "checkpoint":
            os.remove(os.path.join(train, f))
    return np.diff(stamps)[WARM:]


def bench_fit_dlc():
    os.environ["DGP_SNAPSHOT_FORMAT"] = "npz"
    with tempfile.TemporaryDirectory() as tmp:
        proj, train = reaching_project(tmp)
        dt = {"host": [], "hip": []}
        for backend in ("host", "hip", "host", "hip"):
            dt[backend].append(time_fit_dlc(proj, train, backend, iters=dlc_iters))
    res = {}
    for backend, runs in dt.items():
        allv = np.concatenate(runs)
        res[backend] = dict(iterations=int(allv.size), ms_median=round(float(np.median(allv)) * 1e3, 3),
                            ms_p10=round(float(np.percentile(allv, 10)) * 1e3, 3), ms_p90=round(float(np.percentile(allv, 90)) * 1e3, 3),
                            it_per_s=round(1.0 / float(np.median(allv)), 2), runs_ms_median=[round(float(np.median(r)) * 1e3, 3) for r in runs])
    res["hip_over_host_it_per_s"] = round(res["hip"]["it_per_s"] / res["host"]["it_per_s"], 3)
    res["workload"] = "fit_dlc on the Reaching project: ResNet-50, 5 joints, batch 1, crop 0.4, scale 0.8 x U(0.75, 1.25), PREFETCH_DEPTH %d" % fitdgp.PREFETCH_DEPTH
    return res


def bench_dgp_step(depth, nj, H, W, steps):
    NT = 11
    rng = np.random.default_rng(0)
    nx, ny = D.compute_pred_dims(H, W)
    tr = Trainer(depth, nj, H, W, max_frames=NT)
    tr.load_weights(make_weights(depth, nj, True, seed=0, head_std=0.05))
    frames = torch.from_numpy(make_frames(NT, H, W, nj, seed=0)).cuda()
    jl = np.stack([rng.uniform(5, nx - 5, (1, nj)), rng.uniform(5, ny - 5, (1, nj))], -1)
    vm, hm, vt = D.gen_idx_chunk(np.array([5]), np.setdiff1d(np.arange(NT), [5]), jl)
    nl = nj - 1
    S0 = np.zeros((nl, nj))
    for i in range(nl):
        S0[i, i], S0[i, i + 1] = 1, -1
    hy, ws, ws_max = DGPHyper(gm2=1, gm3=3), np.full(nl, 10.0), np.full(nl, 200.0)
    cfg = type("Cfg", (), dict(pos_dist_thresh=17, locref_stdev=7.2801))
    prep = {"host": lambda: fitdgp._locref_targets(jl, NT, [5], nx, ny, nj, cfg),
            "hip": lambda: _device_locref(None, tr.device, jl, NT, [5], nx, ny, nj, cfg)}

    def step(backend):
        lmap, lmask = prep[backend]()
        batch = dict(targets=jl, locref_map=lmap, locref_mask=lmask, visible_marker=vm, hidden_marker=hm, visible_marker_in_targets=vt)
        return tr.step(frames, batch, hy, S0, ws, ws_max, 2000.0, 50.0)

    res = {}
    for backend in ("host", "hip", "host", "hip"):           # alternated; the second block of each is reported
        for _ in range(3):
            step(backend)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            losses = step(backend)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        t0 = time.perf_counter()
        for _ in range(steps):
            prep[backend]()
        torch.cuda.synchronize()
        res[backend] = dict(ms_per_step=round(ms, 3), prep_alone_ms=round((time.perf_counter() - t0) / steps * 1e3, 3),
                            total_loss=round(losses["total_loss"], 5))
    res.update(net="resnet_%d" % depth, nj=nj, H=H, W=W, nt=NT, steps=steps, maps_MB=round(2 * NT * nx * ny * 2 * nj * 4 / 1e6, 2),
               hip_over_host_steps_per_s=round(res["host"]["ms_per_step"] / res["hip"]["ms_per_step"], 3))
    del tr
    torch.cuda.empty_cache()
    return res


def event_ms(fn, calls=100):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(float(np.median(ms)), 4), ms_p10=round(float(np.percentile(ms, 10)), 4),
                ms_p90=round(float(np.percentile(ms, 90)), 4), calls=calls)


def bench_kernels():
    rng = np.random.default_rng(0)
    res = {}

    def maps_case(n, H, W, nj, dgp):
        k = nj
        ent = np.column_stack([np.arange(k, dtype=np.float64), rng.uniform(8, W * 8 - 8, k), rng.uniform(8, H * 8 - 8, k)])
        off = np.zeros(n + 1, np.int32)
        off[n // 2 + 1:] = k                                  # one labeled frame, like a DGP window
        kw = dict(scmap=None, weights=None) if dgp else {}
        r = event_ms(lambda: engine.target_maps(ent, off, n, H, W, nj, pos_dist_thresh=17, **kw))
        r["written_MB"] = round(n * H * W * nj * 4 * (4 if dgp else 6) / 1e6, 3)
        return r
    res["target_maps 1x76x84x5 four maps (fit_dlc)"] = maps_case(1, 76, 84, 5, False)
    res["target_maps 11x60x80x8 locref (fit_dgp nj=4)"] = maps_case(11, 60, 80, 4, True)
    res["target_maps 11x90x160x40 locref (fit_dgp nj=20)"] = maps_case(11, 90, 160, 20, True)
    img = torch.from_numpy(rng.integers(0, 256, (747, 832, 3), dtype=np.uint8)).cuda()
    res["window_resize 747x832 -> 598x666 box"] = event_ms(lambda: engine.window_resize(img, None, (598, 666), "box"))
    res["window_resize 747x832 -> 747x832 x 1.0 bilinear"] = event_ms(lambda: engine.window_resize(img, None, (747, 832), "bilinear"))
    res["window_resize window 401x433 at (203,101) -> 321x346 box, mirrored"] = event_ms(
        lambda: engine.window_resize(img, (203, 101, 203 + 432, 101 + 400), (321, 346), "box", True))
    res["note"] = "engine-level calls on the current stream: the coefficient tables / entries are built on the host and uploaded inside the timed span"
    return res


out = {"metric": "fit_prep", "device": torch.cuda.get_device_name(0)}
out["kernels"] = bench_kernels()
out["fit_dgp_step"] = [bench_dgp_step(50, 4, 480, 640, dgp_steps), bench_dgp_step(101, 20, 720, 1280, dgp_steps)]
out["fit_dlc"] = bench_fit_dlc()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
