#!/usr/bin/env python3
"""The DGP drivers' device frame store (fit_dgp(frame_store="off" | "hip")) on one box, in alternation:

  fit_dgp   the real driver (ResNet-50, batch_size 10, gm2 = 1, gm3 = 3) on the golden Reaching project with a LabeledDirSource over
            tests/golden/reaching_frames as its video (832 x 747 PNGs: every frame_at opens and decodes one), "off" and "hip" alternating,
            both tiers, aug on and off: the seconds between the returns of consecutive TrainSession.run calls, median after a warm-up;
            the store's fill time on its own, and the iteration count from which fill + hip iterations is less than the off iterations
  kernel    engine.gather_frames for 11 x 480 x 640 and 11 x 720 x 1280 against the 11 device-to-device frame copies it replaces,
            hipEvent-timed, alternating blocks; GB/s counts the bytes read plus the bytes written

`bench_frame_store.py [iters] [out.json]` -> one JSON line, also written to profiles/frame_store_bench_line.json.  The "off" figure is the
price of this source's decoder (Pillow on PNGs), not a constant: a stack in memory costs less per frame, a seeking video decoder more."""
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

from deepgraphpose_amd import engine, weights_io
from deepgraphpose_amd.frames import LabeledDirSource
from deepgraphpose_amd.models import fitdgp, session
from deepgraphpose_amd.models.staging import slot_stride
from deepgraphpose_amd.synthetic import make_weights

GOLDEN = os.path.join(ROOT, "tests", "golden")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "frame_store_bench_line.json")
WARM = 6
HBM_PEAK_GBS = 8000.0


def reaching_project(root):
    """The Reaching demo project from the files under tests/golden (as scripts/bench_fit_prep.py assembles it), with a seeded start snapshot"""
    proj = os.path.join(root, "Reaching-Mackenzie-2018-08-30")
    shutil.copytree(os.path.join(GOLDEN, "reaching_project"), proj)
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


def time_fit_dgp(proj, train, frame_store, aug, tier, n):
    """one fit_dgp run of WARM + n iterations -> (seconds between consecutive iterations after the warm-up, the store's stats)"""
    stamps = []
    run = session.TrainSession.run

    def stamped(self, *a, **k):
        r = run(self, *a, **k)                   # (reads the losses and the gradient norm back: the step is over when it returns)
        stamps.append(time.perf_counter())
        return r
    session.TrainSession.run = stamped
    os.environ["DGP_TRAIN_TIER"] = tier
    np.random.seed(0)
    random.seed(0)
    source = LabeledDirSource(os.path.join(GOLDEN, "reaching_frames"))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fitdgp.fit_dgp("snapshot-start", proj, batch_size=10, maxiters=WARM + n, displayiters=10 ** 9, saveiters=10 ** 9, gm2=1, gm3=3,
                           n_max_frames=150, aug=aug, frame_sources=[source], frame_store=frame_store)
    finally:
        session.TrainSession.run = run
        os.environ.pop("DGP_TRAIN_TIER")
    assert len(stamps) == WARM + n, len(stamps)
    for f in os.listdir(train):
        if f.startswith("snapshot-step2") or f == "checkpoint":
            os.remove(os.path.join(train, f))
    return np.diff(stamps)[WARM - 1:], fitdgp.PREP_STATS["frame_store"]


def bench_fit_dgp():
    os.environ["DGP_SNAPSHOT_FORMAT"] = "npz"
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        proj, train = reaching_project(tmp)
        for tier in ("parity", "f16"):
            for aug in (False, True):
                dt, fills, stats = {"off": [], "hip": []}, [], None
                for mode in ("off", "hip", "off", "hip"):
                    d, st = time_fit_dgp(proj, train, mode, aug, tier, iters)
                    dt[mode].append(d)
                    if st is not None:
                        fills.append(st["fill_s"])
                        stats = st
                row = dict(tier=tier, aug=aug)
                for mode, runs in dt.items():
                    allv = np.concatenate(runs)
                    row[mode] = dict(iterations=int(allv.size), ms_median=round(float(np.median(allv)) * 1e3, 3),
                                     ms_p10=round(float(np.percentile(allv, 10)) * 1e3, 3), ms_p90=round(float(np.percentile(allv, 90)) * 1e3, 3),
                                     runs_ms_median=[round(float(np.median(r)) * 1e3, 3) for r in runs])
                gain = (row["off"]["ms_median"] - row["hip"]["ms_median"]) / 1e3
                row.update(fill_s=[round(f, 3) for f in fills], stored_frames=stats["frames"], stored_bytes=stats["bytes"],
                           refused_frames=stats["refused"], off_over_hip=round(row["off"]["ms_median"] / row["hip"]["ms_median"], 2),
                           break_even_iterations=int(np.ceil(np.median(fills) / gain)) if gain > 0 else None)
                res.append(row)
    return dict(runs=res, workload="fit_dgp on the Reaching project: ResNet-50, 5 joints, batch_size 10, gm2 1, gm3 3, n_max_frames 150, "
                                   "832 x 747 frames from a LabeledDirSource (PNG decode per frame_at), PREFETCH_DEPTH %d; WARM %d iterations "
                                   "dropped" % (fitdgp.PREFETCH_DEPTH, WARM))


def event_ms(fn, calls):
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bench_kernel(H, W, nt=11, n_slots=48, calls=60):
    fb = H * W * 3
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randint(0, 256, (n_slots, slot_stride(fb)), dtype=torch.uint8, device=dev, generator=g)
    store = engine.FrameSlots(data, (H, W))
    out = torch.empty((nt, H, W, 3), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(0)
    tables = [rng.choice(n_slots, nt, replace=False) for _ in range(calls)]
    turn = [0]

    def gather():
        turn[0] += 1
        engine.gather_frames(store, tables[turn[0] % calls], out=out)

    def copies():
        turn[0] += 1
        for f, s in enumerate(tables[turn[0] % calls]):
            out[f].view(-1).copy_(data[int(s), :fb])

    copies()
    want = out.clone()
    turn[0] -= 1
    gather()
    assert torch.equal(out, want)
    ms = {"gather_frames": [], "d2d_copies": []}
    for _ in range(3):                                        # alternating blocks; the first block of each also warms up
        for name, fn in (("gather_frames", gather), ("d2d_copies", copies)):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ms[name].append(event_ms(fn, calls))
    res = dict(nt=nt, H=H, W=W, batch_MB=round(nt * fb / 1e6, 3), store_MB=round(data.numel() / 1e6, 1), calls_per_block=calls)
    for name, blocks in ms.items():
        allv = np.concatenate(blocks[1:])
        med = float(np.median(allv))
        res[name] = dict(ms_median=round(med, 4), ms_p10=round(float(np.percentile(allv, 10)), 4), ms_p90=round(float(np.percentile(allv, 90)), 4),
                         block_ms_median=[round(float(np.median(b)), 4) for b in blocks], GBps_read_plus_write=round(2 * nt * fb / med / 1e6, 1),
                         share_of_8TBps_peak=round(2 * nt * fb / med / 1e6 / HBM_PEAK_GBS, 3))
    res["gather_over_copies"] = round(res["gather_frames"]["ms_median"] / res["d2d_copies"]["ms_median"], 3)
    return res


out = {"metric": "frame_store", "device": torch.cuda.get_device_name(0)}
out["kernel"] = [bench_kernel(480, 640), bench_kernel(720, 1280)]
out["kernel_note"] = ("hipEvent spans around engine-level calls on the current stream (launch overheads included: one launch against nt "
                      "copies); the 10-30 MB batch and the store fit the 256 MB last-level cache, so GB/s is not an HBM rate")
if iters > 0:
    out["fit_dgp"] = bench_fit_dgp()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
