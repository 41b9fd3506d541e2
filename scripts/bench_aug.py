#!/usr/bin/env python3
"""The augmentation of the DGP drivers' labeled frames on the device (fit_dgp(aug_backend="host" | "hip")) on one box, in alternation:

  fit_dgp   the real driver (ResNet-50, batch_size 10, gm2 = 1, gm3 = 3, frame_store="hip") on the golden Reaching project, aug on with
            aug_backend "host" and "hip" and aug off, alternating in one run, both tiers: the seconds between the returns of
            consecutive TrainSession.run calls after a warm-up, median and p10-p90
  stages    engine.augment_frames on one 747 x 832 frame with all seven stages forced, hipEvent-timed, and every stage's launch alone
            (engine.aug_*) beside the host stage (augment.apply_<stage>) under the same plan

`bench_aug.py [iters per block] [out.json]` -> one JSON line, also written to profiles/aug_bench_line.json.  Two blocks per column."""
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

from deepgraphpose_amd import augment, engine, weights_io
from deepgraphpose_amd.frames import LabeledDirSource
from deepgraphpose_amd.models import fitdgp, session
from deepgraphpose_amd.synthetic import make_weights

GOLDEN = os.path.join(ROOT, "tests", "golden")
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "aug_bench_line.json")
WARM = 6
COLUMNS = {"host": dict(aug=True, aug_backend="host"), "hip": dict(aug=True, aug_backend="hip"), "aug_off": dict(aug=False)}


def reaching_project(root):
    """The Reaching demo project from the files under tests/golden (as scripts/bench_frame_store.py assembles it), with a seeded start snapshot"""
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


def time_fit_dgp(proj, train, column, tier, n):
    """one fit_dgp run of WARM + n iterations -> (seconds between consecutive iterations after the warm-up, PREP_STATS["aug"])"""
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
                           n_max_frames=150, frame_sources=[source], frame_store="hip", **COLUMNS[column])
    finally:
        session.TrainSession.run = run
        os.environ.pop("DGP_TRAIN_TIER")
    assert len(stamps) == WARM + n, len(stamps)
    for f in os.listdir(train):
        if f.startswith("snapshot-step2") or f == "checkpoint":
            os.remove(os.path.join(train, f))
    return np.diff(stamps)[WARM - 1:], fitdgp.PREP_STATS["aug"]


def summary(values, scale=1e3):
    v = np.asarray(values, dtype=np.float64) * scale
    return dict(n=int(v.size), ms_median=round(float(np.median(v)), 4), ms_p10=round(float(np.percentile(v, 10)), 4),
                ms_p90=round(float(np.percentile(v, 90)), 4))


def bench_fit_dgp():
    os.environ["DGP_SNAPSHOT_FORMAT"] = "npz"
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        proj, train = reaching_project(tmp)
        for tier in ("parity", "f16"):
            dt, stats = {c: [] for c in COLUMNS}, {}
            for column in list(COLUMNS) * 2:
                d, stats[column] = time_fit_dgp(proj, train, column, tier, iters)
                dt[column].append(d)
            row = dict(tier=tier)
            for column, runs in dt.items():
                row[column] = dict(summary(np.concatenate(runs)), runs_ms_median=[round(float(np.median(r)) * 1e3, 3) for r in runs],
                                   aug=stats[column])
            row["host_over_hip"] = round(row["host"]["ms_median"] / row["hip"]["ms_median"], 2)
            row["hip_over_aug_off"] = round(row["hip"]["ms_median"] / row["aug_off"]["ms_median"], 2)
            res.append(row)
    return dict(runs=res, workload="fit_dgp on the Reaching project: ResNet-50, 5 joints, batch_size 10, gm2 1, gm3 3, n_max_frames 150, "
                                   "832 x 747 frames, frame_store hip, PREFETCH_DEPTH %d; %d iterations dropped per block"
                                   % (fitdgp.PREFETCH_DEPTH, WARM))


def event_ms(fn, calls=60, warm=5):
    for _ in range(warm):
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
    return ms


def host_ms(fn, calls=7):
    fn()
    s = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    return s


def bench_stages():
    from PIL import Image
    dev = torch.device("cuda", 0)
    name = sorted(os.listdir(os.path.join(GOLDEN, "reaching_frames")))[0]
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "reaching_frames", name)).convert("RGB")))
    H, W = img.shape[:2]

    def forced(noise):                           # every stage present; the same seed gives the same draws for both noise sources
        p = augment.NumpyAugPipeline(1.0, seed=7)
        plan = [(s, q) for s, q in p.plan(H, W, noise=noise) if s != "crop_and_pad"]
        plan[0] = ("fliplr", {"flip": True})
        return plan + [("crop_and_pad", {"amounts": augment.crop_amounts(-0.2, 0.05, -0.1, 0.08, H, W)})]

    plan_key, plan_field = forced("key"), forced("field")
    frames = torch.from_numpy(img[None].copy()).to(dev)
    pristine = frames.clone()
    src, dst = pristine[0], torch.empty_like(pristine[0])

    def whole():
        frames.copy_(pristine)
        engine.augment_frames(frames, [plan_key], [0])

    res = dict(H=H, W=W, frame_MB=round(img.nbytes / 1e6, 3),
               all_seven_with_reset_copy=summary(event_ms(whole), 1.0), reset_copy=summary(event_ms(lambda: frames.copy_(pristine)), 1.0),
               stages={})
    mask = torch.from_numpy(dict(plan_key)["coarse_dropout"]["mask"].astype(np.uint8)).to(dev)
    field = torch.from_numpy(dict(plan_key)["elastic"]["field"]).to(dev)
    launches = {
        "fliplr": lambda q: engine.aug_affine(src, dst, (-1.0, 0.0, float(W), 0.0, 1.0, 0.0)),
        "rotate": lambda q: engine.aug_affine(src, dst, q["coef"]),
        "motion_blur": lambda q: engine.aug_blur3(src, dst, q["kernel"]),
        "coarse_dropout": lambda q: engine.aug_dropout(src, dst, mask),
        "elastic": lambda q: engine.aug_elastic(src, dst, field),
        "gaussian_noise": lambda q: engine.aug_noise(src, dst, q["scale"], q["per_channel"], q["key"]),
        "crop_and_pad": lambda q: engine._aug_crop_and_pad(src, dst, q),
    }
    kp = np.zeros((0, 2))
    for (stage, q), (_, qf) in zip(plan_key, plan_field):
        res["stages"][stage] = dict(device=summary(event_ms(lambda: launches[stage](q)), 1.0),
                                    host=summary(host_ms(lambda: getattr(augment, "apply_" + stage)(img, kp, qf))))
    res["host_all_seven"] = summary(host_ms(lambda: augment.NumpyAugPipeline(1.0, seed=0).apply_host(plan_field, img, kp)))
    res["note"] = ("device: hipEvent spans around the engine-level call of one stage on the current stream, Python and launch overheads "
                   "included (crop_and_pad: the pad copy, the table upload and the resize launch); host: wall clock of apply_<stage>")
    return res


out = {"metric": "aug_backend", "device": torch.cuda.get_device_name(0)}
out["stages"] = bench_stages()
if iters > 0:
    out["fit_dgp"] = bench_fit_dgp()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
