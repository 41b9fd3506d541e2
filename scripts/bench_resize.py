#!/usr/bin/env python3
"""Resize + crop on the GPU (csrc/dgp_resize.hip, engine.resize_frames) and estimate_pose fed from it.  `bench_resize.py [frames]`
runs four legs, each in a fresh child process under its own time limit, stops at the first one that fails, and writes ONE JSON line to
profiles/resize_bench_line.json (and to stdout):

  kernel    dgp_resize_crop_u8 alone on 32 x 1280x720 -> 640x360: median of hipEvent-timed calls after warm-up, algorithmic bytes
            (source once + destination once), their share of the 8 TB/s HBM peak -- and, in the same process, the parity-tier DGPNet batch
            time at 640x360, i.e. the kernel's share of a step
  e2e_hip   estimate_pose(new_size=(360, 640), resize_backend="hip") on a `frames`-frame in-memory 1280x720 stack (default 4096), second
            call on the snapshot as scripts/bench_pipeline.py does
  e2e_pil   the same call with resize_backend="pil": the host Pillow path, which is the code every resized video ran before the kernel
            existed -- it stands for the previous state of the tree
  plain     estimate_pose on a 640x360 stack without new_size: what the pipeline sustains when nothing is resized

Exit status: 0 when every leg ran, the kernel's bytes equalled Pillow's and "hip" was not slower than "pil" (`hip_not_slower` in the line),
1 when a leg failed, 2 when one of those two conditions did not hold.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC_HW, NET_HW, BATCH = (720, 1280), (360, 640), 32
LEG_TIMEOUT_S = {"kernel": 180, "e2e_hip": 300, "e2e_pil": 420, "plain": 240}


def leg_kernel(_frames):
    import numpy as np
    import torch
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    base = make_frames(BATCH, SRC_HW[0], SRC_HW[1], 4, seed=0)
    src = torch.from_numpy(base).cuda()
    dst = torch.empty((BATCH,) + NET_HW + (3,), dtype=torch.uint8, device="cuda")

    def timed(fn, calls):
        for _ in range(10):
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

    ms = timed(lambda: engine.resize_frames(src, new_size=NET_HW, out=dst), 200)
    med = float(np.median(ms))
    nbytes = src.numel() + dst.numel()
    # byte-exactness of this very shape against Pillow, on the first frames (the tests cover the small shapes)
    from PIL import Image
    want = np.stack([np.asarray(Image.fromarray(f).resize(size=(NET_HW[1], NET_HW[0]))) for f in base[:2]])
    exact = bool(np.array_equal(dst[:2].cpu().numpy(), want))
    net = engine.DGPNet(50, 4, NET_HW[0], NET_HW[1], max_batch=BATCH)
    net.load_weights(make_weights(50, 4, False, seed=0, head_std=0.05))
    traj = torch.zeros((BATCH, 4, 5), dtype=torch.float32, device="cuda")
    net_ms = float(np.median(timed(lambda: net.infer_packed(dst, traj), 30)))
    return {"shape": "%d x %dx%d -> %dx%d" % (BATCH, SRC_HW[1], SRC_HW[0], NET_HW[1], NET_HW[0]), "calls": len(ms),
            "ms_median": round(med, 4), "ms_p10": round(float(np.percentile(ms, 10)), 4), "ms_p90": round(float(np.percentile(ms, 90)), 4),
            "algorithmic_MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med / 1e6, 1), "hbm_peak_GB_per_s": 8000,
            "frac_hbm_peak": round(nbytes / med / 1e6 / 8000, 3), "equals_pillow": exact,
            "dgpnet_parity_batch_ms_at_640x360": round(net_ms, 3), "share_of_a_parity_step": round(med / net_ms, 4)}


def leg_e2e(frames, backend):
    import tempfile
    import numpy as np
    import torch
    import yaml
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.models import eval as E
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    tmp = tempfile.mkdtemp()
    proj = os.path.join(tmp, "proj")
    train = os.path.join(proj, "dlc-models", "iteration-0", "DemoOct2-trainset95shuffle1", "train")
    os.makedirs(train)
    parts = ["a", "b", "c", "d"]
    with open(os.path.join(proj, "config.yaml"), "w") as f:
        yaml.safe_dump(dict(Task="Demo", date="Oct2", iteration=0, TrainingFraction=[0.95], bodyparts=parts, skeleton=[], project_path=proj), f)
    with open(os.path.join(train, "pose_cfg.yaml"), "w") as f:
        yaml.safe_dump(dict(num_joints=4, all_joints_names=parts, net_type="resnet_50"), f)
    snap = weights_io.save_weights(os.path.join(train, "snapshot-step2-final--0"), make_weights(50, 4, False, seed=0, head_std=0.05))
    hw = NET_HW if backend == "plain" else SRC_HW
    stack = np.concatenate([make_frames(16, hw[0], hw[1], 4, seed=0)] * (frames // 16))
    kw = {} if backend == "plain" else dict(new_size=NET_HW, resize_backend=backend)
    cfg = os.path.join(proj, "config.yaml")
    E.estimate_pose(cfg, snap, stack[:64], os.path.join(tmp, "warm"), save_pose=False, batch_size=BATCH, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = E.estimate_pose(cfg, snap, stack, os.path.join(tmp, "pred"), save_pose=False, batch_size=BATCH, **kw)
    dt = time.perf_counter() - t0
    return {"frames_per_s": round(len(stack) / dt, 1), "frames": int(len(stack)), "seconds": round(dt, 3), "batch": BATCH,
            "source": "%dx%d" % (hw[1], hw[0]), "prep_backend": E.RUN_STATS["prep_backend"],
            "host_seconds": {k: round(float(v), 3) for k, v in E.RUN_STATS.items() if k.endswith("_s")},
            "mean_x": round(float(out["x"].mean()), 4)}


def main():
    if "--leg" in sys.argv:
        leg = sys.argv[sys.argv.index("--leg") + 1]
        frames = int(sys.argv[sys.argv.index("--frames") + 1])
        res = leg_kernel(frames) if leg == "kernel" else leg_e2e(frames, {"e2e_hip": "hip", "e2e_pil": "pil", "plain": "plain"}[leg])
        print(json.dumps(res), flush=True)
        return 0
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
    out = {"bench": "resize", "workload": "estimate_pose(new_size=(360, 640)) on a host stack of %d 1280x720x3 u8 frames (ResNet-50, 4 keypoints, "
                                          "parity tier, batch %d), PCIe-inclusive, second call on the snapshot" % (frames, BATCH),
           "baseline": "e2e_pil is the host Pillow path, unchanged: the code every resized video ran before the kernel existed"}
    rc = 0
    for leg in ("kernel", "e2e_hip", "e2e_pil", "plain"):
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames)]
        cp = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
        if cp.returncode != 0 or not ln:
            out[leg] = {"error": "exit status %d: %s" % (cp.returncode, (cp.stderr or cp.stdout)[-400:])}
            rc = 1
            break                                            # nothing more is started on the GPU after a failure
        out[leg] = json.loads(ln[-1])
    if rc == 0:
        out["hip_over_pil"] = round(out["e2e_hip"]["frames_per_s"] / out["e2e_pil"]["frames_per_s"], 2)
        out["hip_over_plain"] = round(out["e2e_hip"]["frames_per_s"] / out["plain"]["frames_per_s"], 3)
        # the one condition this bench sets: the kernel's bytes are Pillow's and "hip" is not slower than "pil".  The exit status says so.
        out["hip_not_slower"] = bool(out["e2e_hip"]["frames_per_s"] >= out["e2e_pil"]["frames_per_s"])
        if not (out["hip_not_slower"] and out["kernel"]["equals_pillow"]):
            rc = 2
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resize_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
