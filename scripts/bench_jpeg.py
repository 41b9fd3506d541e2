#!/usr/bin/env python3
"""JPEG decode for estimate_pose: entropy decode on the host (csrc/dgp_jpeg_host.h), reconstruction on the GPU (csrc/dgp_jpeg.hip).
`bench_jpeg.py [frames]` makes its material once -- `frames` frames (default 4096) of 640x480 written by frames.write_mjpeg_avi at quality
90, 4:2:0, and the same JPEG streams as a directory of .jpg files --, then runs three legs, each in a fresh child process under its own time
limit, stops at the first one that fails, and writes ONE JSON line to profiles/jpeg_bench_line.json (and to stdout):

  entropy   dgp_jpeg_probe + dgp_jpeg_entropy_decode frames/s on 1 host thread and on DECODE_THREADS threads (no GPU)
  kernel    dgp_jpeg_reconstruct_u8 alone on a batch of 32 frames: median of 100 hipEvent-timed calls after warm-up, as GB/s of
            coefficients and tables read plus RGB written; the first frames compared with Pillow byte for byte
  e2e       estimate_pose, parity tier, batch 32, ROUNDS times round-robin in ONE process over four feeds: decode_backend "hip" on the
            AVI; "host" on the AVI (frame_at = Pillow); "host" on the directory (the only way these frames could be read before this
            decoder existed); the in-memory stack of the decoded frames (the ceiling: nothing is decoded).  Median frames/s per feed.

No target is set: the line reports what came out.  Exit status: 0 when every leg ran and the kernel's bytes equalled Pillow's, 1 when a
leg failed, 2 when the bytes differed.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HW, BATCH, QUALITY, SUBSAMPLING, ROUNDS = (480, 640), 32, 90, "4:2:0", 3
LEG_TIMEOUT_S = {"entropy": 240, "kernel": 180, "e2e": 900}


def make_material(tmp, frames):
    import numpy as np
    from deepgraphpose_amd.frames import MjpegAviSource, write_mjpeg_avi
    from deepgraphpose_amd.synthetic import make_frames
    base = make_frames(16, HW[0], HW[1], 4, seed=0)
    avi = os.path.join(tmp, "clip.avi")
    write_mjpeg_avi(avi, (base[i % 16] for i in range(frames)), fps=30.0, quality=QUALITY, subsampling=SUBSAMPLING)
    src = MjpegAviSource(avi)
    d = os.path.join(tmp, "jpegs")
    os.makedirs(d)
    for i in range(frames):
        with open(os.path.join(d, "f%05d.jpg" % i), "wb") as f:
            f.write(src.jpeg_bytes(i))
    np.save(os.path.join(tmp, "decoded16.npy"), np.stack([src.frame_at(i) for i in range(16)]))
    nbytes = os.path.getsize(avi)
    src.close()
    return {"frames": frames, "avi_MB": round(nbytes / 1e6, 1), "jpeg_bytes_per_frame": int(nbytes / frames),
            "npy_stack_MB": round(frames * HW[0] * HW[1] * 3 / 1e6, 1)}


def leg_entropy(tmp, frames):
    import threading
    import numpy as np
    from deepgraphpose_amd import jpeg
    from deepgraphpose_amd.frames import MjpegAviSource
    from deepgraphpose_amd.models import eval as E
    src = MjpegAviSource(os.path.join(tmp, "clip.avi"))
    streams = [src.jpeg_bytes(i) for i in range(frames)]
    info0 = jpeg.probe(streams[0])

    def work(lo, hi):
        coef = np.empty(info0.total_blocks * 64, np.int16)
        qt = np.empty(info0.ncomp * 64, np.uint16)
        for i in range(lo, hi):
            jpeg.entropy_decode(streams[i], jpeg.probe(streams[i]), coef, qt)

    work(0, 32)
    n1 = min(frames, 512)
    t0 = time.perf_counter()
    work(0, n1)
    one = n1 / (time.perf_counter() - t0)
    nt = int(E.DECODE_THREADS)
    per = -(-frames // nt)
    ths = [threading.Thread(target=work, args=(t * per, min(frames, (t + 1) * per))) for t in range(nt)]
    t0 = time.perf_counter()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    many = frames / (time.perf_counter() - t0)
    return {"frames_per_s_1_thread": round(one, 1), "threads": nt, "frames_per_s_threads": round(many, 1),
            "scaling": round(many / one, 2), "cpus_available": len(os.sched_getaffinity(0))}


def leg_kernel(tmp, _frames):
    import numpy as np
    import torch
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.frames import MjpegAviSource
    src = MjpegAviSource(os.path.join(tmp, "clip.avi"))
    streams = [src.jpeg_bytes(i) for i in range(BATCH)]
    info = engine.jpeg_probe(streams[0])
    coef = np.empty((BATCH, info.total_blocks, 64), np.int16)
    qt = np.empty((BATCH, info.ncomp, 64), np.uint16)
    for i, b in enumerate(streams):
        engine.jpeg_entropy_decode(b, engine.jpeg_probe(b), coef[i], qt[i])
    dcoef, dqt = torch.from_numpy(coef).cuda(), torch.from_numpy(qt.view(np.int16)).cuda()
    dst = torch.empty((BATCH,) + HW + (3,), dtype=torch.uint8, device="cuda")
    fn = lambda: engine.jpeg_reconstruct(dcoef, dqt, HW[0], HW[1], info.sampling, out=dst)  # noqa: E731
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(100):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    nbytes = dcoef.numel() * 2 + dqt.numel() * 2 + dst.numel()
    exact = bool(np.array_equal(dst[:4].cpu().numpy(), np.stack([src.frame_at(i) for i in range(4)])))
    return {"shape": "%d x %dx%d %s" % (BATCH, HW[1], HW[0], SUBSAMPLING), "calls": len(ms), "ms_median": round(med, 4),
            "ms_p10": round(float(np.percentile(ms, 10)), 4), "ms_p90": round(float(np.percentile(ms, 90)), 4),
            "algorithmic_MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med / 1e6, 1), "hbm_peak_GB_per_s": 8000,
            "frac_hbm_peak": round(nbytes / med / 1e6 / 8000, 3), "frames_per_s": round(BATCH / med * 1e3, 0), "equals_pillow": exact}


def leg_e2e(tmp, frames):
    import numpy as np
    import torch
    import yaml
    from deepgraphpose_amd import weights_io
    from deepgraphpose_amd.models import eval as E
    from deepgraphpose_amd.synthetic import make_weights
    proj = os.path.join(tmp, "proj")
    train = os.path.join(proj, "dlc-models", "iteration-0", "DemoOct2-trainset95shuffle1", "train")
    os.makedirs(train)
    parts = ["a", "b", "c", "d"]
    with open(os.path.join(proj, "config.yaml"), "w") as f:
        yaml.safe_dump(dict(Task="Demo", date="Oct2", iteration=0, TrainingFraction=[0.95], bodyparts=parts, skeleton=[], project_path=proj), f)
    with open(os.path.join(train, "pose_cfg.yaml"), "w") as f:
        yaml.safe_dump(dict(num_joints=4, all_joints_names=parts, net_type="resnet_50"), f)
    snap = weights_io.save_weights(os.path.join(train, "snapshot-step2-final--0"), make_weights(50, 4, False, seed=0, head_std=0.05))
    cfg = os.path.join(proj, "config.yaml")
    stack = np.concatenate([np.load(os.path.join(tmp, "decoded16.npy"))] * (frames // 16))[:frames]
    avi, jdir = os.path.join(tmp, "clip.avi"), os.path.join(tmp, "jpegs")
    feeds = [("hip_avi", avi, "hip"), ("host_avi", avi, "host"), ("host_dir", jdir, "host"), ("npy_stack", stack, "host")]
    E.estimate_pose(cfg, snap, stack[:64], os.path.join(tmp, "warm"), save_pose=False, batch_size=BATCH)
    fps = {name: [] for name, _, _ in feeds}
    mean_x, stats = {}, {}
    for r in range(ROUNDS):
        for name, video, backend in feeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = E.estimate_pose(cfg, snap, video, os.path.join(tmp, "pred_%s_%d" % (name, r)), save_pose=False, batch_size=BATCH,
                                  decode_backend=backend)
            fps[name].append(frames / (time.perf_counter() - t0))
            assert E.RUN_STATS["decode_backend"] == backend
            mean_x[name] = round(float(out["x"].mean()), 4)
            stats[name] = {k: round(float(v), 3) for k, v in E.RUN_STATS.items() if k.endswith("_s")}
    return {"frames": frames, "batch": BATCH, "rounds": ROUNDS, "decode_threads": int(E.DECODE_THREADS),
            "frames_per_s": {k: round(float(np.median(v)), 1) for k, v in fps.items()},
            "frames_per_s_all": {k: [round(x, 1) for x in v] for k, v in fps.items()}, "host_seconds_last_round": stats,
            "same_labels": len(set(mean_x.values())) == 1, "mean_x": mean_x}


def main():
    if "--leg" in sys.argv:
        leg = sys.argv[sys.argv.index("--leg") + 1]
        frames = int(sys.argv[sys.argv.index("--frames") + 1])
        tmp = sys.argv[sys.argv.index("--tmp") + 1]
        print(json.dumps({"entropy": leg_entropy, "kernel": leg_kernel, "e2e": leg_e2e}[leg](tmp, frames)), flush=True)
        return 0
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
    tmp = tempfile.mkdtemp()
    out = {"bench": "jpeg", "workload": "estimate_pose on %d frames of %dx%d (ResNet-50, 4 keypoints, parity tier, batch %d) from a Motion-JPEG "
                                        ".avi (quality %d, %s), the same JPEGs as a directory, and the decoded stack; second call on the snapshot"
                                        % (frames, HW[1], HW[0], BATCH, QUALITY, SUBSAMPLING),
           "baseline": "host_dir is the only way these frames could be read before: ImageDirSource, one Pillow decode per frame on one thread"}
    rc = 0
    try:
        out["material"] = make_material(tmp, frames)
        for leg in ("entropy", "kernel", "e2e"):
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames),
                   "--tmp", tmp]
            cp = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            if cp.returncode != 0 or not ln:
                out[leg] = {"error": "exit status %d: %s" % (cp.returncode, (cp.stderr or cp.stdout)[-600:])}
                rc = 1
                break                                            # nothing more is started on the GPU after a failure
            out[leg] = json.loads(ln[-1])
            print("[bench_jpeg] %s done" % leg, file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rc == 0:
        f = out["e2e"]["frames_per_s"]
        out["hip_over_host_dir"] = round(f["hip_avi"] / f["host_dir"], 2)
        out["hip_over_host_avi"] = round(f["hip_avi"] / f["host_avi"], 2)
        out["hip_over_npy_stack"] = round(f["hip_avi"] / f["npy_stack"], 3)
        out["hip_faster_than_host_dir"] = bool(f["hip_avi"] > f["host_dir"])
        if not out["kernel"]["equals_pillow"]:
            rc = 2
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jpeg_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
