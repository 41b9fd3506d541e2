#!/usr/bin/env python3
"""Frame selection (deepgraphpose_amd/frame_selection.py, csrc/dgp_select.hip).  `bench_select.py [frames]` writes `frames` frames (default
4096) of 640x480 as a Motion-JPEG .avi with frames.write_mjpeg_avi (quality 90, 4:2:0), then, in ONE process, measures and writes ONE JSON
line to profiles/select_bench_line.json (and to stdout):

  select    kmeans_select(numframes2pick=20) end to end with backend "hip", "host" and "sklearn", alternating ROUNDS times; the median
            seconds of each and of its stages (SELECT_STATS), and whether "hip" and "host" picked the same frames
  pass      the "hip" backend's read loop (frame_selection.device_frame_pass: Huffman decode on the host threads, reconstruction on the
            device) with engine.frame_features as its reducer and with engine.motion_energy in its place, alternating ROUNDS times: median
            frames/s of both.  THE BAR: features >= 0.9 x motion energy -- the thumbnails may not cost more than a second read of bytes
            that were decoded anyway
  kernels   dgp_frame_features_u8 and dgp_motion_energy alone on one batch of 256 decoded frames, and dgp_kmeans_assign / _update /
            _center alone at N = 4096, D = 690, k = 20: median of 100 hipEvent-timed calls after warm-up; GB/s of frame bytes read

Exit status: 0 when everything ran, the two backends agreed and the bar holds; 2 when the backends disagree; 3 when the bar is missed.
"""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HW, QUALITY, SUBSAMPLING, ROUNDS, PICK, BATCH = (480, 640), 90, "4:2:0", 3, 20, 256


def make_material(tmp, frames):
    """a clip with structure to cluster: 16 scenes, each drifting a pixel a frame"""
    import numpy as np
    from deepgraphpose_amd.frames import write_mjpeg_avi
    from deepgraphpose_amd.synthetic import make_frames
    base = make_frames(16, HW[0], HW[1], 4, seed=0)
    per = -(-frames // 16)
    avi = os.path.join(tmp, "clip.avi")
    write_mjpeg_avi(avi, (np.roll(base[i // per], i % per, axis=1) for i in range(frames)), fps=30.0, quality=QUALITY, subsampling=SUBSAMPLING)
    return avi


def timed(fn, calls=100, warm=10):
    import numpy as np
    import torch
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
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "calls": calls}


def main():
    import ctypes as C
    import numpy as np
    import torch
    from deepgraphpose_amd import _lib, engine
    from deepgraphpose_amd import frame_selection as F
    from deepgraphpose_amd.frames import open_frame_source
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
    tmp = tempfile.mkdtemp()
    out = {"bench": "select", "workload": "kmeans_select(numframes2pick=%d, resizewidth=30) over all %d frames of a %dx%d Motion-JPEG .avi "
                                          "(quality %d, %s)" % (PICK, frames, HW[1], HW[0], QUALITY, SUBSAMPLING), "rounds": ROUNDS}
    rc = 0
    try:
        src = open_frame_source(make_material(tmp, frames))
        print("[bench_select] material written", file=sys.stderr, flush=True)
        idx = np.arange(frames)
        # ---- select: the three backends, alternating
        backends = ["hip", "host"] + (["sklearn"] if _has_sklearn() else [])
        runs = {b: [] for b in backends}
        picks = {}
        for r in range(ROUNDS):
            for b in backends:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                picks[b] = F.kmeans_select(src, PICK, seed=0, backend=b)
                runs[b].append(dict(F.SELECT_STATS, wall_s=time.perf_counter() - t0))
                print("[bench_select] round %d %s %.2f s" % (r, b, runs[b][-1]["wall_s"]), file=sys.stderr, flush=True)
        med = lambda rows, key: round(float(np.median([q[key] for q in rows])), 3)  # noqa: E731
        out["select"] = {b: {"seconds": med(rows, "wall_s"), "frames_per_s": round(frames / med(rows, "wall_s"), 1),
                             "read_s": med(rows, "read_s"), "features_s": med(rows, "features_s"), "kmeans_s": med(rows, "kmeans_s"),
                             "iterations": int(rows[-1]["iterations"]), "picked": len(picks[b]),
                             "seconds_all": [round(q["wall_s"], 3) for q in rows]} for b, rows in runs.items()}
        out["hip_equals_host"] = picks["hip"] == picks["host"]
        out["hip_over_host"] = round(out["select"]["host"]["seconds"] / out["select"]["hip"]["seconds"], 2)
        if not out["hip_equals_host"]:
            rc = 2
        # ---- pass: decode + features against decode + motion energy, the same loop
        D = F.feature_geometry(HW[0], HW[1], 30)[-1]
        X = torch.empty((frames, D), dtype=torch.float32, device="cuda")
        reducers = {"features": lambda p0, fr: engine.frame_features(fr, 30, out=X[p0:p0 + fr.shape[0]]),
                    "motion_energy": lambda p0, fr: engine.motion_energy(fr)}
        fps = {name: [] for name in reducers}
        for r in range(ROUNDS):
            for name, fn in reducers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                F.device_frame_pass(src, idx, fn, BATCH)
                torch.cuda.synchronize()
                fps[name].append(frames / (time.perf_counter() - t0))
        f_feat, f_me = float(np.median(fps["features"])), float(np.median(fps["motion_energy"]))
        out["pass"] = {"chunk": BATCH, "decode_threads": int(F.DECODE_THREADS), "features_frames_per_s": round(f_feat, 1),
                       "motion_energy_frames_per_s": round(f_me, 1), "ratio": round(f_feat / f_me, 3), "bar": 0.9,
                       "bar_holds": bool(f_feat >= 0.9 * f_me), "frames_per_s_all": {k: [round(v, 1) for v in vs] for k, vs in fps.items()}}
        if not out["pass"]["bar_holds"]:
            rc = rc or 3
        # ---- kernels alone
        lib = _lib.load()
        got = []
        F.device_frame_pass(src, idx[:BATCH], lambda p0, fr: got.append(fr), BATCH)
        batch = got[0]
        nbytes = batch.numel()
        fb = nbytes // BATCH
        feat = torch.empty((BATCH, D), dtype=torch.float32, device="cuda")
        sums = torch.empty(BATCH, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        k_feat = timed(lambda: engine.frame_features(batch, 30, out=feat))
        k_me = timed(lambda: _lib.check(lib.dgp_motion_energy(ptr(batch), fb, BATCH, None, ptr(sums), stream)))
        for q in (k_feat, k_me):
            q["GB_per_s"] = round(nbytes / q["ms_median"] / 1e6, 1)
            q["frames_per_s"] = round(BATCH / q["ms_median"] * 1e3)
        same = bool(np.array_equal(feat[:8].cpu().numpy(), F.features_host(batch[:8].cpu().numpy(), 30)))
        N, Dk, k = 4096, 690, 20
        g = torch.Generator(device="cuda").manual_seed(0)
        Xk = torch.randn((N, Dk), device="cuda", generator=g) * 30
        Ck = Xk[:k].clone()
        labels = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        dist = torch.empty(N, dtype=torch.float32, device="cuda")
        counts = torch.empty(k + 1, dtype=torch.int32, device="cuda")
        engine.kmeans_assign(Xk, Ck, labels, dist)
        changed = torch.empty(1, dtype=torch.int32, device="cuda")
        scratch = torch.empty(int(lib.dgp_kmeans_scratch_bytes(N, Dk, k)) // 8 + 1, dtype=torch.float64, device="cuda")
        mean = torch.empty(Dk, dtype=torch.float32, device="cuda")
        k_assign = timed(lambda: _lib.check(lib.dgp_kmeans_assign(ptr(Xk), N, Dk, ptr(Ck), k, ptr(labels), ptr(dist), ptr(changed), stream)))
        k_update = timed(lambda: _lib.check(lib.dgp_kmeans_update(ptr(Xk), N, Dk, ptr(labels), ptr(Ck), k, ptr(counts), ptr(scratch),
                                                                  scratch.numel() * 8, stream)))
        k_center = timed(lambda: _lib.check(lib.dgp_kmeans_center(ptr(Xk), N, Dk, ptr(mean), ptr(scratch), scratch.numel() * 8, stream)))
        out["kernels"] = {"batch": "%d x %dx%d" % (BATCH, HW[1], HW[0]), "frame_MB": round(nbytes / 1e6, 1), "frame_features": k_feat,
                          "motion_energy": k_me, "features_over_motion_energy_GB_per_s": round(k_feat["GB_per_s"] / k_me["GB_per_s"], 3),
                          "hbm_peak_GB_per_s": 8000, "features_equal_host": same,
                          "kmeans": {"N": N, "D": Dk, "k": k, "assign": k_assign, "update": k_update, "center": k_center}}
        src.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "select_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


def _has_sklearn() -> bool:
    try:
        import sklearn  # noqa: F401
        return True
    except ImportError:
        return False


if __name__ == "__main__":
    sys.exit(main())
