#!/usr/bin/env python3
"""The annotated movie of plot_dgp: markers drawn and frames turned into quantised DCT coefficients on the GPU (csrc/dgp_jpeg.hip),
Huffman-coded on host threads (csrc/dgp_jpeg_host.h), against the host writer (numpy overlay + one Pillow save per frame on one thread).
`bench_movie.py [frames] [--out FILE]` runs three legs on `frames` frames (default 4096) of 640x480 at quality 90, 4:2:0, with 4 markers of
dotsize 3 per frame, each leg in a fresh child process under its own time limit, stops at the first one that fails, and writes ONE JSON
line to profiles/movie_bench_line.json (or FILE) and to stdout:

  entropy   dgp_jpeg_entropy_encode frames/s on 1 host thread and on ENCODE_THREADS threads (no GPU)
  kernel    dgp_jpeg_forward_u8 alone on a batch of 32 frames with their markers: median of 100 hipEvent-timed calls after warm-up, as
            GB/s of RGB read plus coefficients written; the first frames' streams compared with Pillow's byte for byte
  movie     render.write_annotated_movie, backend "hip" and backend "host" alternating ROUNDS times in ONE process over the same frames
            (16 different frames in turn, from memory): median frames/s of each, and whether the two files are the same bytes

The baseline is "host": the only writer there was before (frames.write_mjpeg_avi).  No target is set: the line reports what came out.
Exit status: 0 when every leg ran and all bytes were equal, 1 when a leg failed, 2 when bytes differed.
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
HW, BATCH, QUALITY, SUBSAMPLING, ROUNDS, NJ, DOTSIZE = (480, 640), 32, 90, "4:2:0", 3, 4, 3
LEG_TIMEOUT_S = {"entropy": 240, "kernel": 180, "movie": 600}


def base_frames():
    from deepgraphpose_amd.synthetic import make_frames
    return make_frames(16, HW[0], HW[1], NJ, seed=0)


def labels(frames):
    import numpy as np
    rng = np.random.default_rng(0)
    x, y = rng.uniform(0, HW[1], (NJ, frames)), rng.uniform(0, HW[0], (NJ, frames))
    return x, y, rng.random((NJ, frames)) > 0.1


class Cycle:
    """`n` frames: the 16 base frames in turn (an open frame source, from memory)"""

    def __init__(self, base, n):
        self.base, self.n_frames, self.fps, self.size = base, n, 30.0, (base.shape[2], base.shape[1])

    def iter_frames(self):
        for i in range(self.n_frames):
            yield self.base[i % len(self.base)]


def leg_entropy(tmp, frames):
    import io
    import threading
    import numpy as np
    from PIL import Image
    from deepgraphpose_amd import jpeg
    from deepgraphpose_amd.models import render
    base = base_frames()
    sampling = jpeg.sampling_id(SUBSAMPLING)
    qt = jpeg.quality_tables(QUALITY)
    coefs, sizes = [], []
    for f in base:                              # Pillow's own coefficients of the frames: no GPU in this leg
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING)
        info = jpeg.probe(b.getvalue())
        c, q = np.empty(info.total_blocks * 64, np.int16), np.empty(info.ncomp * 64, np.uint16)
        jpeg.entropy_decode(b.getvalue(), info, c, q)
        coefs.append(c)
        sizes.append(len(b.getvalue()))
    bound = jpeg.encode_bound(HW[0], HW[1], sampling)

    def work(lo, hi):
        out = np.empty(bound, np.uint8)
        for i in range(lo, hi):
            jpeg.entropy_encode(coefs[i % 16], HW[0], HW[1], sampling, qt, out)

    work(0, 32)
    n1 = min(frames, 512)
    t0 = time.perf_counter()
    work(0, n1)
    one = n1 / (time.perf_counter() - t0)
    nt = int(render.ENCODE_THREADS)
    per = -(-frames // nt)
    ths = [threading.Thread(target=work, args=(t * per, min(frames, (t + 1) * per))) for t in range(nt)]
    t0 = time.perf_counter()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    many = frames / (time.perf_counter() - t0)
    return {"frames_per_s_1_thread": round(one, 1), "threads": nt, "frames_per_s_threads": round(many, 1), "scaling": round(many / one, 2),
            "jpeg_bytes_per_frame": int(sum(sizes) / len(sizes)), "cpus_available": len(os.sched_getaffinity(0))}


def leg_kernel(tmp, _frames):
    import io
    import numpy as np
    import torch
    from PIL import Image
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.models import render
    base = base_frames()
    host = np.stack([base[i % 16] for i in range(BATCH)])
    src = torch.from_numpy(host).cuda()
    x, y, mask = labels(BATCH)
    table = render.marker_table(x, y, mask, DOTSIZE)
    markers = torch.from_numpy(table).cuda()
    nblk, _ = engine.jpeg_block_count(HW[0], HW[1], engine.jpeg_sampling_id(SUBSAMPLING))
    out = torch.empty((BATCH, nblk, 64), dtype=torch.int16, device="cuda")
    fn = lambda: engine.jpeg_forward(src, QUALITY, SUBSAMPLING, markers, DOTSIZE, out=out)  # noqa: E731
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
    nbytes = src.numel() + out.numel() * 2 + markers.numel() * 4 + 256
    got = engine.jpeg_encode(src[:4], QUALITY, SUBSAMPLING, markers[:4], DOTSIZE)
    want = []
    for i in range(4):
        b = io.BytesIO()
        Image.fromarray(render.draw_markers_host(host[i], table[i], DOTSIZE)).save(b, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING)
        want.append(b.getvalue())
    return {"shape": "%d x %dx%d %s, %d markers" % (BATCH, HW[1], HW[0], SUBSAMPLING, NJ), "calls": len(ms), "ms_median": round(med, 4),
            "ms_p10": round(float(np.percentile(ms, 10)), 4), "ms_p90": round(float(np.percentile(ms, 90)), 4),
            "algorithmic_MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med / 1e6, 1), "hbm_peak_GB_per_s": 8000,
            "frac_hbm_peak": round(nbytes / med / 1e6 / 8000, 3), "frames_per_s": round(BATCH / med * 1e3, 0), "equals_pillow": got == want}


def leg_movie(tmp, frames):
    import numpy as np
    import torch
    from deepgraphpose_amd.models import render
    base = base_frames()
    x, y, mask = labels(frames)
    paths = {"hip": os.path.join(tmp, "hip.avi"), "host": os.path.join(tmp, "host.avi")}
    render.write_annotated_movie(Cycle(base, 64), x, y, mask, paths["hip"], DOTSIZE, QUALITY, SUBSAMPLING, "hip")      # warm-up
    fps = {"hip": [], "host": []}
    for _ in range(ROUNDS):
        for backend in ("hip", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render.write_annotated_movie(Cycle(base, frames), x, y, mask, paths[backend], DOTSIZE, QUALITY, SUBSAMPLING, backend)
            fps[backend].append(frames / (time.perf_counter() - t0))
    with open(paths["hip"], "rb") as a, open(paths["host"], "rb") as b:
        same = a.read() == b.read()
    return {"frames": frames, "batch": int(render.MOVIE_BATCH), "rounds": ROUNDS, "encode_threads": int(render.ENCODE_THREADS),
            "frames_per_s": {k: round(float(np.median(v)), 1) for k, v in fps.items()},
            "frames_per_s_all": {k: [round(q, 1) for q in v] for k, v in fps.items()}, "avi_MB": round(os.path.getsize(paths["hip"]) / 1e6, 1),
            "same_file": same}


def main():
    if "--leg" in sys.argv:
        leg = sys.argv[sys.argv.index("--leg") + 1]
        frames = int(sys.argv[sys.argv.index("--frames") + 1])
        tmp = sys.argv[sys.argv.index("--tmp") + 1]
        print(json.dumps({"entropy": leg_entropy, "kernel": leg_kernel, "movie": leg_movie}[leg](tmp, frames)), flush=True)
        return 0
    frames = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 4096
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "movie_bench_line.json")
    tmp = tempfile.mkdtemp()
    out = {"bench": "movie", "workload": "write_annotated_movie on %d frames of %dx%d (%d markers of dotsize %d per frame) to a Motion-JPEG .avi "
                                         "(quality %d, %s), frames from memory" % (frames, HW[1], HW[0], NJ, DOTSIZE, QUALITY, SUBSAMPLING),
           "baseline": "backend host: numpy overlay + one Pillow save per frame on one thread, the only writer there was before"}
    rc = 0
    try:
        for leg in ("entropy", "kernel", "movie"):
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(frames),
                   "--tmp", tmp]
            cp = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            if cp.returncode != 0 or not ln:
                out[leg] = {"error": "exit status %d: %s" % (cp.returncode, (cp.stderr or cp.stdout)[-600:])}
                rc = 1
                break                                            # nothing more is started on the GPU after a failure
            out[leg] = json.loads(ln[-1])
            print("[bench_movie] %s done" % leg, file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rc == 0:
        f = out["movie"]["frames_per_s"]
        out["hip_over_host"] = round(f["hip"] / f["host"], 2)
        out["hip_is_the_faster_writer"] = bool(f["hip"] > f["host"])
        if not (out["kernel"]["equals_pillow"] and out["movie"]["same_file"]):
            rc = 2
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
