#!/usr/bin/env python3
"""bench.py -- frames/s of the DGP hot path on MI355X (BASELINE.json metric).

Workload (config.workload): BASELINE configs[1] -- ResNet-50, 640x480x3 uint8 frames,
4 keypoints, batch 32 per GPU, inference (backbone + part_pred head + DGP soft-argmax +
likelihood), synthetic device-resident frames, seeded random-init weights.
A "step" = one batch of 32 frames through dgp_infer on each GPU.  With N > 1 every rank
processes its own contiguous frame shard and ONE RCCL all-gather (inside the timed region)
reassembles the [T, nj] trajectory: weak scaling.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...            # no launcher: spawns its own N worker processes (one per GPU, RCCL over 127.0.0.1)
    python bench.py --gpus N --scaling strong --total-batches 1024   # ONE fixed stream of 32768 frames split over the N ranks
    python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR  # + the last timed step's mu / conf / idx as DIR/<name>.npy
    python bench.py --gpus 1 --steps K --warmup W --full              # + everything that is not the headline figure (below)

Rank 0 prints ONE JSON line.  A plain run sets up, pre-warms, runs the W warm-up and K timed steps and
prints the line: `value` / `ms_per_step` and the "roofline" object (conv kernel, MFMA-bound, fp32 matrix
peak) from hipEvent pairs recorded around every launch inside the timed region.  `--full` adds what
takes runs of its own: the "sustained" segment, "cpu_baseline" with "accuracy_vs_oracle" (the CPU
oracle = fp32 torch-CPU restatement of the TF1 reference path, timed on the host cores on a bounded
sample; TF1 itself cannot be installed here) and, at N = 1, the child-process legs (strict_f32, tier_f16,
r101_1280x720(_f16), train_step(_f16), host_pipeline(_f16)).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense fp32 matrix
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 matrix peak (v_mfma_f32_32x32x16_bf16)
PEAK_HBM_TBPS = 8.0               # MI355X_MICROARCH.md: HBM3E spec peak (6.3 TB/s measured for a plain copy)


def kernel_peak(kernel: str) -> float:
    """Matrix-pipe ceiling of a conv kernel in fp32-equivalent TFLOP/s: the split kernels issue 6 (or 3) bf16 MFMAs
    per fp32-equivalent product, so their ceiling is the dense bf16 peak / 6 (/ 3)."""
    if kernel.startswith("h1_"):            # 16-bit tier: one fp16 MFMA per product -> the dense 16-bit peak itself
        return PEAK_BF16_MFMA_TFLOPS
    if kernel.startswith("split6"):
        return PEAK_BF16_MFMA_TFLOPS / 6.0
    if kernel.startswith(("split3", "splith3", "stem_pool_fused", "chain_", "unit_")):     # fp16 dense peak = bf16 dense peak
        return PEAK_BF16_MFMA_TFLOPS / 3.0
    return PEAK_F32_MFMA_TFLOPS
H, W, NJ, BATCH = 480, 640, 4, 32
STRIDE = 8.0


def mfma_only_sustained():
    """(TFLOP/s, source): what a loop of NOTHING BUT v_mfma_f32_16x16x32_f16 sustains on this part under its power cap -- read from the
    committed measurement (profiles/r*_mfma_power.txt, newest round first; one box, tagged as such in the line), 1788 when no file is there"""
    import glob, re
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_mfma_power.txt")), reverse=True):
        try:
            vals = [float(m.group(1)) for m in re.finditer(r"v_mfma_f32_16x16x32_f16: (\d+(?:\.\d+)?) TFLOP/s sustained", open(path).read())]
        except OSError:
            vals = []
        if vals:
            return max(vals), "profiles/%s (one MI355X box of the pool, 1400 W board cap)" % os.path.basename(path)
    return 1788.0, "round-5 measurement (profiles file missing)"


def newest_traffic_files(suffix=""):
    """profiles/traffic_r<N><suffix>.json, newest round first"""
    import glob, re
    c = []
    for q in glob.glob(os.path.join(ROOT, "profiles", "traffic_r*%s.json" % suffix)):
        m = re.fullmatch(r"traffic_r(\d+)%s\.json" % re.escape(suffix), os.path.basename(q))
        if m:
            c.append((int(m.group(1)), q))
    return [q for _, q in sorted(c, reverse=True)]


def roofline_from_launches(launches, B, elem_bytes, traffic_files):
    """The `roofline` object of a bench line from the per-launch table of the instrumented steps (dgp_net_profile_launch): the dominant conv
    kernel against its matrix-pipe ceiling, every conv kernel against both roofs.  elem_bytes: 4 for the parity tier's H2 cells, 2 for the
    16-bit tier's H1 cells (arch.launch_algorithmic_bytes); traffic_files: candidate profiles/traffic_*.json, first existing one wins."""
    from deepgraphpose_amd.arch import conv_macs_per_frame
    flop_frame = 2.0 * conv_macs_per_frame(H, W, 50, NJ, False)
    conv = [(n, f, ms) for (n, f, ms) in launches if n.startswith("conv:")]
    conv_ms = sum(ms for _, _, ms in conv)
    conv_flops = sum(f for _, f, _ in conv)
    other_ms = sum(ms for n, _, ms in launches if not n.startswith("conv:"))
    stack_tf = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    from deepgraphpose_amd.arch import launch_algorithmic_bytes
    alg_bytes = {n: launch_algorithmic_bytes(n, H, W, 50, B, elem_bytes) for n, _, _ in conv}      # per launch name (fused launches: external tensors only)
    # per-kernel breakdown (the engine tags every conv launch with the kernel it ran); the roofline object is for
    # the DOMINANT kernel = the one with the largest share of the step
    by_kernel = {}
    for n, f, ms in conv:
        k = n.split("|")[1] if "|" in n else "f32"
        e = by_kernel.setdefault(k, [0, 0.0, 0.0, 0.0])
        e[0] += 1; e[1] += f; e[2] += ms; e[3] += alg_bytes.get(n, 0.0)
    dom = max(by_kernel, key=lambda k: by_kernel[k][2])
    d_n, d_f, d_ms, _ = by_kernel[dom]
    achieved = d_f / (d_ms * 1e-3) / 1e12 if d_ms > 0 else 0.0
    peak = kernel_peak(dom)
    n_mfma = "6" if dom.startswith("split6") else "1" if dom.startswith("h1_") else "3"
    mfma_kind = "f16" if dom.startswith(("splith", "h1_")) else "bf16"
    kname = {"f32": "conv_igemm_f32 / conv_igemm_f32_ls (v_mfma_f32_32x32x2_f32)"}.get(
        dom, ("conv_igemm_split_ls<%s, H1> (fp16 operands from 2-byte H1 cells, ONE v_mfma_f32_16x16x32_f16 per product)" % dom) if dom.startswith("h1_")
        else "conv_igemm_split_ls<%s> (fp32-class products as %s v_mfma_f32_16x16x32_%s)" % (dom, n_mfma, mfma_kind))
    roofline = {
        "bound": "mfma", "kernel": "%s, %d of the %d conv launches of a step" % (kname, d_n, len(conv)),
        "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4), "traffic": None,
        "peak_basis": ("dense %s MFMA peak %.0f TFLOP/s / %s partial products per fp32-class product; achieved counts "
                       "ALGORITHMIC conv FLOPs" % (mfma_kind, PEAK_BF16_MFMA_TFLOPS, n_mfma)) if dom.startswith("split")
                      else ("dense f16 MFMA peak %.0f TFLOP/s, ONE v_mfma_f32_16x16x32_f16 per product; achieved counts ALGORITHMIC conv FLOPs"
                            % PEAK_BF16_MFMA_TFLOPS) if dom.startswith("h1_")
                      else "dense fp32 MFMA peak %.1f TFLOP/s" % PEAK_F32_MFMA_TFLOPS,
        "kernel_ms_per_step": round(d_ms, 3),
        # every conv kernel against BOTH roofs: matrix pipe (algorithmic FLOPs) and HBM (algorithmic bytes of its launches: tensors
        # that enter or leave a launch once + weights; the chain / unit kernels keep X' / R2 on chip, so their bytes are fewer)
        "kernels": {k: {"launches": v[0], "ms_per_step": round(v[2], 3), "tflops": round(v[1] / (v[2] * 1e-3) / 1e12, 1),
                        "frac_of_its_peak": round(v[1] / (v[2] * 1e-3) / 1e12 / kernel_peak(k), 4),
                        "algorithmic_gb_per_step": round(v[3] / 1e9, 3),
                        "hbm_tbps_algorithmic": round(v[3] / (v[2] * 1e-3) / 1e12, 2),
                        "frac_of_hbm_peak": round(v[3] / (v[2] * 1e-3) / 1e12 / PEAK_HBM_TBPS, 4),
                        "bound": "hbm" if v[3] / (v[2] * 1e-3) / 1e12 / PEAK_HBM_TBPS > v[1] / (v[2] * 1e-3) / 1e12 / kernel_peak(k) else "mfma"}
                    for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][2])},
        "conv_stack_algorithmic_gb_per_step": round(sum(alg_bytes.values()) / 1e9, 3),
        "conv_stack_tflops": round(stack_tf, 2),
        "conv_stack_vs_fp32_mfma_peak": round(stack_tf / PEAK_F32_MFMA_TFLOPS, 4),
        "algorithmic_gflop_per_frame": round(flop_frame / 1e9, 3),
        "conv_ms_per_step": round(conv_ms, 3), "other_kernels_ms_per_step": round(other_ms, 3),
        "conv_ms_note": ("sum of the hipEvent-timed conv launches of the INSTRUMENTED steps, which run alone on ONE stream; the timed steps of "
                         "`ms_per_step` are dealt to two engines on two streams (tails of one batch's launches fill with the other's), so "
                         "ms_per_step can be smaller than this sum"),
    }
    # HBM traffic of the dominant kernel, per launch, from the committed rocprofv3 PMC passes of this same command
    # (scripts/profile.sh -> profiles/traffic_r1.json: FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE, separate
    # passes); null when no profile of this kernel has been taken.
    tj = next((q for q in traffic_files if os.path.exists(q)), "")
    if os.path.exists(tj):
        try:
            tr = json.load(open(tj))
            if dom.startswith("h1_"):
                cands = [v for k_, v in tr.get("per_kernel", {}).items() if k_.startswith("conv_igemm_split_ls<128,128,") and v.get("h1")]
                nl_ = sum(v["launches_per_step"] for v in cands)
                if cands and nl_ > 0:
                    roofline["traffic"] = float(sum(v["hbm_bytes_per_launch"] * v["launches_per_step"] for v in cands) / nl_)
                    roofline["traffic_unit"] = ("bytes per launch of the dominant kernel (launch-weighted mean of its loader specialisations), PMC "
                                                "FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE at the L2's memory side")
                    roofline["algorithmic_bytes_per_launch"] = round(by_kernel[dom][3] / d_n, 1)
            elif dom.startswith("split"):
                pk = dom.replace("splith3", "2").replace("split", "").split("_")      # NT, "128x128", "k16[w8]"
                bk, cw = (pk[2][1:].split("w") + ["4"])[:2]
                key = "conv_igemm_split_ls<%s,%s,%s,%s,%s" % (pk[1].split("x")[0], pk[1].split("x")[1], pk[0], bk, cw)
                cands = [v for k_, v in tr.get("per_kernel", {}).items() if k_.startswith(key)]       # (+ ",true": pre-split weights)
                nl_ = sum(v["launches_per_step"] for v in cands)
                if cands and nl_ > 0:      # launch-weighted mean over the kernel's loader specialisations (pointwise / 3x3 walk)
                    roofline["traffic"] = float(sum(v["hbm_bytes_per_launch"] * v["launches_per_step"] for v in cands) / nl_)
                    roofline["traffic_unit"] = ("bytes per launch of the dominant kernel (launch-weighted mean of its loader specialisations), PMC "
                                                "FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE at the L2's memory side: Infinity-Cache hits and "
                                                "the weights fetched once per XCD are included")
                    roofline["algorithmic_bytes_per_launch"] = round(by_kernel[dom][3] / d_n, 1)
            roofline["conv_stack_hbm_bytes_per_step"] = float(tr["conv_hbm_bytes_per_step"])
            roofline["traffic_source"] = "profiles/%s (rocprofv3 --pmc passes of this command, NOT measured in this run)" % os.path.basename(tj)
        except Exception:
            pass
    return roofline, by_kernel




def _read_sclk_mhz(card_index: int = 0):
    """Current shader clock of THIS process's GPU from sysfs (the line marked '*' in pp_dpm_sclk of the card whose PCI address matches
    torch's device `card_index`; a box exposes every card of the node in sysfs), or None when unreadable."""
    import glob
    want = None
    try:
        pr = torch.cuda.get_device_properties(card_index)
        want = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
    except Exception:
        pass
    paths = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
    if want is not None:
        matched = [q for q in paths if want in os.path.realpath(os.path.dirname(q)).lower()]
        paths = matched or paths
    for path in paths:
        try:
            for line in open(path).read().splitlines():
                if line.strip().endswith("*"):
                    return int("".join(ch for ch in line.split(":")[1] if ch.isdigit()))
        except (OSError, ValueError, IndexError):
            continue
    return None


def visible_gpu_count() -> int:
    """GPUs this process may use, WITHOUT touching HIP: KFD topology nodes with SIMDs (CPU nodes report simd_count 0), cut down by
    HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES when one of them is set.  -1 entries end a list, as in the runtime."""
    import glob
    n = 0
    for q in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            props = dict(l.split(None, 1) for l in open(q).read().splitlines() if " " in l)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
        except (OSError, ValueError):
            continue
    if n == 0:                                   # (no KFD topology in this container's sysfs: the render nodes, one per GPU)
        n = len(glob.glob("/dev/dri/renderD*"))
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            ids = []
            for t in v.split(","):
                t = t.strip()
                if t in ("", "-1"):
                    break
                ids.append(t)
            n = min(n, len(ids)) if n else len(ids)
    return n


def spawn_workers(args) -> None:
    """`python bench.py --gpus N` without a launcher: start N worker processes (one per GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in
    their environment, exactly what torch.distributed.run would set), relay rank 0's JSON line and exit with the workers' worst return
    code.  This parent never initialises the GPU -- the visible devices are counted from the KFD topology in sysfs, not through HIP or
    torch.cuda -- and never exec()s."""
    import socket
    import subprocess
    n = max(1, args.gpus)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    have = visible_gpu_count()
    if 0 < have < n and not os.environ.get("DGP_BENCH_VISIBLE_GPUS"):      # (have == 0: nothing to count here -- the workers' own device binding decides)
        raise SystemExit("bench.py: --gpus %d but only %d device(s) visible (set DGP_BENCH_VISIBLE_GPUS to share devices knowingly)" % (n, have))
    visible = int(os.environ.get("DGP_BENCH_VISIBLE_GPUS", n))      # tests: several ranks on one GPU (with DGP_DIST_BACKEND=gloo)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r % max(1, visible)), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), DGP_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # rank 0's stdout is drained by a thread; this loop polls EVERY child: the first one that exits non-zero (OOM, RCCL init failure, bad
    # LOCAL_RANK) takes the others down with it instead of leaving rank 0 inside a collective until a watchdog fires (or for ever),
    # and an overall deadline bounds the run.  Children are terminated / killed by PID, never re-exec'd.
    import threading
    buf = []
    rd = threading.Thread(target=lambda: buf.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    deadline = time.monotonic() + float(os.environ.get("DGP_BENCH_TIMEOUT", 3600))
    failed = None
    while True:
        rcs = [q.poll() for q in procs]
        if all(c is not None for c in rcs):
            break
        bad = [i for i, c in enumerate(rcs) if c not in (None, 0)]
        if bad or time.monotonic() > deadline:
            failed = "rank %d exited with code %d" % (bad[0], rcs[bad[0]]) if bad else "timeout"
            for q in procs:
                if q.poll() is None:
                    q.terminate()
            t_end = time.monotonic() + 10.0
            for q in procs:
                try:
                    q.wait(timeout=max(0.1, t_end - time.monotonic()))
                except subprocess.TimeoutExpired:
                    q.kill()
                    q.wait()
            rcs = [q.returncode for q in procs]
            break
        time.sleep(0.05)
    rd.join(timeout=5.0)
    out0 = buf[0] if buf else ""
    if failed:
        print("bench.py: %s; the other workers were stopped" % failed, file=sys.stderr, flush=True)
        first_bad = next((c for c in rcs if c not in (0, None) and c > 0), 1)
        raise SystemExit(first_bad)
    line = None
    for ln in (out0 or "").splitlines():
        if ln.startswith("{"):
            line = ln
        else:
            print(ln, flush=True)
    if line is not None:
        try:
            d = json.loads(line)
            d["launcher"] = "bench.py spawned %d worker process(es) itself (no torch.distributed.run)" % n
            line = json.dumps(d)
        except ValueError:
            pass
        print(line, flush=True)
    rc = max(abs(c) for c in rcs)
    if rc or line is None:
        raise SystemExit(rc or 1)


def strict_f32_child(args) -> None:
    """Fresh process started by the N = 1 run with DGP_CONV_MODE=f32 in its environment: the same workload on the fp32 MFMA kernels
    (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain; fp32 activations), a few steps, one small JSON line."""
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.arch import conv_macs_per_frame
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    mode = os.environ.get("DGP_CONV_MODE")
    assert mode == "f32"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, K = args.batch, max(3, min(args.steps, 10))
    wts = make_weights(50, NJ, False, seed=0, head_std=0.05)
    net = engine.DGPNet(50, NJ, H, W, max_batch=B, device=0)
    net.load_weights(wts)
    base = make_frames(8, H, W, NJ, seed=100)
    g = torch.Generator().manual_seed(1234)
    sel = torch.randint(0, base.shape[0], (B,), generator=g).numpy()
    noise = torch.randint(-3, 4, (B, H, W, 3), generator=g, dtype=torch.int16).numpy()
    fr = torch.from_numpy(np.clip(base[sel].astype(np.int16) + noise, 0, 255).astype(np.uint8)).to(dev)      # = ring[0] of the main run
    out = torch.zeros((B, NJ, 5), dtype=torch.float32, device=dev)
    for _ in range(3):
        net.infer_packed(fr, out, 1.0, 1)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(K):
        net.infer_packed(fr, out, 1.0, 1)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    fps = K * B / (t1 - t0)
    res = {"frames_per_s": round(fps, 1), "steps": K, "ms_per_step": round((t1 - t0) / K * 1e3, 3)}
    tf = fps * 2.0 * conv_macs_per_frame(H, W, 50, NJ, False) / 1e12
    if mode == "f32":
        res["frac_of_fp32_mfma_peak"] = round(tf / PEAK_F32_MFMA_TFLOPS, 4)
        res["kernels"] = "conv_igemm_f32 / conv_igemm_f32_ls (DGP_CONV_MODE=f32: IEEE fp32 products and activations)"
    if not args.no_cpu_baseline:
        from oracle import dgp_oracle as O      # checker only
        ncmp = 4
        ref = O.infer(fr[:ncmp].cpu().numpy(), wts, 50, STRIDE, 1.0, 1)
        m, c, ix = net.infer(fr[:ncmp].contiguous(), 1.0, 1)
        m = m.cpu().numpy().astype(np.float64)
        ex = m[:, :, 1] * STRIDE + 0.5 * STRIDE - ref["x"][:ncmp]
        ey = m[:, :, 0] * STRIDE + 0.5 * STRIDE - ref["y"][:ncmp]
        res["px_max"] = float(np.sqrt(ex ** 2 + ey ** 2).max())
        res["idx_bit_exact"] = bool(np.array_equal(ix.cpu().numpy(), ref["idx"][:ncmp]))
    print(json.dumps(res), flush=True)


def tier_f16_child(args) -> None:
    """Fresh process started by the N = 1 run: the SAME workload on the 16-bit tier (dgp_net_set_tier(net, 1): 2-byte H1 activation cells from
    the pool output to the block4 features, fp16 weight cells, one MFMA per product; fp32 accumulation, epilogues, heads and soft-argmax).
    Protocol of the main run in small: calibration on ring[0], untimed pre-warm, 3 instrumented steps alone on one stream (per-launch
    hipEvents -> its own roofline object), K timed steps dealt to two engines on two HIP streams; then its error against the CPU oracle over
    256 frames (8 batches): px RMSE / max, index-agreement rate, likelihood difference.  A REPORTED tier, never `value`."""
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, K = args.batch, max(8, args.steps)
    wts = make_weights(50, NJ, False, seed=0, head_std=0.05)
    NS = max(1, args.streams)                       # (--streams 1: the rocprofv3 passes of scripts/profile.sh, every launch alone on the chip)
    pipe = engine.DGPPipeline(50, NJ, H, W, max_batch=B, device=0, n_streams=NS, tier="f16")
    pipe.load_weights(wts)
    net = pipe.nets[0]
    assert all(n.tier == "f16" for n in pipe.nets)
    NB = 8                                          # ring[0..3] are the main run's batches (same seeds); 4 more for the 256-frame error figures
    base = make_frames(8, H, W, NJ, seed=100)
    g = torch.Generator().manual_seed(1234)
    ring = []
    for r in range(NB):
        sel = torch.randint(0, base.shape[0], (B,), generator=g).numpy()
        noise = torch.randint(-3, 4, (B, H, W, 3), generator=g, dtype=torch.int16).numpy()
        ring.append(torch.from_numpy(np.clip(base[sel].astype(np.int16) + noise, 0, 255).astype(np.uint8)).to(dev))
    traj = torch.zeros((NB * B, NJ, 5), dtype=torch.float32, device=dev)
    scr = [torch.zeros((B, NJ, 5), dtype=torch.float32, device=dev) for _ in range(2)]
    pipe.calibrate(ring[0])
    p0 = time.perf_counter()
    while time.perf_counter() - p0 < (1.0 if NS > 1 else 0.1):
        for i in range(8):
            pipe.submit(ring[i % NB], scr[i & 1], 1.0, 1)
        pipe.join()
        torch.cuda.synchronize(dev)
    net.profile_begin(3)
    for i in range(3):
        net.infer_packed(ring[i % NB], scr[0], 1.0, 1)
    torch.cuda.synchronize(dev)
    n_prof, launches = net.profile_end()
    t0 = time.perf_counter()
    for i in range(K):
        net.infer_packed(ring[i % NB], scr[0], 1.0, 1)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    for i in range(K):
        pipe.submit(ring[i % NB], scr[i & 1], 1.0, 1)
    pipe.join()
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    sclk = _read_sclk_mhz(0)
    for i in range(NB):                             # the trajectory the error figures are taken from: two batches in flight, like the timed steps
        pipe.submit(ring[i], traj[i * B:(i + 1) * B], 1.0, 1)
    pipe.join()
    torch.cuda.synchronize(dev)
    ov, _ = pipe.range_status()
    assert not ov, "activation ranges outgrew the calibrated scales during the 16-bit tier's run"
    roofline, by_kernel = roofline_from_launches(launches, B, 2.0, newest_traffic_files("_f16"))
    roofline["steps_profiled"] = n_prof
    sus, sus_src = mfma_only_sustained()               # (a pure fp16 MFMA loop under the board's power cap)
    roofline["mfma_only_sustained_peak"] = sus
    roofline["mfma_only_source"] = sus_src
    roofline["frac_of_mfma_only_sustained"] = round(roofline["achieved"] / sus, 4)
    fps2, fps1 = K * B / (t2 - t1), K * B / (t1 - t0)
    # the WHOLE step against the roof (stem, heads, soft-argmax, epilogues and launch gaps included), not only the dominant kernel
    roofline["frac_whole_step"] = round(fps2 * roofline["algorithmic_gflop_per_frame"] / 1e3 / roofline["peak"], 4)
    roofline["frac_whole_step_one_stream"] = round(fps1 * roofline["algorithmic_gflop_per_frame"] / 1e3 / roofline["peak"], 4)
    res = {"frames_per_s": round(fps2, 1), "ms_per_step": round((t2 - t1) / K * 1e3, 3), "steps": K, "streams": NS,
           "one_stream": {"frames_per_s": round(fps1, 1), "ms_per_step": round((t1 - t0) / K * 1e3, 3)},
           "dtype": "f16", "sclk_mhz_under_load": sclk,
           "dtype_note": ("2-byte activations end to end (H1 cells = NHWC fp16 with calibrated per-tensor power-of-two scales), fp16 weight cells, ONE "
                          "v_mfma_f32_16x16x32_f16 per product; fp32 accumulation, BN / residual / ReLU epilogues, heads and soft-argmax in fp32; the "
                          "root block as in the parity tier.  11-bit operands: outside the 1e-3 px gate, reported beside `value`, never as it"),
           "activation_format": "H1 (16-byte cells of 8 halves; include/dgp_hip.h, dgp_net_set_tier)",
           "roofline": roofline}
    if not args.no_cpu_baseline:
        from oracle import dgp_oracle as O      # checker only
        torch.set_num_threads(max(1, min(args.cpu_threads, os.cpu_count() or 1)))
        rec = traj.cpu().numpy()
        errs, agree, likd, n_idx = [], 0, 0.0, 0
        for i in range(NB):
            ref = O.infer(ring[i].cpu().numpy(), wts, 50, STRIDE, 1.0, 1)
            r = rec[i * B:(i + 1) * B]
            ex = r[:, :, 1].astype(np.float64) * STRIDE + 0.5 * STRIDE - ref["x"]
            ey = r[:, :, 0].astype(np.float64) * STRIDE + 0.5 * STRIDE - ref["y"]
            errs.append(np.sqrt(ex ** 2 + ey ** 2))
            ix = np.ascontiguousarray(r[:, :, 3:5]).view(np.int32)
            agree += int((ix == ref["idx"]).all(-1).sum()); n_idx += ix.shape[0] * ix.shape[1]
            likd = max(likd, float(np.abs(r[:, :, 2] - ref["likelihoods"]).max()))
        err = np.concatenate(errs)
        res["accuracy_vs_oracle"] = {"frames": int(err.shape[0]), "px_rmse": float(np.sqrt((err ** 2).mean())), "px_max": float(err.max()),
                                     "px_p99": float(np.quantile(err, 0.99)), "idx_agreement_rate": agree / n_idx,
                                     "likelihood_max_abs_diff": likd,
                                     "what": "the packed trajectory of %d batches (two in flight) vs the fp32 CPU oracle on the same frames" % NB}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)      # (0.44 s of timed region at 6.9 ms per step; round 2 timed 20 steps = 0.15 s)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the sustained segment, the CPU baseline and oracle check, and (N = 1) the "
                         "child-process legs; the options below that shape those parts act only with --full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=64, help="size of the bounded CPU-baseline sample (batch-1 leg: a quarter of it)")
    ap.add_argument("--cpu-threads", type=int, default=16,
                    help="torch CPU threads for the baseline (16 was the fastest of 8..128 on the GPU box)")
    ap.add_argument("--layer-table", type=str, default="", help="write the per-launch table (tsv) here")
    ap.add_argument("--profile-steps", type=int, default=3, help="timed steps instrumented with per-launch hipEvents (roofline)")
    ap.add_argument("--prewarm-seconds", type=float, default=1.5, help="untimed load before the warm-up steps (clock ramp, calibration)")
    ap.add_argument("--sustain-seconds", type=float, default=5.0, help="length of the sustained segment after the timed region")
    ap.add_argument("--streams", type=int, default=2, help="engines / HIP streams the batches are dealt to (1: single stream)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --steps batches per GPU; strong: --total-batches batches in all, rank r runs its contiguous share")
    ap.add_argument("--total-batches", type=int, default=1024, help="strong scaling: batches of the one fixed stream (1024 x 32 = 32768 frames)")
    ap.add_argument("--no-strict-f32", action="store_true", help="skip the child-process legs after the timed region: DGP_CONV_MODE=f32 (IEEE fp32 MFMA tier), the 16-bit tier, ResNet-101 1280x720, the training step and the PCIe-inclusive estimate_pose run")
    ap.add_argument("--no-host-pipeline", action="store_true", help="skip the PCIe-inclusive estimate_pose child run")
    ap.add_argument("--host-frames", type=int, default=4096, help="host frames of the PCIe-inclusive estimate_pose child run (a multiple of 16)")
    ap.add_argument("--no-r101", action="store_true", help="skip the ResNet-101 1280x720 child run (BASELINE configs[4] per-GPU shape)")
    ap.add_argument("--no-train-step", action="store_true", help="skip the training-step child run (BASELINE configs[3]) after the timed region")
    ap.add_argument("--train-steps", type=int, default=60, help="timed steps of the training-step child run")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="rank 0 writes what the last timed step computed (mu, conf, idx of its batch) as DIR/<name>.npy")
    ap.add_argument("--strict-f32-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tier-f16-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.strict_f32_child:
        return strict_f32_child(args)
    if args.tier_f16_child:
        return tier_f16_child(args)
    # No launcher around us and more than one GPU asked for (or DGP_BENCH_FORCE_SPAWN=1): this process only spawns the workers -- it never
    # touches the GPU -- and relays rank 0's line.
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or os.environ.get("DGP_BENCH_FORCE_SPAWN") == "1"):
        return spawn_workers(args)

    from deepgraphpose_amd import dist as ddist
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.arch import conv_macs_per_frame
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    import torch.distributed as dist

    if os.environ.get("DGP_BENCH_FAULT_RANK") == os.environ.get("RANK", "0"):      # tests: a worker that dies before it joins the group
        raise SystemExit(7)
    # one GPU per rank: refuse to put several ranks on one device by accident (a line measured that way is not an N-GPU line);
    # DGP_BENCH_VISIBLE_GPUS=<n> is the explicit opt-in the one-GPU tests use (with DGP_DIST_BACKEND=gloo).  device_count() does not
    # initialise the GPU on this image
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus and not os.environ.get("DGP_BENCH_VISIBLE_GPUS"):
        raise SystemExit("bench.py: --gpus %d but only %d device(s) visible (set DGP_BENCH_VISIBLE_GPUS to share devices knowingly)" % (args.gpus, n_dev))
    rank, local_rank, world = ddist.init_from_env("nccl")
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N>1 with torch.distributed.run)"
                         % (args.gpus, world))
    if os.environ.get("DGP_BENCH_VISIBLE_GPUS") and n_dev > 0 and local_rank >= n_dev:
        # ranks knowingly sharing devices under a launcher that numbers LOCAL_RANK 0..N-1 (torch.distributed.run on a box with fewer GPUs:
        # the one-GPU test of the driver's exact command line, control plane on gloo)
        local_rank %= n_dev
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    numa = ddist.bind_to_gpu_numa_node(local_rank)      # before any helper thread exists: they inherit the mask
    ident = dict(ddist.device_identity(local_rank), rank=rank, **numa)

    B, K, Wm = args.batch, args.steps, args.warmup
    if K < 1 and args.scaling == "weak":
        raise SystemExit("bench.py: --steps must be at least 1")
    if args.scaling == "strong":      # one fixed stream, independent of N: rank r runs batches [r TB / N, (r + 1) TB / N)
        if args.total_batches % world:
            raise SystemExit("bench.py: --total-batches %d must be a multiple of --gpus %d" % (args.total_batches, world))
        K = args.total_batches // world
    wts = make_weights(50, NJ, False, seed=0, head_std=0.05)
    # two engines on two HIP streams, batches dealt in turn (engine.DGPPipeline): the grid tail of one batch's layers runs under the
    # other batch's kernels.  --streams 1 is the plain single-stream loop
    pipe = engine.DGPPipeline(50, NJ, H, W, max_batch=B, device=local_rank, n_streams=max(1, args.streams))
    pipe.load_weights(wts)
    net = pipe.nets[0]

    # ONE seeded synthetic stream for the whole job: global batch g holds frames [g B, (g + 1) B) of the stream and
    # is ring[g % RING] -- a device-resident ring of RING distinct batches, identical on every rank (seed 100), so that the
    # inputs defeat cache residency but the stream is defined independently of N.  The stream has N K batches; rank r owns the
    # contiguous block shard_range(N K B, r, N) = batches [r K, (r + 1) K): weak scaling, no data-path collective but the ONE
    # all-gather of the packed keypoints at the end (inside the timed region).
    RING = 4
    base = make_frames(8, H, W, NJ, seed=100)
    g = torch.Generator().manual_seed(1234)
    ring = []
    for r in range(RING):
        sel = torch.randint(0, base.shape[0], (B,), generator=g).numpy()
        noise = torch.randint(-3, 4, (B, H, W, 3), generator=g, dtype=torch.int16).numpy()
        fr = np.clip(base[sel].astype(np.int16) + noise, 0, 255).astype(np.uint8)
        ring.append(torch.from_numpy(fr).to(dev))
    n_local = K * B
    lo, hi = ddist.shard_range(world * n_local, rank, world)
    assert (lo, hi) == (rank * n_local, (rank + 1) * n_local)
    g0 = lo // B                                   # first global batch of this rank
    traj = torch.zeros((n_local, NJ, 5), dtype=torch.float32, device=dev)
    scratch = torch.zeros((B, NJ, 5), dtype=torch.float32, device=dev)

    scratches = [scratch] + [torch.zeros_like(scratch) for _ in range(len(pipe.nets) - 1)]

    def step(i, record=True, sequential=False):
        # the soft-argmax kernel writes the packed (row, col, likelihood, iy, ix) records straight into the trajectory slice
        out = traj[i * B:(i + 1) * B] if record else scratches[pipe._next if not sequential else 0]
        if sequential:       # on the caller's stream, engine 0: the steps instrumented with per-launch events
            net.infer_packed(ring[(g0 + i) % RING], out, 1.0, 1)
        else:
            pipe.submit(ring[(g0 + i) % RING], out, 1.0, 1)

    use_pg = dist.is_initialized()

    def barrier():
        if use_pg:
            if dist.get_backend() == "nccl":
                dist.barrier(device_ids=[local_rank])
            else:                                   # DGP_DIST_BACKEND=gloo: several ranks on one GPU (tests/test_boundary_gpu.py)
                dist.barrier()

    # untimed pre-warm (declared in the output): the first forward calibrates the engine's activation scales (layer-by-layer, with
    # syncs) and the GPU needs ~1 s of load to leave its idle clock state; then the W warm-up steps the contract asks for
    # (every rank calibrates on the SAME batch, ring[0], so that the frozen scales -- and with them every output bit -- do not depend
    #  on which shard a rank owns)
    pipe.calibrate(ring[0])
    torch.cuda.synchronize(dev)
    p0 = time.perf_counter()
    while time.perf_counter() - p0 < args.prewarm_seconds:
        for i in range(8):
            step(i % max(K, 1), record=False)
        torch.cuda.synchronize(dev)
    for i in range(Wm):
        step(i % max(K, 1), record=False)
    pipe.join()
    if use_pg:      # warm the collective too
        ddist.gather_trajectory(traj, world * n_local)
    torch.cuda.synchronize(dev)

    # hipEvent pairs around every launch of the FIRST `prof_steps` steps of the timed region (106 event records per step cost ~4 % of a
    # step; the remaining steps run uninstrumented).  Per-kernel durations -> the roofline object.
    prof_steps = min(K, args.profile_steps)
    if prof_steps > 1 and prof_steps * 10 > K:     # short runs: at most a tenth of the timed steps carries the instrumentation
        prof_steps = max(1, K // 10)
    net.profile_begin(max(prof_steps, 1))
    barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(K):
        step(i, sequential=i < prof_steps)      # instrumented steps run alone (per-launch durations are not shared with a second batch)
    pipe.join()
    torch.cuda.synchronize(dev)                         # (this rank's frames are done: what follows is the collective alone)
    tg0 = time.perf_counter()
    full = ddist.gather_trajectory(traj, world * n_local)
    torch.cuda.synchronize(dev)
    tg1 = time.perf_counter()
    barrier()
    t1 = time.perf_counter()
    n_prof, launches = net.profile_end()
    dumped = None
    if args.dump_outputs and rank == 0:
        # the last timed step's batch as a caller of the packed path receives it (dist.unpack_keypoints): soft-argmax coordinates, likelihoods,
        # arg-max indices; the inputs are seeded, so two builds can be compared output for output
        mu, conf, idx = ddist.unpack_keypoints(traj[(K - 1) * B:K * B])
        os.makedirs(args.dump_outputs, exist_ok=True)
        dumped = {"mu": mu.cpu().numpy().astype(np.float32), "conf": conf.cpu().numpy().astype(np.float32),
                  "idx": idx.cpu().numpy().astype(np.float64)}
        for name, a in dumped.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
        dumped = {"dir": args.dump_outputs, "step": K - 1, "arrays": {name: list(a.shape) for name, a in dumped.items()}}

    # sustained segment (--full; untimed for `value`): >= 5 s of back-to-back steps so that clocks, power and the driver's SMI sampler
    # see a loaded GPU; reports the rate and the shader clock sysfs shows while it runs
    sustained = None
    if args.full and (rank == 0 or use_pg):
        s_steps, s0 = 0, time.perf_counter()
        sclk = None
        while True:
            for _ in range(16):
                step(s_steps % max(K, 1), record=False)
                s_steps += 1
            if sclk is None and s_steps >= 64:
                sclk = _read_sclk_mhz(local_rank)
            pipe.join()
            torch.cuda.synchronize(dev)
            if time.perf_counter() - s0 >= args.sustain_seconds:
                break
        s1 = time.perf_counter()
        sustained = {"frames_per_s_per_gpu": round(s_steps * B / (s1 - s0), 1), "seconds": round(s1 - s0, 2), "steps": s_steps,
                     "sclk_mhz_under_load": sclk}
        barrier()

    range_overflow, n_calib = pipe.range_status()         # a forward that outgrew the calibrated activation scales would be invalid
    assert not range_overflow or os.environ.get("DGP_BENCH_ALLOW_OVERFLOW") == "1", \
        "activation ranges outgrew the calibrated scales during the run"      # (the override: timing-only ablation builds, scripts/ablate_unit.sh)
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    elapsed_min = elapsed.clone()
    if use_pg:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
        dist.all_reduce(elapsed_min, op=dist.ReduceOp.MIN)
    elapsed, elapsed_min = float(elapsed.item()), float(elapsed_min.item())
    assert full.shape[0] == world * n_local
    # what RCCL saw, rank by rank, so that an N > 1 line can be verified by its reader: backend and world size as torch.distributed reports
    # them, every rank's device (index, PCI address, uuid, NUMA node, CPUs it was bound to), its own frames/s, and the one collective
    mine = dict(ident, frames_per_s=round(n_local / (t1 - t0), 2), elapsed_s=round(t1 - t0, 6), all_gather_ms=round((tg1 - tg0) * 1e3, 4))
    per_rank = [mine]
    if use_pg:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    collective = {"backend": dist.get_backend() if use_pg else None, "world_size": dist.get_world_size() if use_pg else 1,
                  "initialized": bool(use_pg), "op": "all_gather_into_tensor of the packed keypoints, once per run, inside the timed region",
                  "all_gather_bytes": int(world * (-(-world * n_local // world)) * NJ * 5 * 4),
                  "all_gather_ms": {"rank0": round((tg1 - tg0) * 1e3, 4), "max": max(q["all_gather_ms"] for q in per_rank)},
                  "distinct_devices": len({(q["pci"], q["uuid"]) for q in per_rank}), "ranks": per_rank}
    # every rank ran the same ring: global batch g must reproduce batch g % RING (its first occurrence: rank 0's when K >= RING) bit for bit --
    # the gathered N-rank trajectory equals what one rank computes for the same frames
    shard_check = None
    if world * K > RING:
        fb = full.view(world * K, B, NJ, 5)
        same = all(torch.equal(fb[gb], fb[gb % RING]) for gb in range(RING, world * K))
        same_idx = all(torch.equal(fb[gb][..., 3:], fb[gb % RING][..., 3:]) for gb in range(RING, world * K))
        max_d = max(float((fb[gb][..., :3] - fb[gb % RING][..., :3]).abs().max()) for gb in range(RING, world * K))
        shard_check = {"batches_compared": world * K - RING, "bit_identical_to_rank0": bool(same), "indices_identical": bool(same_idx),
                       "max_abs_diff_row_col_lik": max_d}
        assert (same_idx and max_d < 1e-3 / 8.0) or os.environ.get("DGP_BENCH_ALLOW_OVERFLOW") == "1", "sharded trajectory differs from the single-rank result"

    if rank != 0:
        if use_pg:
            dist.destroy_process_group()
        return

    fps = world * n_local / elapsed
    roofline, by_kernel = roofline_from_launches(launches, B, 4.0, newest_traffic_files(""))
    roofline["steps_profiled"] = n_prof
    # the WHOLE step against the roof (stem, heads, soft-argmax, epilogues and launch gaps included), not only the dominant kernel
    roofline["frac_whole_step"] = round(fps / world * roofline["algorithmic_gflop_per_frame"] / 1e3 / roofline["peak"], 4)
    if args.layer_table:
        os.makedirs(os.path.dirname(os.path.abspath(args.layer_table)), exist_ok=True)
        with open(args.layer_table, "w") as f:
            f.write("launch\tname\tgflop\tavg_ms\ttflops\n")
            for i, (n, fl, ms) in enumerate(launches):
                f.write("%d\t%s\t%.3f\t%.4f\t%.2f\n" % (i, n, fl / 1e9, ms, fl / (ms * 1e-3) / 1e12 if ms > 0 else 0))

    # informative only: what a loop of NOTHING BUT MFMAs sustains on this part under its 1400 W power cap (scripts/micro/mfma_power.hip,
    # profiles/r5_mfma_power.txt: 1.79 PFLOP/s of dense fp16 = 0.71 of the rating, at the cap) -- the ceiling of a kernel that moves no data at all
    sus, sus_src = mfma_only_sustained()
    roofline["mfma_only_sustained_peak"] = round(sus / 3.0, 1)
    roofline["mfma_only_source"] = sus_src
    roofline["frac_of_mfma_only_sustained"] = round(roofline["achieved"] / (sus / 3.0), 4)
    roofline["mfma_only_note"] = ("a pure v_mfma_f32_16x16x32_f16 loop sustains 1788 TFLOP/s at 1350 W of the 1400 W board cap (profiles/r5_mfma_power.txt); the bench "
                                  "workload itself runs at 1347 W with the clock throttled to ~1.96 GHz (profiles/r5_power_probe.txt): `frac` stays against the rated peak")
    if sustained and sustained.get("sclk_mhz_under_load"):
        # informative only: the chip is power-limited under this load, so the matrix pipe never sees its 2400 MHz rating
        mhz = float(sustained["sclk_mhz_under_load"])
        if 500.0 <= mhz <= 2400.0:
            roofline["peak_at_sustained_clock"] = round(roofline["peak"] * mhz / 2400.0, 1)
            roofline["frac_at_sustained_clock"] = round(roofline["achieved"] / (roofline["peak"] * mhz / 2400.0), 4)
            roofline["sustained_clock_note"] = ("sclk %d MHz read from sysfs during the sustained segment (rated 2400): `frac` stays "
                                                "against the rated peak" % int(mhz))
    out = {
        "metric": "frames_per_sec", "value": round(fps, 2), "unit": "frames/s", "n_gpus": world,
        "steps": K, "warmup": Wm, "ms_per_step": round(elapsed / K * 1e3, 3), "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "dtype_note": ("fp32-class arithmetic: fp32 accumulation, every operand carries 22 significant bits as an fp16 high/low pair (products as "
                       "3 MFMAs on the 16-bit matrix pipe); activations live in HBM in that form (H2 cells, same bytes as fp32, scaled by a "
                       "calibrated power of two per tensor), weights are pre-split at load; error vs fp64 <= the fp32-MFMA kernels' "
                       "(scripts/split_sweep.py); DGP_H2=0 / DGP_CONV_MODE=f32|bf16x6 select the other paths")
                      if any(k.startswith("split") for k in by_kernel) else "fp32 MFMA (bitwise fmaf chains)",
        "config": {"workload": "ResNet-50 640x480x3 u8, 4 keypoints, batch %d/GPU, inference "
                               "(scoremap + DGP soft-argmax + likelihood), BASELINE configs[1]" % B,
                   "frames_per_step_per_gpu": B, "sharding": "contiguous frame shards, 1 RCCL all-gather per run",
                   "total_frames": world * n_local},
        "roofline": roofline,
        "full": bool(args.full),          # plain run: no sustained segment, CPU baseline or child legs in this line
        "sustained": sustained,
        "shard_check": shard_check,
        "prewarm_seconds": args.prewarm_seconds,
        "streams": {"n": len(pipe.nets), "note": "batches are dealt in turn to n engines on n HIP streams (engine.DGPPipeline); the "
                    "`steps_profiled` instrumented steps run alone on one stream, the other timed steps overlap pairwise"},
        "range_overflow": bool(range_overflow),
        # DGP_BENCH_ALLOW_OVERFLOW=1 (timing-only ablation builds) switches the range-overflow and sharded-trajectory asserts off: such a line
        # says so and carries no headline number
        "asserts_bypassed": os.environ.get("DGP_BENCH_ALLOW_OVERFLOW") == "1",
        # imbalance between the ranks: `value` divides by the slowest rank's time (both include the barriers and the all-gather)
        "rank_elapsed_s": {"max": round(elapsed, 6), "min": round(elapsed_min, 6), "imbalance": round(elapsed / max(elapsed_min, 1e-12) - 1.0, 4)},
        "frames_per_s": round(fps, 2),
        "collective": collective,
        "activation_format": "H2 (fp16 high/low cells, calibrated per-tensor scales; include/dgp_hip.h)" if n_calib else "fp32",
    }
    if dumped:
        out["dump_outputs"] = dumped

    if args.full and not args.no_cpu_baseline and world == 1:      # rank 0 at N = 1 only
        from oracle import dgp_oracle as O      # checker / baseline only
        nthreads = max(1, min(args.cpu_threads, os.cpu_count() or 1))
        torch.set_num_threads(nthreads)
        O.infer(ring[0][:1].cpu().numpy(), wts, 50, STRIDE, 1.0, 1)             # warm-up
        # the reference's own operating point: batch 1, one session call per frame (eval.py:179,328)
        n1 = max(4, args.cpu_frames // 4)
        f1 = ring[1][:n1].cpu().numpy()
        c0 = time.perf_counter()
        for i in range(n1):
            O.infer(f1[i:i + 1], wts, 50, STRIDE, 1.0, 1)
        c1 = time.perf_counter()
        # batch 32 (the GPU step's batch), one call
        f32 = ring[0].cpu().numpy()
        c2 = time.perf_counter()
        ref = O.infer(f32, wts, 50, STRIDE, 1.0, 1)
        c3 = time.perf_counter()
        fps1, fps32 = n1 / (c1 - c0), f32.shape[0] / (c3 - c2)
        # checked: the trajectory the TIMED REGION wrote -- global batch 0 = ring[0] is traj[0:B] (an instrumented step, alone on one
        # stream), global batch RING = ring[0] again is traj[RING B:(RING + 1) B] (dealt to the two engines, two batches in flight) --
        # all B frames of each against the oracle on the same frames (records: row, col, likelihood fp32 + (iy, ix) int32 bit patterns)
        def _timed_vs_oracle(first):
            rec = traj[first:first + B].cpu().numpy()
            ex_ = rec[:, :, 1].astype(np.float64) * STRIDE + 0.5 * STRIDE - ref["x"]
            ey_ = rec[:, :, 0].astype(np.float64) * STRIDE + 0.5 * STRIDE - ref["y"]
            ix_ = np.ascontiguousarray(rec[:, :, 3:5]).view(np.int32)
            return np.sqrt(ex_ ** 2 + ey_ ** 2), bool(np.array_equal(ix_, ref["idx"])), float(np.abs(rec[:, :, 2] - ref["likelihoods"]).max())
        assert g0 == 0
        err, idx_ok, lik_d = _timed_vs_oracle(0)
        checked = ["timed step 0 (one stream)"]
        if K > RING:
            err2, idx_ok2, lik_d2 = _timed_vs_oracle(RING * B)
            err, idx_ok, lik_d = np.concatenate([err, err2]), idx_ok and idx_ok2, max(lik_d, lik_d2)
            checked.append("timed step %d (two batches in flight)" % RING)
        ncmp = err.shape[0]
        out["cpu_baseline"] = {
            "value": round(max(fps1, fps32), 3), "unit": "frames/s", "cores": nthreads, "kind": "port",
            "batch1_frames_per_s": round(fps1, 3), "batch32_frames_per_s": round(fps32, 3),
            "sample": "%d frames at batch 1 (the reference's operating point, %.1f s) + one batch of %d (%.1f s) of the same "
                      "workload after a 1-frame warm-up; fp32 torch-CPU restatement of the TF1 reference path (TF1 unavailable); "
                      "%d host CPUs visible, %d threads used: the fastest of 8/16/32/64/128 on this pool's boxes "
                      "(scripts/cpu_threads.py) -- more threads lose to synchronisation in the small late layers"
                      % (n1, c1 - c0, f32.shape[0], c3 - c2, os.cpu_count() or 0, nthreads),
        }
        out["accuracy_vs_oracle"] = {
            "px_rmse": float(np.sqrt((err ** 2).mean())), "px_max": float(err.max()), "frames": ncmp,
            "idx_bit_exact": idx_ok, "likelihood_max_abs_diff": lik_d,
            "what": "the packed trajectory written inside the timed region (" + " + ".join(checked) + "), every frame of the batch, vs the "
                    "CPU oracle on the same frames",
        }
        assert idx_ok and float(err.max()) < 1e-3, "timed trajectory outside the parity gate"
    if args.full and world == 1 and not args.no_strict_f32:
        # the IEEE-fp32 tier beside the fp32-class one, timed in THIS run: a fresh child process (the conv mode is read once per
        # process) runs the same workload on the fp32 MFMA kernels for a few steps
        import subprocess
        env = dict(os.environ, DGP_CONV_MODE="f32")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), "--strict-f32-child", "--batch", str(B), "--steps", "8"]
        if args.no_cpu_baseline:
            cmd.append("--no-cpu-baseline")
        for key, mode_ in (("strict_f32", "f32"), ("tier_f16", "f16")):
            # ("tier_f16": the 16-bit tier SURVEY 8(d) asks to report beside the parity tier -- 2-byte activation cells end to end, its own
            #  roofline object and its measured error over 256 frames; a reported tier, not a parity claim)
            cmd_ = list(cmd)
            if mode_ == "f16":
                env.pop("DGP_CONV_MODE", None)
                cmd_ = [sys.executable, os.path.abspath(__file__), "--tier-f16-child", "--batch", str(B), "--steps", str(min(args.steps, 64)),
                        "--cpu-threads", str(args.cpu_threads)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else [])
            else:
                env["DGP_CONV_MODE"] = mode_
            try:
                cp = subprocess.run(cmd_, env=env, capture_output=True, text=True, timeout=420)
                ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
                out[key] = json.loads(ln[-1]) if cp.returncode == 0 and ln else {"error": (cp.stderr or cp.stdout)[-300:]}
            except Exception as e:      # noqa: BLE001 -- the main line must still be printed
                out[key] = {"error": repr(e)[:300]}
    if args.full and world == 1 and not args.no_strict_f32 and not args.no_r101:
        # BASELINE configs[4]'s per-GPU shape (ResNet-101, 1280 x 720, 20 keypoints) in a fresh child process: block3 has 23 units there
        import subprocess
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "DGP_CONV_MODE"):
            env.pop(k, None)
        try:
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_r101.py"), "16", "--json"], env=env, capture_output=True, text=True,
                                timeout=600)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            out["r101_1280x720"] = json.loads(ln[-1]) if cp.returncode == 0 and ln else {"error": (cp.stderr or cp.stdout)[-300:]}
            # ... and on the 16-bit tier (a reported tier: frac against 2500 TFLOP/s)
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_r101.py"), "16", "--json", "--tier", "f16"], env=env, capture_output=True,
                                text=True, timeout=600)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            out["r101_1280x720_f16"] = json.loads(ln[-1]) if cp.returncode == 0 and ln else {"error": (cp.stderr or cp.stdout)[-300:]}
        except Exception as e:      # noqa: BLE001
            out.setdefault("r101_1280x720", {"error": repr(e)[:300]})
    if args.full and world == 1 and not args.no_train_step and not args.no_strict_f32:
        # BASELINE configs[3] next to the headline number, driver-timed: the semi-supervised fit_dgp step (1 labeled + 10 unlabeled 640 x 480
        # frames, gm2 = 1, gm3 = 3, skeleton clique; forward + loss + backward + clip + momentum) -- the call that replaces
        # sess.run([loss, train_op]) (DGP/models/fitdgp.py:801-818) -- in a fresh child process (scripts/bench_train.py), never a re-exec
        import subprocess
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "DGP_CONV_MODE"):
            env.pop(k, None)
        def _train_leg(tier):
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_train.py"), str(args.train_steps), "8", tier], env=env, capture_output=True,
                                text=True, timeout=600)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            if cp.returncode != 0 or not ln:
                return {"error": (cp.stderr or cp.stdout)[-300:]}
            t = json.loads(ln[-1])
            sus_ = mfma_only_sustained()[0] / (1.0 if tier == "f16" else 3.0)
            return {"ms_per_step": t["ms_per_step"], "steps": args.train_steps, "frames_per_step": t["nt"], "frames_per_s": t["frames_per_s"],
                    "frac": t["roofline"]["frac"], "achieved_tflops": t["roofline"]["achieved"], "peak_tflops": t["roofline"]["peak"],
                    "frac_of_mfma_only_sustained": round(t["roofline"]["achieved"] / sus_, 4),
                    "algorithmic_gflop_per_step": t["roofline"]["algorithmic_gflop_per_step"], "loss": t["loss"], "dtype": t["dtype"],
                    "fast_passes": t.get("fast_passes"), "fast_redos": t.get("fast_redos")}
        try:
            out["train_step"] = _train_leg("parity")
            if "error" not in out["train_step"]:
                out["train_step"].update(
                    workload="BASELINE configs[3]: fit_dgp step, ResNet-50 640x480, 1 labeled + 10 unlabeled frames, 4 keypoints, "
                             "fp32-class arithmetic (the parity tier), 8 warm-up steps then `steps` timed ones",
                    frac_basis="3 x forward conv FLOPs (forward + data-gradient + weight-gradient convolutions) / step time / (2500 / 3 TFLOP/s)")
            # the precision configs[3] names: the 16-bit tier of the same step (H1 activations / gradient tensors, one MFMA per product, fp32
            # master weights / momentum / accumulation); gradient agreement with the fp64 oracle: tests/test_train_gpu.py
            out["train_step_f16"] = _train_leg("f16")
            if "error" not in out["train_step_f16"]:
                out["train_step_f16"].update(
                    workload="the same step on the 16-bit tier (Trainer(tier='f16'), dgp_trainer_set_tier): 2-byte H1 activations and gradient tensors with "
                             "predicted scales in every bottleneck unit, weight gradients by LDS-DMA on the tensors themselves; root block = the inference engine's "
                             "fused kernel with the stem's weight gradient fused into the pool's backward, both heads' backward merged on ONE H1 panel; the "
                             "first step of a shape runs on the parity path; `fast_passes` counts what the DEVICE reported as 16-bit passes",
                    frac_basis="3 x forward conv FLOPs / step time / 2500 TFLOP/s (one MFMA per product)")
        except Exception as e:      # noqa: BLE001 -- the main line must still be printed
            out.setdefault("train_step", {"error": repr(e)[:300]})
    if args.full and world == 1 and not args.no_host_pipeline and not args.no_strict_f32:
        # the PCIe-inclusive rate of the boundary that takes HOST frames (A0 estimate_pose: decode thread -> pinned ring -> copy stream -> engines
        # -> one D2H), in a fresh child process; reported beside `value`, never as it
        import subprocess
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "DGP_CONV_MODE"):
            env.pop(k, None)
        try:
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_pipeline.py"), str(args.host_frames), "--json"], env=env, capture_output=True,
                                text=True, timeout=300)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            out["host_pipeline"] = json.loads(ln[-1]) if cp.returncode == 0 and ln else {"error": (cp.stderr or cp.stdout)[-300:]}
            # the same call on the 16-bit tier (estimate_pose(..., tier="f16")): whether the host side can feed an engine twice as fast
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_pipeline.py"), str(args.host_frames), "--json", "--tier", "f16"], env=env,
                                capture_output=True, text=True, timeout=300)
            ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
            out["host_pipeline_f16"] = json.loads(ln[-1]) if cp.returncode == 0 and ln else {"error": (cp.stderr or cp.stdout)[-300:]}
        except Exception as e:      # noqa: BLE001 -- the main line must still be printed
            out.setdefault("host_pipeline", {"error": repr(e)[:300]})
    if out["asserts_bypassed"]:
        out["value_unchecked"], out["value"] = out["value"], None
    print(json.dumps(out), flush=True)
    if use_pg:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
