#!/usr/bin/env python3
"""What location refinement costs in the streaming path (dgp_infer_packed_locref: the locref head in the forward + the fused locref
read-out).  `bench_locref.py [steps]` runs one leg per arithmetic tier, each in a fresh child process under its own time limit, stops at
the first one that fails, and writes ONE JSON line to profiles/locref_bench_line.json (and to stdout).

Workload: ResNet-50, 640x480, 4 keypoints, batch 32, device-resident frames, engine.DGPPipeline with two engines (what estimate_pose
runs).  A step is one batch on each engine (two submits) and a join, timed with a hipEvent pair on the caller's stream; plain steps
(loc_ref=None: 5-lane records, the code path every run took before) and refined steps (loc_ref="dgp" / "dlc": 7-lane records) ALTERNATE
on the one box, so clock and temperature drift hits all of them alike; the medians after warm-up are reported, with frames/s.

launches: from dgp_net_profile_launch on one engine (hipEvent pairs around every launch, so launch gaps are not in them): the read-out
launch alone (plain soft_argmax, soft_argmax_locref, hard_argmax_locref) and the locref head's launch.

There is no gate on the refined rate: exit status 0 when every leg ran, 1 otherwise."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HW, NJ, BATCH, WARMUP = (480, 640), 4, 32, 10
LEG_TIMEOUT_S = 300
MODES = (None, "dgp", "dlc")


def leg(tier, steps):
    import numpy as np
    import torch
    from deepgraphpose_amd import engine
    from deepgraphpose_amd.synthetic import make_frames, make_weights
    wts = make_weights(50, NJ, True, seed=0, head_std=0.05)
    pipe = engine.DGPPipeline(50, NJ, HW[0], HW[1], max_batch=BATCH, with_locref=True, n_streams=2, tier=tier)
    pipe.load_weights(wts)
    frames = torch.from_numpy(np.concatenate([make_frames(16, HW[0], HW[1], NJ, seed=0)] * (BATCH // 16))).cuda()
    traj = {m: [torch.zeros((BATCH, NJ, engine.record_lanes(m)), dtype=torch.float32, device="cuda") for _ in pipe.nets] for m in MODES}

    def step(mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in traj[mode]:
            pipe.submit(frames, t, 1.0, 1, loc_ref=mode)
        pipe.join()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = {m: [] for m in MODES}
    for k in range(WARMUP + steps):
        for m in MODES:                                    # plain, dgp, dlc, plain, ...: alternating
            t = step(m)
            if k >= WARMUP:
                ms[m].append(t)
    overflow = bool(pipe.range_status()[0])
    name = lambda m: "plain" if m is None else m
    res = {"tier": pipe.nets[0].tier, "steps_per_variant": steps, "frames_per_step": 2 * BATCH, "range_overflow": overflow}
    for m in MODES:
        med = float(np.median(ms[m]))
        res[name(m)] = {"step_ms_median": round(med, 4), "step_ms_p10": round(float(np.percentile(ms[m], 10)), 4),
                        "step_ms_p90": round(float(np.percentile(ms[m], 90)), 4), "frames_per_s": round(2 * BATCH / med * 1e3, 1)}
    for m in MODES[1:]:
        res[m]["cost_vs_plain"] = round(res[m]["step_ms_median"] / res["plain"]["step_ms_median"] - 1.0, 4)
    # lanes 0..4 of the refined "dgp" records are the plain records, on this very workload
    res["dgp_lanes_0_4_equal_plain"] = bool(torch.equal(traj["dgp"][0][..., :5].contiguous().view(torch.int32), traj[None][0].view(torch.int32)))
    # the read-out launch and the locref head alone, one engine, launches timed one by one
    net = pipe.nets[0]
    launches = {}
    for m in MODES:
        net.profile_begin(20)
        for _ in range(20):
            net.infer_packed(frames, traj[m][0], 1.0, 1, loc_ref=m)
        torch.cuda.synchronize()
        _, rows = net.profile_end()
        launches[name(m)] = {"readout": [(n, round(t, 4)) for n, _, t in rows if "argmax" in n],
                             "locref_head_ms": [round(t, 4) for n, _, t in rows if "locref_pred" in n],
                             "part_head_ms": [round(t, 4) for n, _, t in rows if "part_pred" in n],
                             "n_launches": len(rows), "sum_ms": round(sum(t for _, _, t in rows), 4)}
    res["launches"] = launches
    return res


def main():
    if "--leg" in sys.argv:
        tier = sys.argv[sys.argv.index("--leg") + 1]
        print(json.dumps(leg(tier, int(sys.argv[sys.argv.index("--steps") + 1]))), flush=True)
        return 0
    steps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 60
    out = {"bench": "locref", "workload": "DGPPipeline (2 engines) on device-resident frames: ResNet-50, %dx%d, %d keypoints, batch %d; plain / "
                                          "dgp / dlc steps alternate, median of hipEvent-timed steps after %d warm-up rounds"
                                          % (HW[1], HW[0], NJ, BATCH, WARMUP)}
    rc = 0
    for tier in ("parity", "f16"):
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--leg", tier, "--steps", str(steps)]
        cp = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        ln = [q for q in cp.stdout.splitlines() if q.startswith("{")]
        if cp.returncode != 0 or not ln:
            out[tier] = {"error": "exit status %d: %s" % (cp.returncode, (cp.stderr or cp.stdout)[-400:])}
            rc = 1
            break                                            # nothing more is started on the GPU after a failure
        out[tier] = json.loads(ln[-1])
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "locref_bench_line.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
