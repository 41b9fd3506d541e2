"""Shared by the fit-preparation tests: the Reaching demo project's labeled frames as a PoseDataset with fit_dlc's overrides, seeded
sample walks, and Pillow's resample applied as numpy integer passes over tables that come from the library's host-only entry points."""
import os
import random
import shutil

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAT = os.path.join(HERE, "golden", "Reaching_Mackenzie95shuffle1.mat")
FRAMES = os.path.join(HERE, "golden", "reaching_frames")
PRECISION_BITS = 22
MAP_KEYS = ("part_score_targets", "part_score_weights", "locref_targets", "locref_mask")


def reaching_cfg(root, **over):
    """The labeled PNGs and the training .mat under `root`, and a PoseDataset config with fit_dlc's overrides (fitdgp.py:93-111)"""
    from deepgraphpose_amd.config import AttrDict
    root = str(root)
    if not os.path.isdir(os.path.join(root, "labeled-data")):
        shutil.copytree(FRAMES, os.path.join(root, "labeled-data", "reachingvideo1"))
        shutil.copy(MAT, root)
    cfg = AttrDict(project_path=root, dataset=os.path.basename(MAT), num_joints=5, locref_stdev=7.2801, stride=8.0, global_scale=0.8,
                   mirror=False, shuffle=True, crop=True, cropratio=0.4, pos_dist_thresh=8, location_refinement=True,
                   scale_jitter_lo=0.75, scale_jitter_up=1.25, batch_size=1, minsize=100, leftwidth=400, rightwidth=400,
                   topheight=400, bottomheight=400, weigh_only_present_joints=False, all_joints=[[i] for i in range(5)])
    cfg.update(over)
    return cfg


def seeded_dataset(cfg, seed):
    from deepgraphpose_amd.dlc_dataset import PoseDataset
    np.random.seed(seed)
    random.seed(seed)
    return PoseDataset(cfg)


def rng_state():
    s = np.random.get_state()
    return (s[0], s[1].tobytes(), s[2:], random.getstate())


def apply_plan(img, out_size, plan_fn):
    """resample axis -2 of a [..., n, C] uint8 array with plan_fn(in, out) -> (ksize, bounds, coeffs): Pillow's 8-bit pass"""
    _, bounds, coeffs = plan_fn(img.shape[-2], out_size)
    out = np.empty(img.shape[:-2] + (out_size, img.shape[-1]), np.uint8)
    src = img.astype(np.int32)
    for xx in range(out_size):
        x0, n = bounds[xx]
        ss = (src[..., x0:x0 + n, :] * coeffs[xx, :n, None]).sum(-2, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        out[..., xx, :] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resize_with(img, oh, ow, plan_fn):
    """[H, W, C] uint8 -> [oh, ow, C]: horizontal pass, clip to uint8, vertical pass"""
    hor = apply_plan(img, ow, plan_fn)
    return np.swapaxes(apply_plan(np.swapaxes(hor, -3, -2), oh, plan_fn), -3, -2)
