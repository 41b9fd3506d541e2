"""Drop-in counterparts of deepgraphpose/models/fitdgp.py on the MI355X training engine.

  fit_dgp_labeledonly(snapshot, dlcpath, ...)   DGP/models/fitdgp.py:257-546   (step 1)
  fit_dgp(snapshot, dlcpath, ...)               DGP/models/fitdgp.py:549-845   (step 2)
  dgp_loss(data_batcher, dgp_cfg)               DGP/models/fitdgp.py:848-1144  (loss pre-computation + closure)
  fit_dlc(snapshot, dlcpath, ...)               DGP/models/fitdgp.py:53-254    (step 0: DLC baseline trainer)

One iteration = `TrainSession.run([loss, train_op], feed_dict)` (models/session.py) = the reference's sess.run([loss, train_op]): it calls
`Trainer.forward_backward` and then `Trainer.apply_gradients`, each with a read-back of its own (the losses, the gradient norm).
`Trainer.step` (deepgraphpose_amd/train.py) is the same step with a single synchronisation; the training benchmark times that one,
the drivers here do not use it.
Snapshots are what the reference's tf.train.Saver leaves in the train folder (fitdgp.py:239-245, 535-540, 832-839):
TensorFlow V2 bundles `snapshot-step{k}--{it}.{index,data-00000-of-00001}`, `snapshot-step{k}--0.*` and
`snapshot-step{k}-final--0.*` plus the `checkpoint` state file, written without TensorFlow (weights_io.Saver,
tf_checkpoint.py); DGP_SNAPSHOT_FORMAT=npz writes `.npz` files of the same names instead.
Host-side hooks: augmentation of the labeled frames (`aug`; deepgraphpose_amd/augment.py: imgaug's pipeline when imgaug is
installed, the numpy / scipy restatement of the same seven augmenters otherwise; fit_dgp*(aug_backend="hip") applies the numpy
pipeline's plan on the device, csrc/dgp_augment.hip) and the Farneback optical flow feeding the
temporal clique (`wt > 0`): OpenCV's on the host when cv2 is importable, otherwise the HIP kernels (csrc/dgp_flow.hip) on the
device -- fit_dgp(flow_backend="cv2" | "hip" | "auto").
"""
from __future__ import annotations

import os
import time
from os import listdir
from os.path import isfile, join
from pathlib import Path
from random import randint

import numpy as np
import torch.distributed as dist

from .. import config as dcfg
from .. import dist as ddist
from ..dataset import MultiDataset, coord2map
from ..loss import DGPHyper
from ..staged import (_FrameStore, _FrameUploader, _ImageCache, _device_augment, _device_flow, _device_locref, _device_sample, _flow_of,
                      _on_current_stream)
from .fitdgp_util import gen_batch

PREFETCH_DEPTH = 2          # iterations of host batches built ahead on a background thread (0: inline); a measured setting, not a switch

PREP_BACKENDS = ("auto", "host", "hip")
# the sample-preparation backend of the last fit_* run ("host" | "hip"), like eval.RUN_STATS["prep_backend"], and its frame stores: None
# with frame_store="off", else {"frames": stored, "bytes": on the device, "refused": selected frames without a slot, "fill_s": seconds
# of the fill, "patched": frames of the LAST batch that were uploaded instead of gathered from a slot}
# "aug": None with aug=False, else {"backend": aug_backend, "frames": labeled frames augmented so far, "stages": {name: plans holding it}}
PREP_STATS = {"backend": None, "frame_store": None, "aug": None}


def resolve_prep_backend(backend: str = "auto", device=None) -> str:
    """"host" | "hip" for fit_*(prep_backend=...): where a fit driver's samples are built -- crop, imresize and the DLC target maps of
    fit_dlc, the locref maps of the DGP drivers.  "auto" follows flow_backend's rule: the host when OpenCV is importable (imresize then
    runs cv2.INTER_AREA, the reference's own filter, which the device path does not restate), the HIP kernels otherwise -- when
    `device`, the trainer's, is a GPU (None: only the name is checked, "auto" stays "auto")."""
    if backend not in PREP_BACKENDS:
        raise ValueError("prep backend must be one of %s, not %r" % (" | ".join(PREP_BACKENDS), backend))
    if backend != "auto" or device is None:
        return backend
    import torch
    from .fitdgp_util import _cv2_available
    return "host" if _cv2_available() or torch.device(device).type != "cuda" else "hip"


FRAME_STORES = ("off", "hip")


def resolve_frame_store(frame_store: str = "off", wt=0, flow_backend=None) -> str:
    """"off" | "hip" for fit_dgp*(frame_store=...).  "off": every batch reads its frames from the source (Dataset.load_data) and uploads
    them.  "hip": the run's selected frames are decoded once into a device store (staged._FrameStore) and every batch is gathered from it
    (engine.gather_frames).  `wt`, `flow_backend`: the run's temporal-clique weight and its RESOLVED flow backend -- a flow computed on the
    host (cv2) needs every frame of every batch on the host, which is what the store does away with, so that pair is refused."""
    if frame_store not in FRAME_STORES:
        raise ValueError("frame store must be one of %s, not %r" % (" | ".join(FRAME_STORES), frame_store))
    if frame_store == "hip" and wt > 0 and flow_backend != "hip":
        raise ValueError("frame_store='hip' keeps the batch's frames on the device, but flow_backend=%r computes the optical flow of the "
                         "temporal clique (wt > 0) on the host and needs every frame there; use flow_backend='hip' or frame_store='off'"
                         % (flow_backend,))
    return frame_store


OPTIMIZERS = ("sgd", "adam")


def resolve_optimizer(optimizer=None, configured="sgd") -> str:
    """The optimiser of a fit driver: `optimizer`, or pose_cfg.yaml's `optimizer` key when None (PET/train.py:94-113, get_optimizer):
    "sgd" = MomentumOptimizer(lr, 0.9), "adam" = AdamOptimizer(lr); anything else is the reference's ValueError."""
    name = configured if optimizer is None else optimizer
    if name not in OPTIMIZERS:
        raise ValueError("unknown optimizer {}".format(name))
    return name


_STATE_KEYS = {"sgd": lambda k: k.endswith("/Momentum"),
               "adam": lambda k: k.endswith(("/Adam", "/Adam_1")) or k in ("beta1_power", "beta2_power")}


def _restore_optimizer_state(trainer, init_weights, optimizer):
    """keep_optimizer_state: when the snapshot a run starts from holds the state of the optimiser it is about to use, put it back"""
    from .. import weights_io
    state = {k: v for k, v in weights_io.load_optimizer_state(init_weights).items() if _STATE_KEYS[optimizer](k)}
    if state:
        trainer.load_optimizer_state(state)
        print("Restored the {} optimizer state ({} tensors) from {}".format(optimizer, len(state), init_weights), flush=True)


def _snapshot_tensors(trainer, keep_optimizer_state):
    """What a snapshot holds: the model variables, and with keep_optimizer_state the optimiser's under the names tf.train.Saver gives them"""
    w = trainer.get_weights()
    if keep_optimizer_state:
        w.update(trainer.get_optimizer_state())
    return w


_VIDEO_EXT = ("avi", "mp4", "mov", "mkv")


def _video_sets(dlc_base_path: Path, cfg):
    """<project>/videos_dgp/* when present, else the project's video_sets (fitdgp.py:589-604).  Directories of
    frames and .npy stacks are accepted next to real videos (no decoder is required for them)."""
    video_path = str(dlc_base_path / "videos_dgp")
    if not os.path.exists(video_path):
        print(video_path + " does not exist!")
        return list(cfg["video_sets"])
    out = []
    for f in sorted(listdir(video_path)):
        p = join(video_path, f)
        if (isfile(p) and (any(f.find(e) > 0 for e in _VIDEO_EXT) or f.endswith(".npy"))) or os.path.isdir(p):
            out.append(p)
    return out


def _limb_statistics(labels_list, S0, stride, ws, ws_max):
    """ws_l = ws / mean non-zero limb length, ws_max_l = ws_max * max limb length, in px (fitdgp.py:875-892)."""
    nj = S0.shape[1]
    full = np.empty((0, nj, 2))
    for j in labels_list:
        if len(j) > 0:
            full = np.vstack((j, full))
    j1 = np.copy(full).swapaxes(1, 2).reshape(-1, nj)
    j1[np.isnan(j1)] = 1e10
    limb = np.matmul(j1, S0.T)
    limb[np.abs(limb) > 1e5] = 0
    limb = np.sqrt(np.sum(np.square(np.reshape(limb, [full.shape[0], 2, -1])), 1))
    limb = limb.T * stride + stride / 2
    ws_max_v = np.max(np.nan_to_num(limb), 1) * ws_max if limb.size else np.zeros(S0.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_nz = np.true_divide(limb.sum(1), (limb != 0).sum(1)) if limb.size else np.zeros(S0.shape[0])
    return 1 / (np.nan_to_num(mean_nz) + 1e-20) * ws, ws_max_v


def dgp_loss(data_batcher, dgp_cfg):
    """-> (loss, total_loss, total_loss_visible, placeholders), the reference's return contract (fitdgp.py:848, 1130-1144):
    `loss` maps the loss-term names to evaluable handles, `placeholders` holds the same 12 keys, and
    `TrainSession(trainer, loss.graph).run([loss, train_op], feed_dict)` is the reference's `sess.run([loss, train_op], feed_dict)`
    (models/session.py).  The pre-computation of fitdgp.py:865-892 (limb statistics -> ws, ws_max) happens here; the loss terms
    themselves are HIP kernels (csrc/dgp_loss.hip) launched by the session."""
    from .session import LossGraph
    hyper = DGPHyper(ws=dgp_cfg.ws, ws_max=dgp_cfg.ws_max, wt=dgp_cfg.wt, wt_max=dgp_cfg.wt_max,
                     wn_visible=dgp_cfg.wn_visible, wn_hidden=dgp_cfg.wn_hidden, gamma=dgp_cfg.gamma,
                     gauss_len=dgp_cfg.gauss_len, lengthscale=dgp_cfg.lengthscale, lr=dgp_cfg.lr, gm2=dgp_cfg.gm2,
                     gm3=dgp_cfg.gm3, stride=dgp_cfg.stride, locref_loss_weight=dgp_cfg.locref_loss_weight,
                     locref_huber_loss=dgp_cfg.locref_huber_loss)
    if hyper.gm2 not in (0, 1, 2) or hyper.gm3 not in (0, 3):
        raise Exception("Not implemented")                        # fitdgp.py:1019, :1036
    S0 = np.asarray(data_batcher.S0, dtype=np.float64).reshape(-1, data_batcher.nj)
    ws, ws_max = _limb_statistics([d.labels for d in data_batcher.datasets], S0, dgp_cfg.stride, dgp_cfg.ws,
                                  dgp_cfg.ws_max)
    graph = LossGraph(hyper, S0, ws, ws_max, data_batcher.n_frames_total, data_batcher.n_visible_frames_total,
                      data_batcher.nj)
    return graph.loss, graph.total_loss, graph.total_loss_visible, graph.placeholders


def _feed(placeholders, images, joint_loc, lmap, lmask, addn, wt_mask, vector_field, wt, nx_out, ny_out, learning_rate, lr):
    """The reference's feed_dict (fitdgp.py:796-815), key for key."""
    vm, hm, vt = addn
    nt = images.shape[0]
    xg, yg = np.meshgrid(np.linspace(0, nx_out - 1, nx_out), np.linspace(0, ny_out - 1, ny_out))
    alpha = np.array([xg, yg]).swapaxes(1, 2)                     # 2 x nx_out x ny_out
    return {placeholders["inputs"]: images, placeholders["targets"]: joint_loc, placeholders["locref_map"]: lmap,
            placeholders["locref_mask"]: lmask, placeholders["visible_marker_pl"]: vm, placeholders["hidden_marker_pl"]: hm,
            placeholders["visible_marker_in_targets_pl"]: vt,
            placeholders["wt_batch_mask_pl"]: np.asarray(wt_mask if wt_mask is not None else np.ones(max(nt - 1, 0))),
            placeholders["vector_field_tf"]: vector_field, placeholders["nt_batch_pl"]: nt,
            placeholders["wt_batch_pl"]: np.ones(max(nt - 1, 0)) * wt, placeholders["alpha_tf"]: alpha, learning_rate: lr}


def _setup(snapshot, dlcpath, shuffle, trainingsetindex, frame_sources):
    dlc_base_path = Path(dlcpath)
    config_path = dlc_base_path / "config.yaml"
    print("config_path", config_path)
    cfg = dcfg.read_config(config_path)
    modelfolder = dcfg.GetModelFolder(cfg["TrainingFraction"][trainingsetindex], shuffle, cfg)
    train_path = dlc_base_path / modelfolder / "train"
    video_sets = _video_sets(dlc_base_path, cfg)
    print("video_sets: ", video_sets)
    S0 = dcfg.skeleton_matrix(cfg)
    data_batcher = MultiDataset(config_yaml=config_path, video_sets=video_sets, shuffle=shuffle, S0=S0,
                                sources=frame_sources)
    return data_batcher, str(train_path / snapshot)


def _dp_index(it, n):
    """Data-parallel runs (torch.distributed initialised, world W > 1): the schedule is identical on every
    rank (same seeds), iteration `it` of rank r consumes entry it*W + r, and TrainSession.run averages the gradients over the
    ranks -- W windows per optimiser step.  Single process: the reference's schedule, unchanged."""
    if ddist.data_parallel():
        return (it * dist.get_world_size() + dist.get_rank()) % n
    return it


def _make_trainer(data_batcher, init_weights, max_frames, device=0):
    import torch  # noqa: F401
    from .. import weights_io
    from ..train import Trainer
    wts = weights_io.load_weights(init_weights)
    depth = weights_io.net_depth(wts)
    nj = data_batcher.nj
    if "pose/locref_pred/block4/weights" not in wts:
        raise KeyError("snapshot %s has no pose/locref_pred head (dgp_loss trains both heads)" % init_weights)
    # DGP_TRAIN_TIER=f16: the 16-bit tier of the training step (BASELINE configs[3]'s precision; include/dgp_hip.h, dgp_trainer_set_tier);
    # default: the parity tier
    tr = Trainer(depth, nj, data_batcher.nx_in, data_batcher.ny_in, max_frames=max_frames, device=device,
                 tier=os.environ.get("DGP_TRAIN_TIER") or None)
    tr.load_weights(wts)
    return tr


def _make_uploader(trainer):
    """The prefetch thread's frame uploader (staged.py), or None when batches are built inline (PREFETCH_DEPTH = 0, read at call time)."""
    return _FrameUploader(trainer.device) if PREFETCH_DEPTH > 0 else None


def _locref_targets(joint_loc, nt, vis_within, nx_out, ny_out, nj, dgp_cfg):
    lt, lm = coord2map(joint_loc, nx_out, ny_out, nj, dgp_cfg.pos_dist_thresh, dgp_cfg.locref_stdev) \
        if joint_loc.shape[0] else (np.zeros((0,)), np.zeros((0,)))
    lmap = np.zeros((nt, nx_out, ny_out, nj * 2), dtype=np.float32)       # fp32 here (on the prefetch thread): the trainer's upload of
    lmask = np.zeros((nt, nx_out, ny_out, nj * 2), dtype=np.float32)      # the two maps is then a plain copy, no conversion pass
    if lm.shape[0] != 0:
        lmap[vis_within], lmask[vis_within] = lt, lm
    return lmap, lmask


def _save(saver, trainer, prefix, step, it, final, debug="", keep_optimizer_state=False):
    """The reference's three Saver.save calls (fitdgp.py:535-540, 832-839): `<prefix>-step{k}-` at global_step it and 0, and
    `<prefix>-step{k}-final-` at 0 after the last iteration."""
    if ddist.data_parallel() and dist.get_rank() != 0:      # every rank holds the same weights: one writer
        return
    w = _snapshot_tensors(trainer, keep_optimizer_state)
    model_name = prefix + "-step" + str(step) + debug + "-"
    saver.save(w, model_name, global_step=it)
    saver.save(w, model_name, global_step=0)
    if final:
        saver.save(w, prefix + "-step" + str(step) + debug + "-final-", global_step=0)


AUG_BACKENDS = ("host", "hip")
_SAID_NUMPY_PLANS = [False]


def resolve_aug_backend(aug_backend: str = "host", device=None) -> str:
    """"host" | "hip" for fit_dgp*(aug_backend=...): where the pixels of the labeled frames are augmented.  "host": the pipeline object
    runs on the prefetch thread (augment.data_aug).  "hip": the draws and the labels stay on the host (augment.plan_aug) and the pixels
    are made on the device from the plan (engine.augment_frames); `device`, the trainer's, must then be a GPU (None: only the name is
    checked)."""
    if aug_backend not in AUG_BACKENDS:
        raise ValueError("aug backend must be one of %s, not %r" % (" | ".join(AUG_BACKENDS), aug_backend))
    if aug_backend == "hip" and device is not None:
        import torch
        if torch.device(device).type != "cuda":
            raise ValueError("aug_backend='hip' augments the labeled frames on the GPU, but the trainer's device is %s; use "
                             "aug_backend='host'" % (device,))
    return aug_backend


def _aug_pipeline(dgp_cfg, aug_backend="host"):
    """The augmentation pipeline of the labeled frames (fitdgp.py:446-447, 735-736: build_aug(apply_prob=0.8)), or None.  aug_backend
    "hip" needs a plan, which only the numpy pipeline draws: it is built even when imgaug is importable (said once)."""
    if not dgp_cfg.aug:
        return None
    from ..augment import build_aug
    if aug_backend != "hip":
        return build_aug(apply_prob=0.8)
    try:
        import imgaug  # noqa: F401
        if not _SAID_NUMPY_PLANS[0]:
            _SAID_NUMPY_PLANS[0] = True
            print("aug_backend='hip': the augmentation is planned by the numpy pipeline (imgaug's own pipeline object draws no plan)",
                  flush=True)
    except ImportError:
        pass
    return build_aug(apply_prob=0.8, backend="numpy")


def _count_aug(plans):
    """PREP_STATS["aug"]: the frames augmented so far in this run and how many of their plans hold each stage"""
    from ..augment import plan_stages
    stats = PREP_STATS["aug"]
    stats["frames"] += len(plans)
    for stage, k in plan_stages(plans).items():
        stats["stages"][stage] = stats["stages"].get(stage, 0) + k


def _dp_setup():
    """Data-parallel runs (torchrun: RANK / WORLD_SIZE in the environment): join the process group BEFORE any GPU use and
    return (rank, world, local_rank).  The batch schedule must be identical on every rank, so rank 0's RNG seeds are broadcast."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return 0, 1, 0
    import random
    import torch
    rank, local, world = ddist.init_from_env()
    seed = torch.tensor([np.random.randint(0, 2 ** 31 - 1)], dtype=torch.int64)
    if dist.get_backend() == "nccl":
        seed = seed.cuda(local)
    dist.broadcast(seed, 0)
    np.random.seed(int(seed.item()))
    random.seed(int(seed.item()))
    return rank, world, local


def _prefetched(make_item, n_items: int, depth=None):
    """make_item(0), make_item(1), ... in order, built by ONE background thread up to `depth` items ahead of the consumer: the host
    work of iteration it + 1 (frame reads, augmentation, target maps) runs while the GPU trains on iteration it.  A single producer
    keeps the order of every random draw, so a run is the same with or without prefetching (PREFETCH_DEPTH = 0: inline)."""
    import queue
    import threading
    if depth is None:
        depth = PREFETCH_DEPTH
    if depth <= 0 or n_items <= 1:
        for i in range(n_items):
            yield make_item(i)
        return
    q = queue.Queue(maxsize=depth)
    stop = threading.Event()

    def work():
        try:
            for i in range(n_items):
                item = make_item(i)
                while not stop.is_set():
                    try:
                        q.put((item, None), timeout=0.1)
                        break
                    except queue.Full:
                        pass
                if stop.is_set():
                    return
        except BaseException as e:      # surfaces in the consumer
            while not stop.is_set():
                try:
                    q.put((None, e), timeout=0.1)
                    break
                except queue.Full:
                    pass

    th = threading.Thread(target=work, name="dgp-batch-prefetch", daemon=True)
    th.start()
    try:
        for _ in range(n_items):
            item, err = q.get()
            if err is not None:
                raise err
            yield item
    finally:
        stop.set()
        th.join(timeout=5.0)


def _pretrained_checkpoint(net_type: str, dlc_cfg) -> str:
    """ImageNet backbone checkpoint `resnet_v1_<depth>.ckpt`.  The reference looks inside the installed deeplabcut
    package (fitdgp.py:101-106); here: $DGP_PRETRAINED_DIR, <package>/pretrained/, then pose_cfg.yaml's init_weights."""
    name = net_type.split("_")[0] + "_v1_" + net_type.split("_")[1] + ".ckpt"
    here = Path(__file__).resolve().parent.parent
    cands = [Path(os.environ["DGP_PRETRAINED_DIR"]) / name] if os.environ.get("DGP_PRETRAINED_DIR") else []
    cands += [here / "pretrained" / name, Path(str(dlc_cfg.get("init_weights", "")))]
    for c in cands:
        for suffix in ("", ".npz", ".index", ".safetensors"):
            if str(c) and os.path.isfile(str(c) + suffix):
                return str(c)
    raise FileNotFoundError("ImageNet checkpoint %s not found (looked in %s); set DGP_PRETRAINED_DIR or start from a "
                            "snapshot via the `snapshot` argument" % (name, ", ".join(str(c) for c in cands)))


def _fresh_heads(wts, depth, nj, seed=None):
    """Head variables absent from an ImageNet checkpoint, initialised like slim.conv2d_transpose does
    (pose_net.py:37-44: xavier/glorot-uniform weights over (fan_in + fan_out)/2, zero biases)."""
    rng = np.random.RandomState(seed)
    cin = wts["resnet_v1_%d/block4/unit_3/bottleneck_v1/conv3/weights" % depth].shape[-1]
    for scope, cout in (("pose/part_pred/block4", nj), ("pose/locref_pred/block4", 2 * nj)):
        if scope + "/weights" in wts:
            continue
        fan_in, fan_out = cout * 9, cin * 9                      # kernel [3,3,out,in]: fan_in = shape[-2]*9, fan_out = shape[-1]*9
        limit = np.sqrt(3.0 / ((fan_in + fan_out) / 2.0))
        wts[scope + "/weights"] = rng.uniform(-limit, limit, size=(3, 3, cout, cin)).astype(np.float32)
        wts[scope + "/biases"] = np.zeros(cout, dtype=np.float32)
    return wts


def fit_dlc(snapshot, dlcpath, shuffle=1, step=0, saveiters=1000, displayiters=100, maxiters=200000,
            trainingsetindex=0, prep_backend="auto", optimizer=None, keep_optimizer_state=False):
    """Run the DLC baseline trainer (step 0), DGP/models/fitdgp.py:53-254: one randomly scaled / cropped labeled
    image per iteration (PoseDataset), loss = sigmoid CE on binary target disks + locref Huber (pose_net.train),
    multi-step learning rate, MomentumOptimizer(0.9) without clipping; snapshots snapshot-step0-{it} and
    snapshot-step0-final--0.  `snapshot`: a 'snapshot-*' name inside the train folder, or anything else to start
    from the ImageNet resnet_v1_<depth>.ckpt.
    prep_backend: "host" | "hip" | "auto" (resolve_prep_backend).  "host": every sample is read, cropped, resized and its four target
    maps are built by PoseDataset.next_batch, then uploaded.  "hip": the prefetch thread draws the sample's plan
    (PoseDataset.plan_batch) and the pixels (engine.window_resize, from a device cache of the labeled images) and the maps
    (engine.target_maps) are made on the device, bit for bit the host path's without OpenCV; the main thread uploads nothing.
    optimizer: None (pose_cfg.yaml's `optimizer`, default "sgd") | "sgd" | "adam" (resolve_optimizer): MomentumOptimizer(lr, 0.9) or
    AdamOptimizer(lr) with TF's defaults, neither with clipping (PET/train.py:94-113).
    keep_optimizer_state: snapshots also hold the optimiser's state (`<var>/Momentum`, or `<var>/Adam`, `<var>/Adam_1`, beta1_power,
    beta2_power, as tf.train.Saver names them), and a run that starts from a snapshot holding the state of its optimiser restores it.
    Default: snapshots hold the model variables alone and every run starts from zero state."""
    import torch
    prep_backend = resolve_prep_backend(prep_backend)
    from .. import weights_io
    from ..dlc_dataset import LearningRate, PoseDataset
    from ..train import Trainer

    # data-parallel like the other fit drivers: every rank draws the SAME sample sequence (seeds broadcast by _dp_setup) and takes
    # every W-th sample, Trainer averages the gradients over the ranks, rank 0 alone writes snapshots and the learning-stats file
    rank, world, local_rank = _dp_setup()
    dlc_base_path = Path(dlcpath)
    config_path = dlc_base_path / "config.yaml"
    print("config_path", config_path)
    cfg = dcfg.read_config(config_path)
    modelfoldername = dcfg.GetModelFolder(cfg["TrainingFraction"][trainingsetindex], shuffle, cfg)
    pose_config_yaml = Path(os.path.join(cfg["project_path"], str(modelfoldername), "train", "pose_cfg.yaml"))

    dlc_cfg = dcfg.load_config(pose_config_yaml)                  # fitdgp.py:93-111: the reference's overrides
    dlc_cfg.crop = True
    dlc_cfg.cropratio = 0.4
    dlc_cfg.global_scale = 0.8
    dlc_cfg.multi_step = [[0.001, 10000], [0.005, 430000], [0.002, 730000], [0.001, 1030000]]
    final = dlc_cfg.snapshot_prefix + "-step0-final--0"
    if weights_io.exists(final):
        print(final, "  exists! The original DLC has already been run.", flush=True)
        return None
    if "snapshot" in snapshot:
        init_weights = str(dlc_base_path / modelfoldername / "train" / snapshot)
    else:
        init_weights = _pretrained_checkpoint(dlc_cfg.net_type, dlc_cfg)
    dlc_cfg.init_weights = init_weights
    dlc_cfg.pos_dist_thresh = 8
    dlc_cfg.output_stride = 16

    if dlc_cfg.batch_size != 1:
        raise ValueError("fit_dlc: batch_size must be 1 (every sample has its own size)")
    if dlc_cfg.intermediate_supervision:
        raise NotImplementedError("intermediate_supervision is off in every DGP configuration and is not built")
    optimizer = resolve_optimizer(optimizer, dlc_cfg.optimizer)

    dataset = PoseDataset(dlc_cfg)
    wts = weights_io.load_weights(init_weights)
    depth = weights_io.net_depth(wts)
    nj = int(dlc_cfg.num_joints)
    if "snapshot" in Path(init_weights).stem:
        print("Loading already trained DLC with backbone:", dlc_cfg.net_type, flush=True)
    else:
        print("Loading ImageNet-pretrained", dlc_cfg.net_type, flush=True)
        wts = {k: v for k, v in wts.items() if k.startswith("resnet_v1")}
    wts = _fresh_heads(wts, depth, nj)
    trainer = Trainer(depth, nj, 64, 64, max_frames=1, device=local_rank)
    trainer.load_weights(wts)
    if keep_optimizer_state and "snapshot" in Path(init_weights).stem:
        _restore_optimizer_state(trainer, init_weights, optimizer)

    display_iters = max(1, int(dlc_cfg.get("display_iters", 1000) if displayiters is None else displayiters))
    save_iters = max(1, int(dlc_cfg.get("save_iters", 50000) if saveiters is None else saveiters))
    max_iter = int(dlc_cfg.multi_step[-1][1]) if maxiters is None else min(int(dlc_cfg.multi_step[-1][1]), int(maxiters))
    print("Display_iters overwritten as", display_iters, flush=True)
    print("Save_iters overwritten as", save_iters, flush=True)
    print("Max_iters overwritten as", max_iter, flush=True)

    saver = weights_io.Saver(max_to_keep=5)                       # fitdgp.py:150-152
    lr_gen = LearningRate(dlc_cfg)
    stats_path = Path(pose_config_yaml).with_name("learning_stats.csv")
    lrf = open(str(stats_path) if rank == 0 else os.devnull, "w")
    cumloss, partloss, locrefloss = 0.0, 0.0, 0.0
    print("Starting training....", flush=True)
    dev = trainer.device
    prep_backend = resolve_prep_backend(prep_backend, dev)
    PREP_STATS["backend"] = prep_backend
    uploader = _make_uploader(trainer) if prep_backend == "hip" else None
    cache = _ImageCache(dataset, dev, uploader) if prep_backend == "hip" else None

    def own_sample():
        if prep_backend != "hip":
            return dataset.next_batch()
        frames, maps = _device_sample(dataset, dataset.plan_batch(), cache, uploader, dev)
        return dict(maps, inputs=frames)

    def next_sample(_i):                      # W samples per optimiser step: rank r trains on sample it * W + r of the common sequence
        batch = None
        for r in range(world):                # the other ranks' samples only advance the random streams (no image read, no target maps)
            if r == rank:
                batch = own_sample()
            else:
                dataset.skip_batch()
        return batch

    max_iter = max(1, max_iter // world) if world > 1 else max_iter
    for it, batch in enumerate(_prefetched(next_sample, max_iter + 1)):      # image read / scale / targets one step ahead
        current_lr = lr_gen.get_lr(it * world)
        img = batch["inputs"]
        frames = _on_current_stream(img) if prep_backend == "hip" else torch.from_numpy(img).to(dev)
        trainer.set_input_size(frames.shape[1], frames.shape[2])
        losses = trainer.forward_backward_dlc(
            frames, batch["part_score_targets"], batch["locref_targets"], batch["locref_mask"],
            part_score_weights=batch["part_score_weights"] if dlc_cfg.weigh_part_predictions else None,
            locref_loss_weight=dlc_cfg.locref_loss_weight, locref_huber_loss=dlc_cfg.locref_huber_loss,
            location_refinement=dlc_cfg.location_refinement)
        if world > 1:
            trainer.allreduce_gradients()         # mean gradient over the ranks (RCCL): replicas stay bit-identical
        trainer.apply_gradients(current_lr, 0.9, clip_norm=0.0, optimizer=optimizer)  # Momentum / Adam, no clipping (train.py:94-113)

        partloss += losses["part_loss"]
        if dlc_cfg.location_refinement:
            locrefloss += losses["locref_loss"]
        cumloss += losses["total_loss"]
        if it % display_iters == 0 and it > 0:
            vals = (it, "total loss {0:.4f}".format(cumloss / display_iters),
                    "scoremap loss {0:.4f}".format(partloss / display_iters),
                    "learning rate {0:.4f}".format(locrefloss / display_iters), current_lr)     # labels as in fitdgp.py:212-230
            print("iteration: {} loss: {} scmap loss: {} locref loss: {} lr: {}".format(*vals), flush=True)
            lrf.write("iteration: {}, loss: {}, scmap loss: {}, locref loss: {}, lr: {}\n".format(*vals))
            lrf.flush()
        if rank == 0 and ((it % save_iters == 0 and it != 0) or it == max_iter):      # fitdgp.py:237-245
            w = _snapshot_tensors(trainer, keep_optimizer_state)
            saver.save(w, dlc_cfg.snapshot_prefix + "-step" + str(step) + "-", global_step=it)
            if it == max_iter:
                saver.save(w, dlc_cfg.snapshot_prefix + "-step" + str(step) + "-final-", global_step=0)
    print("Finish training {} iterations\n".format(it), flush=True)
    lrf.close()
    return None


def _open_project(snapshot, dlcpath, shuffle, trainingsetindex, frame_sources, hyper, final, done, ns, nc, n_max_frames):
    """What a DGP driver does before it builds anything: join the process group, read the project, put its hyper-parameters on the
    config singleton, stop when `<snapshot_prefix><final>` already exists, select the frames.
    -> (data_batcher, init_weights, world, local_rank), or None when this step has been run before."""
    from .. import weights_io
    rank, world, local_rank = _dp_setup()
    data_batcher, init_weights = _setup(snapshot, dlcpath, shuffle, trainingsetindex, frame_sources)
    dgp_cfg = data_batcher.dlc_config
    dgp_cfg.update(**hyper)
    final = dgp_cfg.snapshot_prefix + final
    if weights_io.exists(final):
        print(final, done, flush=True)
        return None
    data_batcher.create_batches_from_resnet_output(0, ns_jump=None, step=1, ns=ns, nc=nc, n_max_frames=n_max_frames)
    return data_batcher, init_weights, world, local_rank


def _train(data_batcher, init_weights, world, local_rank, *, labeled_only, max_frames, schedule, entry, progress, finished, step,
           save_every, displayiters, debug="", flow_backend=None, prep_backend="host", optimizer="sgd", keep_optimizer_state=False,
           frame_store="off", aug_backend="host"):
    """The loop of both DGP drivers.  schedule() draws the run's entries, entry(data_batcher, e) -> (dataset_i, visible frames, hidden
    frames) of one of them, progress(...) prints a displayed iteration's lines, `finished` is the closing line.  Iteration `it` trains on
    entry _dp_index(it) and rank 0 saves every `save_every` iterations and after the last.  labeled_only: the objective is
    total_loss_visible and the batch is the general one without hidden frames, frame pairs or flow.  prep_backend "hip": the locref
    maps are built on the device (_device_locref) and handed to the loss as Staged tensors instead of two host arrays.  optimizer: "sgd"
    (the reference's MomentumOptimizer) | "adam", both behind clip_by_global_norm(10); keep_optimizer_state as in fit_dlc.
    frame_store "hip": every dataset's selected frames are put on the device before iteration 0 (_frame_stores) and make_batch
    gathers the batch there: the Dataset gives the index sets and labels without pixels, only the labeled frames' host copies go
    through data_aug (the same draws in the same order), and the augmented frames travel as the gather's patch.
    aug_backend "hip": make_batch draws the plans of the labeled frames and moves their labels on the host (augment.plan_aug: data_aug's
    draws in data_aug's order), gets the batch onto the device as it would anyway -- the store's gather, now without a patch for the
    labeled frames, or the upload -- and has engine.augment_frames make the pixels there (_device_augment), on the uploader's stream
    and before the batch's event is recorded."""
    from .. import weights_io
    from .session import Placeholder, TrainSession
    dgp_cfg, nj = data_batcher.dlc_config, data_batcher.nj
    loss, total_loss, total_loss_visible, placeholders = dgp_loss(data_batcher, dgp_cfg)
    pipeline = _aug_pipeline(dgp_cfg, aug_backend)        # before the expensive setup: a broken augmentation stack fails here
    trainer = _make_trainer(data_batcher, init_weights, max_frames=max_frames, device=local_rank)
    if pipeline is not None:
        resolve_aug_backend(aug_backend, trainer.device)
    learning_rate = Placeholder("learning_rate")
    if keep_optimizer_state:
        _restore_optimizer_state(trainer, init_weights, optimizer)
    train_op = loss.graph.minimize(total_loss_visible if labeled_only else total_loss, learning_rate,      # fitdgp.py:412-418, 708-713
                                   optimizer=optimizer)
    sess = TrainSession(trainer, loss.graph)
    saver = weights_io.Saver(max_to_keep=dgp_cfg.max_to_keep)     # fitdgp.py:401, 696
    uploader = _make_uploader(trainer)
    prep_backend = resolve_prep_backend(prep_backend, trainer.device)
    PREP_STATS["backend"], PREP_STATS["frame_store"] = prep_backend, None
    PREP_STATS["aug"] = None if pipeline is None else {"backend": aug_backend, "frames": 0, "stages": {}}
    stores = _frame_stores(data_batcher, trainer.device, uploader) if frame_store == "hip" else None
    entries = schedule()
    n_sched = len(entries)
    maxiters = max(1, n_sched // world)          # data-parallel: W windows per optimiser step
    data_batcher.reset()
    print("Begin Training for {} iterations".format(maxiters))
    t_start = time.time()
    it = -1

    def make_batch(it):                          # host side of one iteration (runs one iteration ahead on the prefetch thread)
        dataset_i, vis_b, hid_b = entry(data_batcher, entries[_dp_index(it, n_sched)])
        d = data_batcher.datasets[dataset_i]
        (vis, hid, _, images, joint_loc, wt_mask, _, addn), _ = data_batcher.next_batch(0, dataset_i, vis_b, hid_b, pixels=stores is None)
        all_frame = np.sort(list(vis) + list(hid))
        vis_within = [int(np.where(all_frame == i)[0][0]) for i in vis]
        replaced, plans = None, None
        if pipeline is not None and dgp_cfg.wt == 0 and len(vis_within) > 0:      # fitdgp.py:481-482, 778-779
            from ..augment import data_aug, plan_aug
            if aug_backend == "hip":                                  # the draws and the labels here, the pixels on the device below
                plans, joint_loc = plan_aug(len(vis), int(d.nx_in), int(d.ny_in), joint_loc, pipeline, dgp_cfg)
            elif stores is None:
                images, joint_loc = data_aug(images, vis_within, joint_loc, pipeline, dgp_cfg)
            else:                                                     # the labeled frames alone: data_aug reads no other
                labeled = np.stack([stores[dataset_i].host[int(i)] for i in vis])
                labeled, joint_loc = data_aug(labeled, list(range(len(vis))), joint_loc, pipeline, dgp_cfg)
                replaced = dict(zip(vis_within, labeled))
            _count_aug(plans if plans is not None else getattr(pipeline, "last_plans", [[]] * len(vis)))
        if prep_backend == "hip":                                     # (after data_aug, which moves joint_loc)
            lmap, lmask = _device_locref(uploader, trainer.device, joint_loc, len(all_frame), vis_within, d.nx_out, d.ny_out, nj, dgp_cfg)
        else:
            lmap, lmask = _locref_targets(joint_loc, len(all_frame), vis_within, d.nx_out, d.ny_out, nj, dgp_cfg)
        vector_field, frames = None, None
        if stores is not None:                                        # the batch is gathered on the device, the flow computed from it
            frames = stores[dataset_i].batch(all_frame, replaced)
            PREP_STATS["frame_store"]["patched"] = stores[dataset_i].last_patched
            if plans is not None:
                frames = _device_augment(uploader, trainer.device, frames.tensor, plans, vis_within)
            images = frames.tensor
            if dgp_cfg.wt > 0:
                frames, vector_field = _flow_of(uploader, images)
        elif dgp_cfg.wt > 0 and flow_backend == "hip":                # temporal clique: flow magnitude on the device
            frames, vector_field = _device_flow(uploader, trainer.device, images)
        elif dgp_cfg.wt > 0:                                          # temporal clique: flow field from the host hook
            from .fitdgp_util import learn_wt
            vector_field = learn_wt(images, backend=flow_backend)
        elif plans is not None:                                       # the batch goes up now, the labeled frames are augmented there
            frames = _device_augment(uploader, trainer.device, images, plans, vis_within)
        feed_dict = _feed(placeholders, images, joint_loc, lmap, lmask, addn, None if labeled_only else wt_mask, vector_field,
                          dgp_cfg.wt, d.nx_out, d.ny_out, learning_rate, dgp_cfg.lr)
        if frames is None and uploader is not None:
            frames = uploader(images)
        if frames is not None:
            feed_dict[placeholders["inputs"]] = frames
        return dataset_i, vis_b, hid_b, feed_dict

    for it, (dataset_i, vis_b, hid_b, feed_dict) in enumerate(_prefetched(make_batch, maxiters)):
        t0 = time.time()
        loss_eval, _ = sess.run([loss, train_op], feed_dict)
        if it % displayiters == 0 and it > 0:
            print("\nIteration {}/{}".format(it, maxiters))
            progress(dataset_i, vis_b, hid_b, t0, loss_eval)
        if (it % save_every == 0) or (it + 1) == maxiters:
            _save(saver, trainer, dgp_cfg.snapshot_prefix, step, it, (it + 1) == maxiters, debug, keep_optimizer_state)
    print(finished.format(it), flush=True)
    print("\n\n TOTAL TIME ELAPSED: ", time.time() - t_start)


def _frame_stores(data_batcher, device, uploader):
    """frame_store="hip": one _FrameStore per Dataset, filled here, sharing staged.FRAME_STORE_BYTES (read now) in dataset order; what
    does not fit is said once.  Every rank of a data-parallel run fills its own.  -> the stores, and PREP_STATS["frame_store"]."""
    from .. import staged
    left, said, stores = staged.FRAME_STORE_BYTES, [], []

    def announce(line):
        if not said:
            said.append(line)
            print(line, flush=True)

    for d in data_batcher.datasets:
        stores.append(_FrameStore(d, device, uploader, budget=left, announce=announce))
        left -= stores[-1].bytes
    PREP_STATS["frame_store"] = {"frames": sum(len(s.slots) for s in stores), "bytes": sum(s.bytes for s in stores),
                                 "refused": sum(len(s.refused) for s in stores), "fill_s": sum(s.fill_s for s in stores), "patched": 0}
    return stores


def _labeled_entry(data_batcher, row):
    """(dataset, labeled frame) -> that frame alone"""
    dataset_i, frame_i = row
    return dataset_i, np.array([frame_i]), np.array([], dtype=int)


def _labeled_progress(dataset_i, vis_b, hid_b, t0, loss_eval):
    print("dataset_i: ", dataset_i, " visible_frame_batch_i: ", [vis_b[0]], flush=True)
    print(" running time: ", time.time() - t0, "\n loss: ", loss_eval, flush=True)


def fit_dgp_labeledonly(snapshot, dlcpath, shuffle=1, step=1, saveiters=1000, displayiters=5, maxiters=50000, ns=10,
                        nc=2048, n_max_frames=2000, aug=True, trainingsetindex=0, frame_sources=None, prep_backend="auto", optimizer="sgd",
                        keep_optimizer_state=False, frame_store="off", aug_backend="host"):
    """Run DGP with labeled frames only (fitdgp.py:257-546): batch = one labeled frame, loss =
    total_loss_visible.  `frame_sources` (new, optional) injects already-open frame sources per video.
    prep_backend: "host" | "hip" | "auto" (resolve_prep_backend): where the locref target maps are built.
    optimizer: "sgd", the reference's hard-coded MomentumOptimizer(lr, 0.9), or "adam", AdamOptimizer(lr); both on gradients clipped to a
    global norm of 10.  keep_optimizer_state: see fit_dlc.
    frame_store: "off" | "hip" (resolve_frame_store).  "hip": the labeled frames are read once, kept on the device (and on the host, for
    the augmentation), and every iteration's frame is gathered there; only an augmented frame is uploaded.
    aug_backend: "host" | "hip" (resolve_aug_backend), with aug=True.  "hip": the augmentation is drawn on the host as a plan
    (augment.NumpyAugPipeline.plan: the same draws in the same order, so the labels and every other feed are the host path's, bit for
    bit) and applied to the frame on the device (engine.augment_frames, csrc/dgp_augment.hip); with a frame store nothing is uploaded.
    Five of the seven stages give the host stages' bytes, elastic is within rounding of float64 like the host's, and the additive
    noise is a different stream from the same distribution as the host's PCG64 ziggurat field."""
    aug_backend = resolve_aug_backend(aug_backend)
    prep_backend = resolve_prep_backend(prep_backend)
    frame_store = resolve_frame_store(frame_store)
    optimizer = resolve_optimizer(optimizer)
    hyper = dict(ws=0, ws_max=1.2, wt=0, wt_max=0, wn_visible=1, wn_hidden=0, gamma=1, gauss_len=1, lengthscale=1,
                 max_to_keep=5, batch_size=1, n_times_all_frames=100, lr=0.005, gm2=0, gm3=0, aug=aug)
    run = _open_project(snapshot, dlcpath, shuffle, trainingsetindex, frame_sources, hyper, "-step1-final--0",
                        "  exists! DGP with labeled frames has already been run.", ns, nc, n_max_frames)
    if run is None:
        return None
    data_batcher = run[0]

    def schedule():                              # `nepoch` uniform draws from the table of every (dataset, labeled frame)
        nepoch = int(np.min([int(data_batcher.n_visible_frames_total * data_batcher.dlc_config.n_times_all_frames), maxiters]))
        table = np.array([(i, vv) for i, d in enumerate(data_batcher.datasets) for vv in d.idxs["pv"]]).reshape(-1, 2)
        return table[np.random.randint(0, table.shape[0], size=nepoch)]

    _train(*run, labeled_only=True, max_frames=1, schedule=schedule, entry=_labeled_entry, progress=_labeled_progress,
           finished="Finished training {} iterations\n", step=step, save_every=saveiters, displayiters=displayiters,
           prep_backend=prep_backend, optimizer=optimizer, keep_optimizer_state=keep_optimizer_state, frame_store=frame_store,
           aug_backend=aug_backend)
    return None


def _window_entry(data_batcher, batch_ind):
    """One window of gen_batch's schedule, [frame, ..., frame, dataset] -> its labeled and its unlabeled frames"""
    dataset_i = int(batch_ind[-1])
    idxs = data_batcher.datasets[dataset_i].idxs
    all_frame_batch = batch_ind[:-1]
    visible_frame_i = idxs["pv"]
    all_frame_i = list(idxs["chunk"]) + list(idxs["ph"])
    vis_b = np.sort(np.array([i for i in all_frame_batch if i in visible_frame_i], dtype=int))
    if len(vis_b) == 0 and len(visible_frame_i) > 0:              # guarantee one labeled frame (fitdgp.py:755-758)
        vis_b = np.array([visible_frame_i[randint(0, len(visible_frame_i) - 1)]])
    hid_b = np.sort(np.array([i for i in all_frame_batch if (i in all_frame_i) and (i not in visible_frame_i)], dtype=int))
    return dataset_i, vis_b, hid_b


def _window_progress(dataset_i, vis_b, hid_b, t0, loss_eval):
    print("dataset_i: ", dataset_i, flush=True)
    print("visible_frame_batch_i: ", vis_b, flush=True)
    print("hidden_frame_batch_i: ", hid_b, flush=True)
    print("\n running time: ", time.time() - t0, flush=True)
    print("\n loss: ", loss_eval, flush=True)


def fit_dgp(snapshot, dlcpath, batch_size=10, shuffle=1, step=2, saveiters=1000, displayiters=5, maxiters=200000, ns=10,
            nc=2048, n_max_frames=2000, gm2=0, gm3=0, nepoch=100, wt=0, aug=True, debug="", trainingsetindex=0,
            frame_sources=None, flow_backend="auto", prep_backend="auto", optimizer="sgd", keep_optimizer_state=False,
            frame_store="off", aug_backend="host"):
    """Run DGP (fitdgp.py:549-845): batches of `batch_size` consecutive frames of the selected windows, at least
    one labeled frame per batch, loss = total_loss (visible + hidden CE, locref, spatial clique; + the temporal clique when wt > 0).
    flow_backend (wt > 0): "cv2" | "hip" | "auto" as learn_wt's backend.  With "hip" the flow magnitude is computed on the device from
    the batch's uploaded frames (engine.optical_flow) and handed to the loss as a device tensor: it never crosses to the host.
    prep_backend: "host" | "hip" | "auto" (resolve_prep_backend): where the locref target maps are built; with "hip" the two
    [nt, H, W, 2 nj] maps are written on the device from the labeled frames' coordinates and never exist on the host.
    optimizer / keep_optimizer_state: as in fit_dgp_labeledonly.
    frame_store: "off" | "hip" (resolve_frame_store).  "hip": the selected frames (idxs chunk, pv, ph of every video) are read from their
    source once, in ascending order, and kept on the device within staged.FRAME_STORE_BYTES; a batch is one engine.gather_frames launch
    over them plus a patch of what was made for it (augmented labeled frames, frames the store could not hold), and with wt > 0 the
    flow is computed from the gathered batch, which needs flow_backend "hip" (a host flow with "hip" is a ValueError).
    aug_backend: as in fit_dgp_labeledonly; with "hip" and a frame store only the frames the store refused are patched.  wt > 0 skips
    the augmentation with either backend, as the reference does."""
    from .fitdgp_util import resolve_flow_backend
    aug_backend = resolve_aug_backend(aug_backend)
    optimizer = resolve_optimizer(optimizer)
    prep_backend = resolve_prep_backend(prep_backend)
    flow_backend = resolve_flow_backend(flow_backend) if wt > 0 else None
    frame_store = resolve_frame_store(frame_store, wt, flow_backend)
    hyper = dict(ws=1000, ws_max=1.2, wt=wt, wt_max=0, wn_visible=5, wn_hidden=3, gamma=1, gauss_len=1, lengthscale=1,
                 max_to_keep=5, batch_size=batch_size, n_times_all_frames=nepoch, lr=0.005, gm2=gm2, gm3=gm3, aug=aug)
    run = _open_project(snapshot, dlcpath, shuffle, trainingsetindex, frame_sources, hyper, "-step{}{}-final--0".format(step, debug),
                        "  exists! DGP has already been run.", ns, nc, n_max_frames)
    if run is None:
        return None
    data_batcher = run[0]
    print("n_hidden_frames_total", data_batcher.n_frames_total - data_batcher.n_visible_frames_total, flush=True)
    print("n_visible_frames_total", data_batcher.n_visible_frames_total, flush=True)
    print("n_frames_total", data_batcher.n_frames_total, flush=True)

    def schedule():                              # gen_batch's windows over every dataset's selected frames
        idxs = [d.idxs for d in data_batcher.datasets]
        return gen_batch([i["pv"] for i in idxs], [i["ph"] for i in idxs], [i["chunk"] for i in idxs], data_batcher.dlc_config,
                         maxiters)

    _train(*run, labeled_only=False, max_frames=batch_size + 1, schedule=schedule, entry=_window_entry, progress=_window_progress,
           finished="Finished {} iterations\n", step=step, save_every=max(int(saveiters / batch_size), 1), displayiters=displayiters,
           debug=debug, flow_backend=flow_backend, prep_backend=prep_backend, optimizer=optimizer,
           keep_optimizer_state=keep_optimizer_state, frame_store=frame_store, aug_backend=aug_backend)
    return None
