"""Drop-in counterparts of deepgraphpose/models/eval.py on the MI355X engine.

Same entry points and signatures as the reference (DGP/models/eval.py):
  setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=False, gauss_len=1, gamma=1)     :147
  estimate_pose(proj_cfg_file, dgp_model_file, video_file, output_dir, shuffle=1, ...)    :217
  export_pose_like_dlc / load_pose_from_dlc_to_dict                                      :621 / :648
  plot_dgp(video_file, output_dir='', ...)                                               :816
The TF session call `sess.run([mu_n, scmap], feed_dict={inputs: frame[None]})` (:328) is served by
`EvalSession.run`, which batches frames through the fused HIP path (dgp_infer); the per-joint likelihood
loop (:331-343) runs inside the soft-argmax kernel.  Video decode and movie rendering are untouched
third-party territory (moviepy) and only used when installed -- except Motion-JPEG .avi files and .jpg frames, which are read
(frames.MjpegAviSource) and decoded (decode_backend: Pillow on the host, or dgp_jpeg_entropy_decode + dgp_jpeg_reconstruct_u8) here,
and plot_dgp's annotated movie, which without moviepy is written as a Motion-JPEG .avi by render.write_annotated_movie (movie_backend).
"""
from __future__ import annotations

import os
import time
from os.path import join
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import yaml

from . import staging


class _Fetch:
    """Symbolic handle standing in for a TF tensor of the eval graph."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<dgp fetch %s>" % self.name


class EvalSession:
    """What `TF.Session` + the restored graph were in the reference: holds the weights and one DGPNet per
    frame size (the TF placeholder was [1, None, None, 3]); `run` accepts the same fetch list."""

    def __init__(self, weights: Dict[str, np.ndarray], depth: int, nj: int, loc_ref: bool, gauss_len, gamma,
                 mean_pixel, max_batch: int = 32, device: int = 0, tier: Optional[str] = None):
        self.weights, self.depth, self.nj, self.loc_ref = weights, depth, nj, loc_ref
        self.tier = resolve_tier(tier)
        self.gauss_len, self.gamma, self.mean_pixel = gauss_len, gamma, tuple(mean_pixel)
        self.max_batch, self.device = max_batch, device
        self._nets = {}
        self.mu_n, self.softmax_tensor = _Fetch("mu_n"), _Fetch("softmax_tensor")
        self.scmap, self.inputs = _Fetch("scmap"), _Fetch("inputs")
        self.locref = _Fetch("locref") if loc_ref else None
        self.likelihood, self.idx = _Fetch("likelihood"), _Fetch("mu_likelihoods")

    def net_for(self, h: int, w: int):
        """The engine at frame size h x w.  ONE net is kept: a new size re-plans the layers (dgp_net_set_input_size) and
        keeps the uploaded, repacked weights -- the TF placeholder was [1, None, None, 3] and accepted any size too."""
        from .. import engine
        net = self._nets.get("net")
        if net is not None and (net.max_batch < self.max_batch or net.device.index != int(self.device)):
            self._nets = {}                        # (a kept session asked for larger batches / another GPU: new engines)
            net = None
        if net is None:
            net = engine.DGPNet(self.depth, self.nj, h, w, max_batch=self.max_batch, with_locref=self.loc_ref,
                                device=self.device, mean_pixel=self.mean_pixel, tier=self.tier)
            net.load_weights(self.weights)
            self._nets["net"] = net
        elif (net.in_h, net.in_w) != (h, w):
            net.set_input_size(h, w)
        return net

    def pipe_for(self, h: int, w: int, n_streams: int = 2):
        """The streaming form of net_for: engine.DGPPipeline (n engines on n HIP streams, batches dealt in turn) whose engine 0 is
        net_for's engine; the further engines load the same weights once."""
        from .. import engine
        net = self.net_for(h, w)
        pipe = self._nets.get("pipe")
        if pipe is None:
            pipe = engine.DGPPipeline(self.depth, self.nj, h, w, max_batch=self.max_batch, with_locref=self.loc_ref,
                                      device=self.device, n_streams=n_streams, mean_pixel=self.mean_pixel, first=net, tier=self.tier)
            for n in pipe.nets[1:]:
                n.load_weights(self.weights)
            self._nets["pipe"] = pipe
        elif (pipe.in_h, pipe.in_w) != (h, w):
            pipe.set_input_size(h, w)
        return pipe

    def run(self, fetches, feed_dict):
        import torch
        from .. import engine
        single = not isinstance(fetches, (list, tuple))
        fl = [fetches] if single else list(fetches)
        frames = feed_dict[self.inputs]
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8:
                # the reference feeds img_as_ubyte frames cast to fp32 (eval.py:326-328): integral 0..255
                frames = np.clip(np.rint(frames), 0, 255).astype(np.uint8)
            frames = torch.from_numpy(np.require(frames, requirements=["C", "W"])).cuda(self.device)      # (read-only memmaps: copy)
        B, h, w, _ = frames.shape
        net = self.net_for(h, w)
        names = {f.name for f in fl}
        out = {}
        for s in range(0, B, self.max_batch):
            fb = frames[s:s + self.max_batch].contiguous()
            if self.loc_ref and "locref" in names:
                scm, loc = net.forward(fb, want_locref=True)
            else:
                scm, loc = net.forward(fb), None
            part = {"scmap": scm, "locref": loc}
            if names & {"mu_n", "softmax_tensor", "likelihood", "mu_likelihoods"}:
                mu, conf, idx, pmap = engine.soft_argmax(scm, self.gamma, self.gauss_len, want_pmap=True)
                part.update(mu_n=mu, softmax_tensor=pmap, likelihood=conf, mu_likelihoods=idx)
            for k, v in part.items():
                if k in names:
                    out.setdefault(k, []).append(v.cpu().numpy())
        res = [np.concatenate(out[f.name], 0) for f in fl]
        return res[0] if single else res

    def close(self):
        """tf.Session.close(): drops the engines -- unless this is the session kept for the next call on the same snapshot
        (setup_dgp_eval_graph; clear_session_cache() frees it)"""
        if _SESSION_CACHE.get("sess") is not self:
            self._nets = {}


def resolve_tier(tier: Optional[str] = None) -> Optional[str]:
    """The arithmetic tier of an entry point: the `tier` argument, else the environment's DGP_EVAL_TIER, else None = the library's
    default (the parity tier: 1e-3 px / bit-exact indices).  "f16" = the 16-bit tier (2-byte activation cells, one MFMA per product,
    ~2 x the frames/s): a REPORTED tier with measured error, never what parity claims are made on."""
    t = tier if tier is not None else (os.environ.get("DGP_EVAL_TIER") or None)
    if t is None:
        return None
    t = str(t).lower()
    if t in ("bf16", "fp16", "half", "16", "h1"):
        t = "f16"
    if t not in ("parity", "f32x", "f16"):
        raise ValueError("tier must be 'parity' or 'f16' (got %r)" % (tier if tier is not None else os.environ.get("DGP_EVAL_TIER"),))
    return t


def setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=False, gauss_len=1, gamma=1, tier=None):
    """-> (sess, mu_n, softmax_tensor, scmap, locref, inputs), as eval.py:147-214.  `tier` is new (resolve_tier): None / "parity" / "f16".

    `dgp_model_file` is what Saver.restore takes (eval.py:194-211): the prefix of a TF V2 bundle (`<prefix>.index` +
    `.data-*`, written by the reference or by this package's fit drivers), a V1 `.ckpt` file, or an .npz / .safetensors
    file with TF variable names; optimiser slots and non-float variables (global_step) in a checkpoint are skipped;
    a missing file raises FileNotFoundError, a net_type that does not match the snapshot raises
    KeyError (the reference relies on exactly that failure to fall back from resnet_50 to resnet_101)."""
    from .. import weights_io
    depth = int(str(dlc_cfg.net_type).split("_")[-1])
    mean_pixel = dlc_cfg.get("mean_pixel", [123.68, 116.779, 103.939])
    # One session is kept between calls (run_dgp_demo / plot_dgp label a project's videos one after the other with ONE snapshot: the
    # reference restored the graph for every video): same snapshot files (path, size, mtime), same graph arguments -> the engines with
    # their uploaded, re-packed weights are reused; activation scales are calibrated again on every video's first batch.
    key = None
    if os.environ.get("DGP_EVAL_SESSION_CACHE", "1") != "0":
        try:
            f = weights_io.resolve(str(dgp_model_file))
            stamp = tuple((q, os.path.getsize(q), os.stat(q).st_mtime_ns) for q in sorted(_snapshot_files(f)))
            key = (stamp, depth, int(dlc_cfg.num_joints), bool(loc_ref), gauss_len, gamma, tuple(float(v) for v in mean_pixel), resolve_tier(tier))
        except OSError:
            key = None
    if key is not None and _SESSION_CACHE.get("key") == key:
        sess = _SESSION_CACHE["sess"]
        return sess, sess.mu_n, sess.softmax_tensor, sess.scmap, sess.locref, sess.inputs
    weights = weights_io.load_weights(str(dgp_model_file))
    if ("resnet_v1_%d/conv1/weights" % depth) not in weights:
        raise KeyError("snapshot %s holds no resnet_v1_%d variables" % (dgp_model_file, depth))
    sess = EvalSession(weights, depth, int(dlc_cfg.num_joints), bool(loc_ref), gauss_len, gamma, mean_pixel, tier=tier)
    if key is not None:
        clear_session_cache()
        _SESSION_CACHE.update(key=key, sess=sess)
    return sess, sess.mu_n, sess.softmax_tensor, sess.scmap, sess.locref, sess.inputs


_SESSION_CACHE: Dict[str, object] = {}


def _snapshot_files(resolved: str):
    """the files a snapshot consists of: a V2 bundle's .index + .data-* shards, or the single file"""
    import glob
    if resolved.endswith(".index"):
        return [resolved] + glob.glob(resolved[:-len(".index")] + ".data-*")
    return [resolved]


def clear_session_cache():
    """Drop the engines kept for the next call on the same snapshot (frees their device memory)."""
    old = _SESSION_CACHE.pop("sess", None)
    _SESSION_CACHE.pop("key", None)
    if old is not None:
        old._nets = {}


# counters of the last estimate_pose call (tests, soak runs): chunks processed and chunks re-run after a range overflow
RUN_STATS = {"chunks": 0, "chunk_reruns": 0, "strict_passes": 0, "stage_s": 0.0, "wait_frames_s": 0.0, "wait_h2d_s": 0.0, "drain_s": 0.0,
             "setup_s": 0.0, "alloc_s": 0.0, "calibrate_s": 0.0, "finish_s": 0.0, "prep_backend": "none", "loc_ref": None,
             "decode_backend": "host", "movie_backend": None}      # movie_backend: plot_dgp's ("moviepy" | "hip" | "host", None = skipped)

# location refinement of estimate_pose / plot_dgp (engine.LOC_REF_MODES): None = the reference's video path (soft-argmax only), "dgp" =
# soft-argmax + the softmax-weighted locref offset, "dlc" = DLC's hard arg-max + the offset at that cell
LOC_REF_CHOICES = (None, "dgp", "dlc")
LOCREF_VARIABLE = "pose/locref_pred/block4/weights"


def refined_pose(records, stride, locref_stdev, scale_x=1.0, scale_y=1.0):
    """Pixel coordinates from 7-lane read-out records [..., 7] = (row, col, likelihood, iy, ix, dx, dy) (engine.DGPNet.infer_packed with
    loc_ref; "dlc" records carry the arg-max cell in lanes 0..1): -> (x, y, likelihood), float64,

        x = (col * stride + stride / 2 + dx * locref_stdev) * scale_x
        y = (row * stride + stride / 2 + dy * locref_stdev) * scale_y.

    This is DLC's geometry (PET/nnet/predict.py:62-77) and the one the locref targets are built in: channel 2j of the head is joint j's x
    offset, 2j + 1 its y offset (compute_target_part_scoremap).  The reference's experimental loc_ref_calc='dgp' branch of evaluate_dgp
    (DGP/models/eval.py:769-780; soft_argmax_locref_pose here) adds channel 2j to the ROW instead; evaluate_dgp keeps that branch as it
    is, the video path does not copy it."""
    r = np.asarray(records, dtype=np.float64)
    if r.shape[-1] != 7:
        raise ValueError("refined_pose: records have %d lanes, not 7" % r.shape[-1])
    x = (r[..., 1] * stride + 0.5 * stride + r[..., 5] * locref_stdev) * scale_x
    y = (r[..., 0] * stride + 0.5 * stride + r[..., 6] * locref_stdev) * scale_y
    return x, y, r[..., 2].copy()

# who resizes / crops the frames of estimate_pose(new_size=, crop_size=): "hip" = engine.resize_frames on the copy stream (source-size
# frames cross PCIe), "pil" = Pillow per frame on the host (the reference's code), "auto" = "hip" unless the kernel refuses the shape
RESIZE_BACKENDS = ("auto", "pil", "hip")

# who decodes the frames of a source that holds baseline JPEG streams (frames.MjpegAviSource, a directory of .jpg files): "host" = the
# source's frame_at / iter_frames (Pillow; one thread), "hip" = DECODE_THREADS host threads Huffman-decode whole batches into pinned
# coefficient slots (staging.stage_jpeg) and engine.jpeg_reconstruct rebuilds the pixels on the copy stream -- the same bytes --, "auto" =
# "hip" when the source offers jpeg_bytes and dgp_jpeg_probe takes its first frame, else "host" (with one printed line for a source
# that decodes at all; an in-memory stack has nothing to decode and stays silent)
DECODE_BACKENDS = ("auto", "host", "hip")
# host threads of the "hip" decode path (at most 16).  Measured (profiles/jpeg_bench_line.json, 640x480 at quality 90): one thread
# entropy-decodes 3130 frames/s, 8 threads 21 900 (7.0 x) -- 4.7 x what the parity engines take and 2.3 x the 16-bit tier's, with half of a
# rank's 16 CPUs left to the staging consumer and the other ranks' threads; idle decoders wait on the ring and cost nothing
DECODE_THREADS = 8

# The host pipeline's geometry (measured settings, not run-time switches; tests patch the module attributes): engines / HIP streams the
# batches are dealt to, pinned staging slots, host threads staging an in-memory stack, copy streams the uploads alternate on, bytes of
# frames a chunk keeps resident for a re-run after a range overflow.
EVAL_STREAMS, PINNED_SLOTS, STAGE_THREADS, COPY_STREAMS, CHUNK_BYTES = 2, 8, 2, 2, 1 << 30

# pinned staging ring, kept between calls (pinning host memory costs ~ 10 ms per 30-MB buffer; a project's videos share one frame size)
_PINNED = {"key": None, "bufs": []}


def _pinned_ring(nslots: int, shape, dtype=None):
    import torch
    dtype = dtype or torch.uint8
    key = (nslots, tuple(shape)) if dtype == torch.uint8 else (nslots, tuple(shape), dtype)
    if _PINNED["key"] != key:
        _PINNED["bufs"] = []                       # (drop the old ring first)
        _PINNED["bufs"] = [torch.empty(shape, dtype=dtype).pin_memory() for _ in range(nslots)]
        _PINNED["key"] = key
    return _PINNED["bufs"]


class _PoseRun:
    """estimate_pose's state for one video on one rank, and the steps of a pass over the rank's frames [lo, hi).

    Host pipeline: host threads fill a ring of pinned staging buffers (models/staging.py: an in-memory stack is
    staged by STAGE_THREADS threads, ONE GIL-free copy per batch; a decoder is sequential and keeps one thread), copy streams move
    batch k+1 to the GPU while batch k runs through dgp_infer on the compute stream, and the keypoints of the whole video come back in
    ONE device-to-host copy at the end (the reference fetched the full scoremap every frame)."""

    def __init__(self, sess, clip, video_file, lo, hi, world, batch_size, new_size, crop_size, resize_backend, loc_ref=None,
                 decode_backend="host"):
        self.sess, self.clip, self.video_file, self.loc_ref = sess, clip, video_file, loc_ref
        self.decode_backend, self.decode, self.jpeg_info = decode_backend, None, None      # decode: "host" | "hip", decided on the first frame
        self.lanes = 5 if loc_ref is None else 7          # fp32 lanes of a (frame, joint) record (engine.record_lanes)
        self.records = None                               # loc_ref: the whole video's 7-lane records, float32 [n_frames, nj, 7]
        self.lo, self.hi, self.world, self.n_frames, self.batch_size = lo, hi, world, int(clip.n_frames), batch_size
        self.new_size, self.crop_size, self.resize_backend = new_size, crop_size, resize_backend
        resizing = new_size is not None or crop_size is not None
        self.prep_backend = "pil" if resizing and resize_backend == "pil" else None if resizing else "none"      # None: decided on the first frame
        self.scale_x = self.scale_y = 1
        self.markers = np.zeros((self.n_frames, sess.nj, 2))
        self.likelihoods = np.zeros((self.n_frames, sess.nj))

    def choose_prep_backend(self, first):
        """"hip" when dgp_resize_crop_u8 takes the video's frames (tried on the first one, which also uploads the tables)"""
        import torch
        from .. import engine, _lib
        try:
            if first.dtype != np.uint8 or first.ndim != 3 or first.shape[2] != 3:
                raise _lib.DgpError("frames are %s %s, not uint8 RGB" % (first.dtype, first.shape))
            engine.resize_frames(torch.from_numpy(np.ascontiguousarray(first[None])).to(self.dev), self.new_size, self.crop_size)
        except _lib.DgpError as e:
            if self.resize_backend == "hip":
                raise
            print("resize_backend auto: frames of %s are resized with Pillow on the host (%s)" % (self.video_file, e), flush=True)
            return "pil"
        return "hip"

    def choose_decode_backend(self):
        """"hip" when the source hands out JPEG streams, dgp_jpeg_probe takes the first one and no host resize stands between the decoder
        and the engines; decode_backend "hip" raises ValueError otherwise, "auto" says why in one line and decodes on the host"""
        from .. import jpeg, _lib
        if self.decode_backend == "host":
            return "host"
        clip, why = self.clip, None
        if not callable(getattr(clip, "jpeg_bytes", None)):
            why = "the source holds no JPEG streams"
        elif not getattr(clip, "jpeg_only", True):
            why = "not every frame of the source is a .jpg file"
        elif self.prep_backend == "pil":
            why = "the frames are resized with Pillow on the host"
        else:
            try:
                data = clip.jpeg_bytes(0)
                if data is None:
                    why = "the first frame is not a JPEG file"
                else:
                    self.jpeg_info = jpeg.probe(data)
            except _lib.DgpError as e:
                why = str(e)
        if why is None:
            return "hip"
        if self.decode_backend == "hip":
            raise ValueError("estimate_pose: decode_backend 'hip' cannot decode %s: %s" % (self.video_file, why))
        if not hasattr(clip, "frames"):                # (an in-memory stack decodes nothing: no line)
            print("decode_backend auto: frames of %s are decoded on the host (%s)" % (self.video_file, why), flush=True)
        return "host"

    def prep(self, frame):
        """the frame as it is staged: the reference's PIL resize / crop (eval.py:307-326) on the "pil" backend, else the source frame"""
        if self.prep_backend != "pil":
            return np.asarray(frame)
        from PIL import Image
        im = Image.fromarray(frame)
        if self.new_size is not None:
            im = im.resize(size=(self.new_size[1], self.new_size[0]))
        if self.crop_size is not None:
            im = im.crop(self.crop_size)
        return np.asarray(im)

    def allocate(self, sh, sw):
        """The engines, the pinned ring and the device buffers of a pass whose staged frames are sh x sw: dchunk keeps the frames of a
        CHUNK of batches (staging.chunk_plan) on the device until the chunk's range check has come back clean -- a chunk whose activations
        outgrew the calibrated H2 scales is re-run from HBM, without decoding anything again."""
        import torch
        from .. import engine
        B, dev = self.batch_size, self.dev
        self.on_gpu = self.prep_backend == "hip"       # source-size frames are staged and uploaded, engine.resize_frames fills dchunk
        hh, ww = engine.resize_output_shape(sh, sw, self.new_size, self.crop_size) if self.on_gpu else (sh, sw)      # the network's frame size
        t_ = time.perf_counter()
        self.net = self.sess.pipe_for(hh, ww, n_streams=EVAL_STREAMS)      # two engines on two HIP streams, batches dealt in turn
        torch.cuda.synchronize(dev)
        RUN_STATS["setup_s"] += time.perf_counter() - t_      # the engines of this frame size: weights re-packed and uploaded (first call of a size)
        t_ = time.perf_counter()
        if self.decode == "hip":
            # a slot holds a batch's quantised coefficients (int16 [B][total_blocks * 64]) followed by its tables (uint16 [B][ncomp * 64]);
            # one device copy of it per copy stream: the upload lands there and jpeg_reconstruct behind it, on the same stream, writes the pixels
            ji = self.jpeg_info
            if (ji.height, ji.width) != (sh, sw):
                raise ValueError("the first JPEG of %s is %d x %d, its decoded frame %d x %d" % (self.video_file, ji.width, ji.height, sw, sh))
            self.coef_elems, self.qt_elems = ji.total_blocks * 64, ji.ncomp * 64
            self.pinned = _pinned_ring(PINNED_SLOTS, (B * (self.coef_elems + self.qt_elems),), torch.int16)
            self.dcoef = [torch.empty((B * (self.coef_elems + self.qt_elems),), dtype=torch.int16, device=dev) for _ in range(COPY_STREAMS)]
        else:
            self.pinned = _pinned_ring(PINNED_SLOTS, (B, sh, sw, 3))      # batches being staged / copied + slack for bursts
        self.chunk_batches, self.n_rounds = staging.chunk_plan(self.n_frames, self.world, B, B * hh * ww * 3,
                                                               int(os.environ.get("DGP_EVAL_CHUNK_BATCHES", "64")), CHUNK_BYTES)
        self.dchunk = torch.empty((self.chunk_batches, B, hh, ww, 3), dtype=torch.uint8, device=dev)
        # one source-size batch per copy stream: the upload lands here and the resize kernel behind it, on the same stream, fills dchunk
        self.dsrc = [torch.empty((B, sh, sw, 3), dtype=torch.uint8, device=dev) for _ in range(COPY_STREAMS)] if self.on_gpu else []
        RUN_STATS["alloc_s"] += time.perf_counter() - t_        # pinned ring (kept between calls) + the chunk's device buffer
        self.copy_streams = [torch.cuda.Stream(device=dev) for _ in range(COPY_STREAMS)]
        self.compute = torch.cuda.current_stream(dev)
        self.traj = torch.zeros((max(self.hi - self.lo, 1), self.sess.nj, self.lanes), dtype=torch.float32, device=dev)      # packed (row, col, likelihood, iy, ix[, dx, dy])

    def calibrate_on_first_batch(self):
        """Calibration: every engine of every rank calibrates its activation scales on the video's FIRST batch (not on its own shard's),
        so the frozen scales -- and with them every output bit -- are those of a single-process run.  Sharded runs of a seekable source
        do it here; a single process finds the video's first batch first in its ring, and upload_and_submit calibrates on that (as does
        a sharded run of a source that cannot seek -- on its own shard's first batch)."""
        import torch
        from .. import engine
        nb0 = min(self.batch_size, self.n_frames)
        if self.decode == "hip":                   # (the ring holds coefficients; frame_at gives the same bytes the device decoder will)
            self.cal_batch = torch.from_numpy(np.stack([np.asarray(self.clip.frame_at(t)) for t in range(nb0)])).to(self.dev)
        else:
            for t in range(nb0):
                np.copyto(self.pinned[0][t].numpy(), self.prep(self.clip.frame_at(t)))
            self.cal_batch = self.pinned[0][:nb0].to(self.dev)
        if self.on_gpu:
            self.cal_batch = engine.resize_frames(self.cal_batch, self.new_size, self.crop_size)
        self.net.calibrate(self.cal_batch, self.sess.gamma, self.sess.gauss_len, self.loc_ref)
        torch.cuda.synchronize(self.dev)

    def start_staging(self, f0, rest):
        """the ring over the pinned buffers and the started threads that fill it with this shard's batches"""
        import itertools
        import threading
        B, clip = self.batch_size, self.clip
        if self.decode == "hip":                   # whole batches, dealt to DECODE_THREADS Huffman decoders as stage_stack deals its copies
            nc = B * self.coef_elems
            self.ring = ring = staging.StagingRing([(p.numpy()[:nc].reshape(B, self.coef_elems),
                                                     p.numpy()[nc:].view(np.uint16).reshape(B, self.qt_elems)) for p in self.pinned])
            ring.set_total(-(-(self.hi - self.lo) // B))
            n_thr = max(1, min(int(DECODE_THREADS), 16))
            threads = [threading.Thread(target=staging.stage_jpeg, daemon=True,
                                        args=(ring, clip, self.jpeg_info, self.lo, self.hi, B, t, n_thr, self.video_file)) for t in range(n_thr)]
            for th in threads:
                th.start()
            return threads
        self.ring = ring = staging.StagingRing([p.numpy() for p in self.pinned])
        if self.prep_backend != "pil" and hasattr(clip, "iter_batches") and hasattr(clip, "frames"):      # an in-memory stack: whole batches
            ring.set_total(-(-(self.hi - self.lo) // B))
            threads = [threading.Thread(target=staging.stage_stack, args=(ring, clip.frames, self.lo, self.hi, B, t, STAGE_THREADS), daemon=True)
                       for t in range(STAGE_THREADS)]
        else:
            frames = itertools.chain([f0], (self.prep(x) for x in rest))
            threads = [threading.Thread(target=staging.stage_decoded, args=(ring, frames, self.hi - self.lo, B), daemon=True)]
        for th in threads:
            th.start()
        return threads

    def release(self, block):
        """Slot return: a pinned slot goes back to the ring only after its H2D event has completed, without the host waiting for every
        copy; block: wait for the oldest copy when none has completed"""
        freed = 0
        while self.pending and self.pending[0][0].query():
            freed += 1
            self.ring.give_back(self.pending.pop(0)[1])
        if block and not freed and self.pending:
            t_ = time.perf_counter()
            self.pending[0][0].synchronize()
            RUN_STATS["wait_h2d_s"] += time.perf_counter() - t_
            self.release(False)

    def next_batch(self, k):
        """(slot, frames) of batch k, or None when the shard has no batch k"""
        t_ = time.perf_counter()
        try:
            return self.ring.get(k, lambda: self.release(True))
        finally:
            RUN_STATS["wait_frames_s"] += time.perf_counter() - t_

    def upload_and_submit(self, kb, slot, nb, k, start):
        """Batch number kb (1-based) of the shard, staged in pinned[slot]: into dchunk[k], through the engines, records to traj[start:].
        Stream roles: the upload and its resize run on copy stream kb % COPY_STREAMS, and the compute stream waits on that event."""
        import torch
        from .. import engine
        net, sess, dst = self.net, self.sess, self.dchunk[k][:nb]
        cs = self.copy_streams[kb % len(self.copy_streams)]
        with torch.cuda.stream(cs):
            if self.decode == "hip":
                # (this stream's device slot: the next upload into it queues behind this reconstruct)
                ji, h, d = self.jpeg_info, self.pinned[slot], self.dcoef[kb % len(self.copy_streams)]
                nc, q0 = nb * self.coef_elems, self.batch_size * self.coef_elems
                d[:nc].copy_(h[:nc], non_blocking=True)
                d[q0:q0 + nb * self.qt_elems].copy_(h[q0:q0 + nb * self.qt_elems], non_blocking=True)
                px = self.dsrc[kb % len(self.copy_streams)][:nb] if self.on_gpu else dst
                engine.jpeg_reconstruct(d[:nc].view(nb, ji.total_blocks, 64), d[q0:q0 + nb * self.qt_elems].view(nb, ji.ncomp, 64),
                                        ji.height, ji.width, ji.sampling, out=px)
                if self.on_gpu:
                    engine.resize_frames(px, self.new_size, self.crop_size, out=dst)
            elif self.on_gpu:
                src = self.dsrc[kb % len(self.copy_streams)]      # (this stream's: the next upload into it queues behind this resize)
                src[:nb].copy_(self.pinned[slot][:nb], non_blocking=True)
                engine.resize_frames(src[:nb], self.new_size, self.crop_size, out=dst)
            else:
                dst.copy_(self.pinned[slot][:nb], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(cs)
        self.compute.wait_event(copied)
        self.pending.append((copied, slot))
        if self.cal_batch is None:
            self.cal_batch = dst.clone()
            t_ = time.perf_counter()
            net.calibrate(self.cal_batch, sess.gamma, sess.gauss_len, self.loc_ref)      # (what the first submit would do: timed apart)
            RUN_STATS["calibrate_s"] += time.perf_counter() - t_
        net.submit(dst, self.traj[start:start + nb], sess.gamma, sess.gauss_len, self.loc_ref)      # written in place by the soft-argmax kernel, on the next engine's stream
        # the consumer blocks on its oldest pending copy once it holds all slots but one
        self.release(len(self.pending) >= len(self.pinned) - 1)

    def settle_chunk(self, entries, end, strict):
        """Settle loop, on every rank every round; -> True when the scales were widened.  H2 activation scales (include/dgp_hip.h): a batch
        that outgrew the scales calibrated on the first batch invalidates the results since the last clean check, i.e. THIS chunk's
        (`entries`: (slot in dchunk, frames, offset in traj), ending at shard frame `end`).  All ranks decide together (any_rank, once per
        attempt; the fifth failure raises); every engine of every rank then re-calibrates on the calibration batch with 3 more bits of
        headroom (same scales everywhere again -- a rank that did not overflow widens first, to follow the one that did) and the ranks
        whose chunk overflowed re-run it from the frames still resident in HBM; strict: every rank re-runs it on the new scales."""
        import torch
        from .. import dist as ddist
        net, sess = self.net, self.sess
        widened = False
        for attempt in range(5):
            t_ = time.perf_counter()
            net.join()
            torch.cuda.synchronize(self.dev)
            RUN_STATS["drain_s"] += time.perf_counter() - t_
            overflow = bool(net.range_status()[0])
            if not ddist.any_rank(overflow, device="cuda:%d" % sess.device):
                break
            if attempt == 4:
                raise RuntimeError("activation scales did not settle after 4 re-calibrations in %s" % self.video_file)
            if not overflow:
                net.widen()
            net.calibrate(self.cal_batch, sess.gamma, sess.gauss_len, self.loc_ref)
            widened = True
            if overflow or strict:
                print("activation ranges outgrew the calibrated scales: re-calibrated, re-running frames %d-%d of %s"
                      % (self.lo + entries[0][2] if entries else self.lo, self.lo + end, self.video_file), flush=True)
                RUN_STATS["chunk_reruns"] += 1
                for k, nb, off in entries:
                    net.submit(self.dchunk[k][:nb], self.traj[off:off + nb], sess.gamma, sess.gauss_len, self.loc_ref)
        return widened

    def gather(self, n_done):
        """the trajectory into markers / likelihoods: ONE all-gather per video when sharded (20 bytes per (frame, joint)), ONE device-to-host copy"""
        from .. import dist as ddist
        t_ = time.perf_counter()
        if self.world > 1:
            rec = ddist.gather_trajectory(self.traj[:self.hi - self.lo], self.n_frames)
            n_done = self.n_frames
        else:
            rec = self.traj[:n_done]
        mu_t, lik_t, _ = ddist.unpack_keypoints(rec)
        self.markers[:n_done] = mu_t.cpu().numpy()
        self.likelihoods[:n_done] = lik_t.cpu().numpy()
        if self.loc_ref is not None:                 # refined_pose composes the coordinates from the whole records
            self.records = np.zeros((self.n_frames, self.sess.nj, 7), dtype=np.float32)
            self.records[:n_done] = rec.cpu().numpy()
        RUN_STATS["finish_s"] += time.perf_counter() - t_

    def run_pass(self, first_pass):
        """One pass over the shard; -> True when an earlier chunk holds results of narrower scales than the video ended with."""
        import torch
        self.dev = torch.device("cuda", self.sess.device)
        first, rest = staging.shard_frames(self.clip, self.lo, self.hi, self.world, self.video_file)
        first = np.asarray(first)
        if self.new_size is not None:                  # (all frames of a video have one size)
            self.scale_x, self.scale_y = first.shape[1] / self.new_size[1], first.shape[0] / self.new_size[0]
        if self.prep_backend is None:
            self.prep_backend = self.choose_prep_backend(first)
        if self.decode is None:
            self.decode = self.choose_decode_backend()
        f0 = self.prep(first)
        self.allocate(*f0.shape[:2])
        if first_pass:
            self.net.reset_scales()               # engines kept from an earlier video: THIS video's first batch sets the scales, on the default
                                                  # headroom -- the same bits as a fresh session (a strict re-pass keeps the widened scales)
        self.cal_batch = None                     # the batch every engine (and every rank) calibrates its activation scales on
        if self.world > 1 and hasattr(self.clip, "frame_at"):
            self.calibrate_on_first_batch()
        strict = os.environ.get("DGP_EVAL_STRICT", "0") == "1"
        threads = self.start_staging(f0, rest)
        self.pending = []                         # (H2D-complete event, pinned slot) of the uploads in flight, oldest first
        stale = False
        try:
            start, finished, kb = 0, False, 0
            # Chunk rounds: every rank runs the SAME number (a short shard ends with empty ones), because the decision to re-calibrate
            # after a range overflow is a collective
            for rnd in range(self.n_rounds):
                entries = []
                while len(entries) < self.chunk_batches and not finished:
                    item = self.next_batch(kb)
                    if item is None:
                        finished = True
                        break
                    kb += 1
                    self.upload_and_submit(kb, item[0], item[1], len(entries), start)
                    entries.append((len(entries), item[1], start))
                    start += item[1]
                if self.settle_chunk(entries, start, strict) and rnd > 0:
                    stale = True                  # chunks [0, rnd) were computed with the narrower scales (valid, but other bits)
                RUN_STATS["chunks"] += 1 if entries else 0
            if not finished:
                assert self.next_batch(kb) is None, "more frames than the shard holds"
            while self.pending:
                self.release(True)
            for th in threads:
                th.join()
        except BaseException as e:               # Error handling: a failure on this side must not leave the staging threads waiting for a slot for ever
            self.ring.fail(e)
            raise
        RUN_STATS["stage_s"] += self.ring.stage_s
        self.gather(start)
        return stale


def estimate_pose(proj_cfg_file, dgp_model_file, video_file, output_dir, shuffle=1, save_pose=True, save_str="",
                  new_size=None, crop_size=None, batch_size: int = 32, tier: Optional[str] = None, resize_backend: str = "auto",
                  loc_ref: Optional[str] = None, decode_backend: str = "auto"):
    """Estimate pose on an arbitrary video (eval.py:217-372).  Returns {'x','y','likelihoods'} [T,nj] float64,
    or the csv path if labels already exist (:247-249).  `batch_size` is new: frames go through the GPU in
    batches instead of one sess.run per frame.  `tier` is new (resolve_tier): None = DGP_EVAL_TIER or the parity tier; "f16" = the
    16-bit tier (reported error band, ~2 x the frames/s).  `resize_backend` is new (RESIZE_BACKENDS): who runs the reference's per-frame
    PIL resize / crop of eval.py:307-326 when `new_size` / `crop_size` are given -- "hip": engine.resize_frames (Pillow's bytes, computed on
    the GPU behind the upload of the source-size frames), "pil": Pillow on the host, "auto": "hip", and "pil" (with one printed line) only
    for a shape the kernel refuses or frames that are not uint8 RGB.  RUN_STATS["prep_backend"] names the one that ran ("none": no resize).
    `loc_ref` is new (LOC_REF_CHOICES): location refinement with the snapshot's trained pose/locref_pred head, which the reference's
    video path never applied (DLC's own always does).  None: as the reference.  "dgp": soft-argmax position + the softmax-weighted
    offset, likelihood = the window sigmoid; "dlc": hard arg-max cell + the offset at that cell, likelihood = the arg-max probability
    (PET/nnet/predict.py:62-77).  Coordinates are composed by refined_pose (DLC's axis convention).  A snapshot without the head raises
    KeyError naming the variable.  RUN_STATS["loc_ref"] names the mode that ran.
    `decode_backend` is new (DECODE_BACKENDS): who decodes a source of baseline JPEG streams (a Motion-JPEG .avi, a directory of .jpg
    files) -- "host": the source's own Pillow decode, one thread; "hip": DECODE_THREADS threads Huffman-decode batches and
    engine.jpeg_reconstruct rebuilds the pixels on the GPU, the same bytes (ValueError for a source without JPEG streams or a first frame
    the decoder refuses); "auto": "hip" where that works, else "host" with one printed line.  RUN_STATS["decode_backend"] names the one
    that ran.

    Multi-GPU: under torchrun (one process per GPU; RANK / WORLD_SIZE / LOCAL_RANK in the environment, or an
    already initialised torch.distributed group) rank r decodes and infers only the contiguous frame block
    shard_range(T, r, W), ONE RCCL all-gather of the packed keypoints reassembles the [T, nj] trajectory on every rank, and rank 0
    writes the csv / h5.  Every rank returns the full label dict."""
    from ..config import get_train_config
    from ..frames import open_frame_source
    from .. import dist as ddist
    import torch.distributed as tdist
    t_entry = time.perf_counter()
    if resize_backend not in RESIZE_BACKENDS:
        raise ValueError("estimate_pose: resize_backend must be one of %s, not %r" % ("|".join(RESIZE_BACKENDS), resize_backend))
    if loc_ref not in LOC_REF_CHOICES:
        raise ValueError("estimate_pose: loc_ref must be None, 'dgp' or 'dlc', not %r" % (loc_ref,))
    if decode_backend not in DECODE_BACKENDS:
        raise ValueError("estimate_pose: decode_backend must be one of %s, not %r" % ("|".join(DECODE_BACKENDS), decode_backend))
    RUN_STATS.update(chunks=0, chunk_reruns=0, strict_passes=0, stage_s=0.0, wait_frames_s=0.0, wait_h2d_s=0.0, drain_s=0.0, setup_s=0.0,
                     alloc_s=0.0, calibrate_s=0.0, finish_s=0.0, loc_ref=loc_ref)

    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not tdist.is_initialized():
        ddist.init_from_env()                      # before anything touches the GPU
    world = tdist.get_world_size() if tdist.is_initialized() else 1
    rank = tdist.get_rank() if tdist.is_initialized() else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0
    if world > 1:          # the decode / staging threads started below inherit the mask: each rank's host work stays on its GPU's NUMA node
        ddist.bind_to_gpu_numa_node(local_rank)

    f = os.path.basename(str(video_file)).rsplit(".", 1)
    save_file = join(output_dir, f[0] + "_labeled%s" % save_str)
    if ddist.from_rank0(os.path.exists(save_file + ".csv")):      # rank 0 decides for everyone: a per-rank test could diverge and leave
        print("labels already exist! video at %s will not be processed" % video_file)      # some ranks alone in the collectives below
        return save_file + ".csv"

    video_clip = open_frame_source(video_file)
    with open(proj_cfg_file, "r") as stream:
        proj_config = yaml.safe_load(stream)
    proj_config["video_path"] = None
    dlc_cfg = get_train_config(proj_config, shuffle=shuffle)
    with_head = loc_ref is not None
    try:
        dlc_cfg.net_type = "resnet_50"
        sess = setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=with_head, tier=tier)[0]
    except KeyError:
        dlc_cfg.net_type = "resnet_101"
        sess = setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=with_head, tier=tier)[0]
    if with_head and LOCREF_VARIABLE not in sess.weights:      # (checked after the depth is settled: not a reason to try ResNet-101)
        sess.close()
        video_clip.close()
        raise KeyError("snapshot %s holds no %s: estimate_pose(loc_ref=%r) needs a model trained with location refinement"
                       % (dgp_model_file, LOCREF_VARIABLE, loc_ref))
    sess.max_batch = int(batch_size)
    sess.device = local_rank
    lo, hi = ddist.shard_range(int(video_clip.n_frames), rank, world)        # this rank's frames
    run = _PoseRun(sess, video_clip, video_file, lo, hi, world, batch_size, new_size, crop_size, resize_backend, loc_ref, decode_backend)

    # Bit-identity of a sharded run with a single-process run holds as long as no chunk overflows (or only the first one does).  After an
    # overflow in a LATER chunk the earlier chunks keep the (valid) results of the narrower scales, which a run that started with the
    # wide scales would not reproduce bit for bit.  DGP_EVAL_STRICT=1 restores the guarantee at the cost of a second pass over the video:
    # the engines keep the widened headroom and everything is computed again on those scales (the decision is collective).
    RUN_STATS["setup_s"] = time.perf_counter() - t_entry      # config, snapshot -> engine (read, re-pack, upload): before the first frame moves
    for _pass in range(4):
        if not (run.run_pass(_pass == 0) and os.environ.get("DGP_EVAL_STRICT", "0") == "1"):
            break
        RUN_STATS["strict_passes"] += 1
        print("DGP_EVAL_STRICT: scales were widened after the first chunk; computing %s again on the final scales" % video_file, flush=True)
    RUN_STATS["prep_backend"] = run.prep_backend
    RUN_STATS["decode_backend"] = run.decode
    sess.close()
    video_clip.close()

    xr = run.markers[:, :, 1] * dlc_cfg.stride + 0.5 * dlc_cfg.stride      # eval.py:352-353
    yr = run.markers[:, :, 0] * dlc_cfg.stride + 0.5 * dlc_cfg.stride
    xr *= run.scale_x
    yr *= run.scale_y
    labels = {"x": xr, "y": yr, "likelihoods": run.likelihoods}
    if loc_ref is not None:
        xr, yr, lik = refined_pose(run.records, dlc_cfg.stride, dlc_cfg.locref_stdev, run.scale_x, run.scale_y)
        labels = {"x": xr, "y": yr, "likelihoods": lik}
    if save_pose and rank == 0:
        if not Path(save_file).parent.exists():
            os.makedirs(os.path.dirname(save_file))
        export_pose_like_dlc(labels, os.path.basename(str(dgp_model_file)), dlc_cfg.all_joints_names, save_file)
    if world > 1:
        tdist.barrier()                # the csv / h5 is complete before any rank goes on (callers read it back)
    return labels


def export_pose_like_dlc(labels, scorer, joints_names, save_file):
    """DLC-format export (eval.py:621-645): columns MultiIndex (scorer, bodyparts, coords), index = frame
    number; csv always, hdf5 (key df_with_missing, table format) when pytables is installed."""
    import pandas as pd
    n_frames, n_labels = labels["x"].shape
    data = np.empty((n_frames, 3 * n_labels), dtype=labels["x"].dtype)
    data[:, 0::3] = labels["x"]
    data[:, 1::3] = labels["y"]
    data[:, 2::3] = labels["likelihoods"]
    cols = pd.MultiIndex.from_product([[scorer], list(joints_names), ["x", "y", "likelihood"]],
                                      names=["scorer", "bodyparts", "coords"])
    df = pd.DataFrame(data, columns=cols, index=np.arange(n_frames))
    try:
        df.to_hdf(save_file + ".h5", key="df_with_missing", format="table", mode="w")
    except ImportError:
        print("pytables not installed: skipping %s.h5 (csv is written)" % save_file)
    df.to_csv(save_file + ".csv")


def load_pose_from_dlc_to_dict(filename):
    """eval.py:648-653."""
    dlc = np.genfromtxt(filename, delimiter=",", dtype=None, encoding=None)
    dlc = dlc[3:, 1:].astype("float")
    return {"x": dlc[:, 0::3], "y": dlc[:, 1::3], "likelihoods": dlc[:, 2::3]}


def plot_dgp(video_file, output_dir="", label_dir=None, proj_cfg_file=None, dgp_model_file=None, shuffle=1, dotsize=3,
             colormap="jet", save_str="", mask_threshold=0.1, new_size=None, tier=None, loc_ref=None, decode_backend="auto",
             movie_backend="auto", movie_quality=90):
    """eval.py:816-874 (`tier`, `loc_ref` and `decode_backend` are new: estimate_pose's).  Exports the labels when missing, then hands (clip, x, y, mask) to the movie
    renderer.  movie_backend (new): "moviepy" = the reference's route (render.create_annotated_movie, an .mp4); "hip" and "host" = this
    package's own writer (render.write_annotated_movie: a Motion-JPEG <name>_labeled<save_str>.avi at movie_quality, the markers drawn and
    the frames encoded on the GPU, or by numpy and Pillow -- the same bytes); "auto" = moviepy when it is installed, else "hip" when a
    GPU is visible, else the labels alone: the csv path is returned and a line says why.  "hip" without a GPU is a ValueError.
    RUN_STATS["movie_backend"] names the writer that ran (None: skipped)."""
    if movie_backend not in ("auto", "moviepy", "hip", "host"):
        raise ValueError("movie_backend must be 'auto', 'moviepy', 'hip' or 'host', got %r" % (movie_backend,))
    if movie_backend == "hip":
        import torch
        if not torch.cuda.is_available():
            raise ValueError("movie_backend 'hip' needs a GPU, and none is visible: use 'host' (the same file, written by Pillow) or 'auto'")
    f = os.path.basename(str(video_file)).rsplit(".", 1)
    save_file = join(output_dir, f[0] + "_labeled%s.mp4" % save_str)
    if label_dir is None:
        label_dir = output_dir
    label_file = join(label_dir, f[0] + "_labeled%s.csv" % save_str)
    from .. import dist as ddist
    import torch.distributed as tdist
    labels = None
    if not ddist.from_rank0(os.path.exists(label_file)):
        labels = estimate_pose(proj_cfg_file, dgp_model_file, video_file, label_dir, shuffle=shuffle, save_str=save_str,
                               new_size=new_size, tier=tier, loc_ref=loc_ref, decode_backend=decode_backend)
    if not isinstance(labels, dict):                       # labels were there already (estimate_pose returns the csv path then)
        labels = load_pose_from_dlc_to_dict(label_file)
    mask_array = labels["likelihoods"].T > mask_threshold
    if tdist.is_available() and tdist.is_initialized() and tdist.get_rank() != 0:
        return label_file                                  # sharded run: rank 0 alone renders the movie
    RUN_STATS["movie_backend"] = None
    if movie_backend == "auto":
        try:
            from moviepy.editor import VideoFileClip  # noqa: F401
            movie_backend = "moviepy"
        except ImportError:
            import torch
            if not torch.cuda.is_available():
                print("moviepy not installed: labels written to %s, annotated movie skipped (%d/%d markers above the "
                      "%.2f likelihood mask)" % (label_file, int(mask_array.sum()), mask_array.size, mask_threshold))
                return label_file
            movie_backend = "hip"
    if movie_backend == "moviepy":
        from .render import create_annotated_movie           # thin moviepy wrapper, optional
        create_annotated_movie(video_file, labels["x"].T, labels["y"].T, mask_array=mask_array, filename=save_file,
                               dotsize=dotsize, colormap=colormap)
    else:
        from .render import write_annotated_movie
        save_file = join(output_dir, f[0] + "_labeled%s.avi" % save_str)
        write_annotated_movie(video_file, labels["x"].T, labels["y"].T, mask_array, save_file, dotsize=dotsize, quality=movie_quality,
                              backend=movie_backend)
    RUN_STATS["movie_backend"] = movie_backend
    return save_file


def pairwisedistances(DataCombined, scorer1, scorer2, pcutoff=-1, bodyparts=None):
    """Per-(image, bodypart) Euclidean px distance between two scorers (PET/evaluate.py:22-32)."""
    mask = DataCombined[scorer2].xs("likelihood", level=1, axis=1) >= pcutoff
    a, b = (DataCombined[scorer1], DataCombined[scorer2]) if bodyparts is None else \
        (DataCombined[scorer1][bodyparts], DataCombined[scorer2][bodyparts])
    sq = (a - b) ** 2
    rmse = np.sqrt(sq.xs("x", level=1, axis=1) + sq.xs("y", level=1, axis=1))
    return rmse, rmse[mask]


def _read_collected_data(folder, scorer):
    """CollectedData_<scorer>.h5 (key df_with_missing) when pytables is installed, else the .csv twin
    (3 header rows: scorer / bodyparts / coords; index = image path)."""
    import pandas as pd
    base = join(folder, "CollectedData_" + scorer)
    try:
        return pd.read_hdf(base + ".h5", "df_with_missing")
    except (ImportError, FileNotFoundError):
        return pd.read_csv(base + ".csv", header=[0, 1, 2], index_col=0)


def soft_argmax_locref_pose(locref, softmax_map, stride, locref_stdev):
    """eval.py:757-786 for one frame: locref [H,W,2nj] (raw head output), softmax_map [H,W,nj] (normalised map of
    argmax_2d_from_cm) -> pose [nj,3] = (soft-argmax position in px + sum_map(softmax * locref * stdev))[::-1], likelihood 1.
    The reference builds `pose_hard_st` as well and keeps `pose_hard_st1`; with a normalised map the two agree."""
    H, W = locref.shape[:2]
    nj = softmax_map.shape[-1]
    lr = np.reshape(np.asarray(locref), (H, W, -1, 2)) * locref_stdev
    xg, yg = np.meshgrid(np.linspace(0, H - 1, H), np.linspace(0, W - 1, W))
    alpha = np.array([xg, yg]).swapaxes(1, 2)                     # 2 x H x W: (row, col) grids
    out = []
    for j in range(nj):
        st_j = np.expand_dims(softmax_map[:, :, j], 0)
        lr_j = np.transpose(lr[:, :, j, :], [2, 0, 1])
        soft = np.sum(np.sum(st_j * alpha, 1), 1) * stride + 0.5 * stride
        offset = np.sum(np.sum(st_j * lr_j, 1), 1)
        out.append(np.hstack((soft + offset)[::-1]))
    return np.hstack((np.array(out), np.ones((nj, 1))))


def evaluate_dgp(proj_cfg_file, dgp_model_file, shuffle=1, loc_ref=None, loc_ref_calc="dlc", tier=None):
    """Evaluate a model by RMSE (px) on the human-labeled train/test images (eval.py:656-813).  `tier` is new (resolve_tier).

    loc_ref=True + loc_ref_calc='dlc': DLC hard arg-max + location refinement (HIP `hard_argmax` kernel);
    loc_ref=False: DGP soft-argmax (HIP `soft_argmax` kernel).  loc_ref=True + any other loc_ref_calc ('dgp'): soft-argmax
    position plus the softmax-weighted mean location-refinement offset (eval.py:752-786; the normalised map and the locref
    field come from the HIP kernels, the two small weighted sums are host numpy as in the reference).  Returns the RMSE
    DataFrame over all train/test data."""
    import pickle
    import pandas as pd
    from PIL import Image
    from ..config import get_train_config, GetTrainingSetFolder
    from .predict import pose_from_argmax
    from .. import engine
    import torch

    with open(proj_cfg_file, "r") as stream:
        proj_config = yaml.safe_load(stream)
    proj_config["video_path"] = None
    dlc_cfg = get_train_config(proj_config, shuffle=shuffle)
    loc_ref = dlc_cfg.location_refinement if loc_ref is None else loc_ref
    if not loc_ref:
        dlc_cfg.location_refinement = False
    try:
        dlc_cfg.net_type = "resnet_50"
        sess, mu_n, softmax_tensor, scmap_t, locref_t, inputs = setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=loc_ref, tier=tier)
    except KeyError:
        dlc_cfg.net_type = "resnet_101"
        sess, mu_n, softmax_tensor, scmap_t, locref_t, inputs = setup_dgp_eval_graph(dlc_cfg, dgp_model_file, loc_ref=loc_ref, tier=tier)

    tsfolder = GetTrainingSetFolder(proj_config)
    scorer_dgp = "DGP"
    Data = _read_collected_data(join(proj_config["project_path"], str(tsfolder)), proj_config["scorer"])
    bodyparts = list(proj_config["bodyparts"])
    meta = join(proj_config["project_path"], str(tsfolder), "Documentation_data-" + proj_config["Task"] + "_" +
                str(int(proj_config["TrainingFraction"][0] * 100)) + "shuffle" + str(shuffle) + ".pickle")
    with open(meta, "rb") as f:
        _, trainIndices, testIndices, _ = pickle.load(f)

    nj = len(dlc_cfg["all_joints_names"])
    pred = np.ones((len(Data.index), 3 * nj))
    for i, imagename in enumerate(Data.index):
        with Image.open(join(proj_config["project_path"], imagename)) as im:
            image = np.asarray(im.convert("RGB"))
        if loc_ref and loc_ref_calc.lower() != "dlc":
            lr, st = sess.run([locref_t, softmax_tensor], feed_dict={inputs: image[None]})
            pose = soft_argmax_locref_pose(lr[0], st[0], dlc_cfg.stride, dlc_cfg.locref_stdev)
        elif loc_ref:
            net = sess.net_for(image.shape[0], image.shape[1])
            fr = torch.from_numpy(np.require(image[None], requirements=["C", "W"])).cuda(sess.device)
            scm, loc = net.forward(fr, want_locref=True)
            idx, prob, offs = engine.hard_argmax(scm, loc)
            pose = pose_from_argmax(idx[0].cpu().numpy(), prob[0].cpu().numpy(), offs[0].cpu().numpy(), dlc_cfg.stride,
                                    dlc_cfg.locref_stdev)
        else:
            mu = sess.run(mu_n, feed_dict={inputs: image[None]})
            p = mu * dlc_cfg.stride + 0.5 * dlc_cfg.stride
            pose = np.hstack([p[0, :, ::-1], np.ones((nj, 1))])
        pred[i, :] = pose.flatten()
    sess.close()

    index = pd.MultiIndex.from_product([[scorer_dgp], dlc_cfg["all_joints_names"], ["x", "y", "likelihood"]],
                                       names=["scorer", "bodyparts", "coords"])
    DataMachine = pd.DataFrame(pred, columns=index, index=Data.index.values)
    DataCombined = pd.concat([Data.T, DataMachine.T], axis=0).T
    RMSE, _ = pairwisedistances(DataCombined, proj_config["scorer"], scorer_dgp, proj_config["pcutoff"], bodyparts)
    testerror = np.nanmean(RMSE.iloc[testIndices].values.flatten())
    trainerror = np.nanmean(RMSE.iloc[trainIndices].values.flatten())
    print("Train error:", np.round(trainerror, 2), " pixels")
    print("Test error:", np.round(testerror, 2), " pixels")
    return RMSE
