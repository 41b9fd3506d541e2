"""Torch-facing wrapper over the C-ABI (include/dgp_hip.h).

torch is plumbing here: it owns device memory and streams; every computation on the hot
path is a HIP kernel in libdgp_hip.so reached through ctypes.  Nothing in this module
falls back to torch ops or to the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .arch import MEAN_PIXEL, BN_EPS


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_cuda(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.DgpError("%s must be a device (cuda/HIP) tensor" % name)
    if t.dtype != dtype:
        raise _lib.DgpError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.DgpError("%s must be contiguous" % name)


class DGPNet:
    """ResNet-v1 backbone + DGP heads on one MI355X.

    Replaces the TF graph built by setup_dgp_eval_graph (DGP/models/eval.py:147-214):
    `forward` is sess.run(scmap), `infer` is the whole per-frame body of estimate_pose's loop
    (eval.py:306-345) for a batch of frames.
    """

    def __init__(self, depth: int = 50, num_joints: int = 4, in_h: int = 480, in_w: int = 640,
                 max_batch: int = 32, with_locref: bool = False, device: int = 0,
                 mean_pixel=MEAN_PIXEL, bn_eps: float = BN_EPS, tier: Optional[str] = None):
        """tier: None = the library's default (the parity tier, or the 16-bit tier under DGP_CONV_MODE=f16); "parity" / "f32x": fp32-class
        arithmetic on H2 cells (the 1e-3 px / bit-exact-index gate); "f16": the 16-bit tier -- 2-byte H1 activation cells, one MFMA per
        product (include/dgp_hip.h, dgp_net_set_tier): a reported tier with measured error, not a parity claim."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.DgpError("no HIP device visible: DGPNet needs an MI355X (there is no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        d = _lib.DgpNetDesc(depth, num_joints, in_h, in_w, max_batch, int(with_locref),
                            (C.c_float * 3)(*mean_pixel), bn_eps)
        h = C.c_void_p()
        _lib.check(self.lib.dgp_net_create(C.byref(d), C.byref(h)), "dgp_net_create")
        self._h = h
        self.depth, self.nj, self.in_h, self.in_w = depth, num_joints, in_h, in_w
        self.max_batch, self.with_locref = max_batch, with_locref
        oh, ow, fh, fw = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.dgp_net_output_dims(h, C.byref(oh), C.byref(ow), C.byref(fh), C.byref(fw)))
        self.out_h, self.out_w, self.feat_h, self.feat_w = oh.value, ow.value, fh.value, fw.value
        self._ws: Optional[torch.Tensor] = None
        self._ws_batch = 0
        # bookkeeping of the H2 activation scales for callers that keep several engines in step (DGPPipeline): widen_count = how often
        # the headroom was raised since load_weights, scale_epoch = bumped by everything that invalidates the calibrated scales
        self.widen_count = 0
        self.scale_epoch = 0
        if tier is not None:
            self.set_tier(tier)

    TIERS = {"parity": 0, "f32x": 0, "f16": 1}

    def set_tier(self, tier):
        t = self.TIERS[tier] if isinstance(tier, str) else int(tier)
        _lib.check(self.lib.dgp_net_set_tier(self._h, t), "dgp_net_set_tier")
        self.scale_epoch += 1                   # the next forward calibrates again

    @property
    def tier(self) -> str:
        return "f16" if self.lib.dgp_net_get_tier(self._h) == 1 else "parity"

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.dgp_net_destroy(h)
            self._h = None

    # -- weights ---------------------------------------------------------------------
    def load_weights(self, weights: Dict[str, np.ndarray]):
        """weights: TF variable name -> fp32 array in TF layout (see synthetic.make_weights)."""
        keep = []
        views = (_lib.DgpTensorView * len(weights))()
        for i, (k, v) in enumerate(weights.items()):
            a = np.ascontiguousarray(v, dtype=np.float32)
            keep.append(a)
            views[i].name = k.encode()
            views[i].data = a.ctypes.data_as(C.POINTER(C.c_float))
            views[i].ndim = a.ndim
            for j in range(4):
                views[i].shape[j] = a.shape[j] if j < a.ndim else 1
        _lib.check(self.lib.dgp_net_load_weights(self._h, views, len(weights)), "dgp_net_load_weights")
        self.widen_count = 0                    # (the library resets the headroom with the weights)
        self.scale_epoch += 1

    def set_input_size(self, in_h: int, in_w: int):
        """Re-plan the geometry for another frame size; weights stay (DLC's step-0 loader changes the size every
        iteration, pose_defaultdataset.py:131-196)."""
        if (in_h, in_w) == (self.in_h, self.in_w):
            return
        _lib.check(self.lib.dgp_net_set_input_size(self._h, in_h, in_w), "dgp_net_set_input_size")
        self.in_h, self.in_w = in_h, in_w
        oh, ow, fh, fw = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.dgp_net_output_dims(self._h, C.byref(oh), C.byref(ow), C.byref(fh), C.byref(fw)))
        self.out_h, self.out_w, self.feat_h, self.feat_w = oh.value, ow.value, fh.value, fw.value
        self._ws_batch = 0                      # workspace is re-checked against the new geometry

    # -- workspace -------------------------------------------------------------------
    def workspace(self, batch: int) -> torch.Tensor:
        if self._ws is None or batch > self._ws_batch:
            n = C.c_size_t()
            _lib.check(self.lib.dgp_net_workspace_bytes(self._h, batch, C.byref(n)), "dgp_net_workspace_bytes")
            if self._ws is None or self._ws.numel() < n.value:
                self._ws = torch.empty(n.value, dtype=torch.uint8, device=self.device)
            self._ws_batch = batch
        return self._ws

    def stats(self, batch: int) -> Tuple[int, float]:
        nl, fl = C.c_int32(), C.c_double()
        _lib.check(self.lib.dgp_net_stats(self._h, batch, C.byref(nl), C.byref(fl)))
        return nl.value, fl.value

    # -- measurement -----------------------------------------------------------------
    def profile_begin(self, max_steps: int):
        _lib.check(self.lib.dgp_net_profile_begin(self._h, max_steps), "dgp_net_profile_begin")

    def profile_end(self):
        """-> list of (name, algorithmic flops, avg ms) per launch of one step."""
        ns, nl = C.c_int32(), C.c_int32()
        _lib.check(self.lib.dgp_net_profile_end(self._h, C.byref(ns), C.byref(nl)), "dgp_net_profile_end")
        out = []
        buf = C.create_string_buffer(256)
        for i in range(nl.value):
            fl, ms = C.c_double(), C.c_double()
            _lib.check(self.lib.dgp_net_profile_launch(self._h, i, buf, 256, C.byref(fl), C.byref(ms)))
            if buf.value:
                out.append((buf.value.decode(), fl.value, ms.value))
        return ns.value, out

    # -- compute ---------------------------------------------------------------------
    def forward(self, frames: torch.Tensor, want_locref: bool = False, want_features: bool = False, check_range: bool = True):
        """frames uint8 [B,H,W,3] on device -> scmap [B,out_h,out_w,nj] (and locref / features).  check_range: as in infer()."""
        _need_cuda(frames, torch.uint8, "frames")
        B = frames.shape[0]
        if tuple(frames.shape[1:]) != (self.in_h, self.in_w, 3):
            raise _lib.DgpError("frames must be [B,%d,%d,3], got %s" % (self.in_h, self.in_w, tuple(frames.shape)))
        scmap = torch.empty((B, self.out_h, self.out_w, self.nj), dtype=torch.float32, device=self.device)
        locref = torch.empty((B, self.out_h, self.out_w, 2 * self.nj), dtype=torch.float32,
                             device=self.device) if want_locref else None
        feats = torch.empty((B, self.feat_h, self.feat_w, 2048), dtype=torch.float32,
                            device=self.device) if want_features else None
        ws = self.workspace(B) if B else None
        for attempt in range(5 if B else 0):           # (an empty batch -- e.g. the empty shard of a short video -- gives empty outputs, like sess.run)
            _lib.check(self.lib.dgp_forward(self._h, _ptr(frames), B, _ptr(ws), ws.numel(), _ptr(scmap), _ptr(locref),
                                            _ptr(feats), _stream(self.device)), "dgp_forward")
            if not check_range or not self.range_status()[0]:
                break
        else:
            if B:
                raise _lib.DgpError("dgp_forward: activation ranges still overflow after 4 re-calibrations (non-finite weights or input?)")
        out = [scmap]
        if want_locref:
            out.append(locref)
        if want_features:
            out.append(feats)
        return out[0] if len(out) == 1 else tuple(out)

    def infer(self, frames: torch.Tensor, gamma: float = 1.0, gauss_len: int = 1, out=None,
              scmap_out: Optional[torch.Tensor] = None, check_range: bool = True):
        """Fused frames -> (mu [B,nj,2] (row,col), conf [B,nj], idx [B,nj,2] int32).

        check_range (default): synchronise and read the H2 range flag after the forward; a batch that outgrew the calibrated
        activation scales is re-run (the engine re-calibrates on it, up to 4 times, then DgpError).  Streaming callers pass
        check_range=False and poll range_status() themselves at a point where they can re-run (eval.estimate_pose, bench.py)."""
        _need_cuda(frames, torch.uint8, "frames")
        B = frames.shape[0]
        if tuple(frames.shape[1:]) != (self.in_h, self.in_w, 3):
            raise _lib.DgpError("frames must be [B,%d,%d,3], got %s" % (self.in_h, self.in_w, tuple(frames.shape)))
        if out is None:
            mu = torch.empty((B, self.nj, 2), dtype=torch.float32, device=self.device)
            conf = torch.empty((B, self.nj), dtype=torch.float32, device=self.device)
            idx = torch.empty((B, self.nj, 2), dtype=torch.int32, device=self.device)
        else:
            mu, conf, idx = out
        if B == 0:                                      # an empty batch gives empty outputs, like sess.run
            return mu, conf, idx
        ws = self.workspace(B)
        for attempt in range(5):
            _lib.check(self.lib.dgp_infer(self._h, _ptr(frames), B, _ptr(ws), ws.numel(), float(gamma), int(gauss_len),
                                          _ptr(mu), _ptr(conf), _ptr(idx), _ptr(scmap_out), _stream(self.device)),
                       "dgp_infer")
            if not check_range or not self.range_status()[0]:
                return mu, conf, idx
        raise _lib.DgpError("dgp_infer: activation ranges still overflow after 4 re-calibrations (non-finite weights or input?)")


    def range_status(self) -> Tuple[bool, int]:
        """(overflow, calibrations).  Synchronises the stream.  overflow: a forward since the last call outgrew the calibrated scale of
        one of its H2 activation tensors (include/dgp_hip.h, "H2"): its results are invalid, the flag is cleared and the next
        forward re-calibrates on its own batch -- re-run what was computed since the last clean status."""
        ov, nc = C.c_int32(), C.c_int32()
        _lib.check(self.lib.dgp_net_range_status(self._h, C.byref(ov), C.byref(nc), _stream(self.device)), "dgp_net_range_status")
        if ov.value:                       # the library widened this engine's headroom and will re-calibrate
            self.widen_count += 1
            self.scale_epoch += 1
        return bool(ov.value), nc.value

    def recalibrate(self):
        """Force a calibration pass of the activation scales on the next forward."""
        _lib.check(self.lib.dgp_net_recalibrate(self._h), "dgp_net_recalibrate")
        self.scale_epoch += 1

    def reset_scales(self):
        """Default headroom again and a calibration pass on the next forward: the state right after load_weights (an engine kept between
        videos starts every video as a fresh one would)."""
        _lib.check(self.lib.dgp_net_reset_scales(self._h), "dgp_net_reset_scales")
        self.widen_count = 0
        self.scale_epoch += 1

    def copy_scales_from(self, other: "DGPNet"):
        """Take `other`'s calibrated activation scales (same network, weights, tier, frame size): what this engine would find by calibrating
        on the same batch itself, without the layer-by-layer pass (dgp_net_copy_scales)."""
        _lib.check(self.lib.dgp_net_copy_scales(self._h, other._h, _stream(self.device)), "dgp_net_copy_scales")
        self.widen_count = other.widen_count
        self.scale_epoch += 1

    def widen(self):
        """Re-calibrate on the next forward with 3 more bits of headroom -- what range_status() does on an overflow -- for a rank
        that follows another rank's overflow in a sharded run."""
        _lib.check(self.lib.dgp_net_widen(self._h), "dgp_net_widen")
        self.widen_count += 1
        self.scale_epoch += 1

    def infer_packed(self, frames: torch.Tensor, traj: torch.Tensor, gamma: float = 1.0, gauss_len: int = 1,
                     scmap_out: Optional[torch.Tensor] = None, loc_ref: Optional[str] = None,
                     locref_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fused frames -> traj [B,nj,5] fp32 lanes (row, col, likelihood, iy, ix; indices as int32 bit patterns): the record
        layout of the per-video trajectory (dist.unpack_keypoints splits it).  `traj` is a caller-owned contiguous slice of the
        trajectory buffer, written in place by the soft-argmax kernel.

        loc_ref (LOC_REF_MODES): location refinement -- the forward also runs the locref head and the read-out writes 7-lane records
        traj [B,nj,7] whose lanes 5..6 are the raw (dx, dy) offset (dist.unpack_offsets).  "dgp": lanes 0..4 as above, the offset is the
        expectation of the locref field under the soft-argmax's map; "dlc": the hard arg-max cell (as floats), its sigmoid, the cell
        again and the offset at that cell.  The net must have been created with_locref."""
        _need_cuda(frames, torch.uint8, "frames")
        _need_cuda(traj, torch.float32, "traj")
        B = frames.shape[0]
        if tuple(frames.shape[1:]) != (self.in_h, self.in_w, 3):
            raise _lib.DgpError("frames must be [B,%d,%d,3], got %s" % (self.in_h, self.in_w, tuple(frames.shape)))
        lanes = record_lanes(loc_ref)
        if tuple(traj.shape) != (B, self.nj, lanes):
            raise _lib.DgpError("traj must be [%d,%d,%d], got %s" % (B, self.nj, lanes, tuple(traj.shape)))
        ws = self.workspace(B)
        if loc_ref is None:
            _lib.check(self.lib.dgp_infer_packed(self._h, _ptr(frames), B, _ptr(ws), ws.numel(), float(gamma), int(gauss_len),
                                                 _ptr(traj), _ptr(scmap_out), _stream(self.device)), "dgp_infer_packed")
        else:
            _lib.check(self.lib.dgp_infer_packed_locref(self._h, _ptr(frames), B, _ptr(ws), ws.numel(), float(gamma), int(gauss_len),
                                                        LOC_REF_MODES[loc_ref], _ptr(traj), _ptr(scmap_out), _ptr(locref_out),
                                                        _stream(self.device)), "dgp_infer_packed_locref")
        return traj


# location refinement in the streaming read-out (dgp_infer_packed_locref's mode): None = off, 5-lane records
LOC_REF_MODES = {"dgp": 1, "dlc": 2}


def record_lanes(loc_ref: Optional[str]) -> int:
    """fp32 lanes of one (frame, joint) record of infer_packed: 5, or 7 with location refinement"""
    if loc_ref is None:
        return 5
    if loc_ref not in LOC_REF_MODES:
        raise ValueError("loc_ref must be None, 'dgp' or 'dlc', not %r" % (loc_ref,))
    return 7


class DGPPipeline:
    """Two engines on two HIP streams, batches dealt to them in turn.

    A forward is a chain of ~50 dependent launches; most layers' grids do not fill a whole number of rounds of the 512 resident
    workgroups, so the tail of every layer runs on a partly idle chip.  With a second, independent batch in flight on another
    stream the hardware fills those tails with the other batch's workgroups: +5 % frames/s on ResNet-50 640x480 batch 32
    (scripts/two_stream_probe.py: 4279 -> 4492 over 300 steps; a third stream adds nothing).  Every engine keeps its own repacked
    weights and workspace (one forward at a time per dgp_net, include/dgp_hip.h); all engines calibrate their activation scales on
    the SAME batch (`calibrate`), so which engine a batch lands on does not change a bit of its result.

    submit() enqueues one batch and returns at once; join() makes the caller's stream wait for everything submitted."""

    def __init__(self, depth: int = 50, num_joints: int = 4, in_h: int = 480, in_w: int = 640, max_batch: int = 32,
                 with_locref: bool = False, device: int = 0, n_streams: int = 2, mean_pixel=MEAN_PIXEL,
                 first: Optional[DGPNet] = None, tier: Optional[str] = None):
        """first: an existing engine of the same configuration to adopt as engine 0 (its weights stay loaded); tier: as DGPNet's."""
        if n_streams < 1:
            raise _lib.DgpError("n_streams must be >= 1")
        self.nets = [first] if first is not None else []
        while len(self.nets) < n_streams:
            self.nets.append(DGPNet(depth, num_joints, in_h, in_w, max_batch, with_locref, device, mean_pixel, tier=tier))
        if tier is not None and first is not None:
            want = "f16" if DGPNet.TIERS[tier] == 1 else "parity"      # compare with the tier that was ASKED for (with n_streams == 1 there is no second engine)
            if first.tier != want:
                first.set_tier(tier)
        self.device = self.nets[0].device
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(n_streams)]
        self.nj, self.max_batch = num_joints, max_batch
        self._next = 0
        self._calibrated = False
        self._epochs = [n.scale_epoch for n in self.nets]
        n0 = self.nets[0]
        self.in_h, self.in_w, self.out_h, self.out_w = n0.in_h, n0.in_w, n0.out_h, n0.out_w

    def load_weights(self, weights: Dict[str, np.ndarray]):
        for n in self.nets:
            n.load_weights(weights)
        self._calibrated = False

    def set_input_size(self, in_h: int, in_w: int):
        for n in self.nets:
            n.set_input_size(in_h, in_w)
        n0 = self.nets[0]
        self.in_h, self.in_w, self.out_h, self.out_w = n0.in_h, n0.in_w, n0.out_h, n0.out_w

    def calibrate(self, frames: torch.Tensor, gamma: float = 1.0, gauss_len: int = 1, loc_ref: Optional[str] = None):
        """Engine 0 runs `frames` (it calibrates on them after load_weights / recalibrate / an overflow) and the other engines take its
        scales (dgp_net_copy_scales: the calibration is deterministic, so that is what each would have found on the same batch -- round 6,
        one layer-by-layer pass per video instead of one per engine); synchronises.  loc_ref: the variant the submits will run."""
        scratch = torch.empty((frames.shape[0], self.nj, record_lanes(loc_ref)), dtype=torch.float32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        n0, st0 = self.nets[0], self.streams[0]
        st0.wait_stream(cur)
        with torch.cuda.stream(st0):
            n0.infer_packed(frames, scratch, gamma, gauss_len, loc_ref=loc_ref)
        st0.synchronize()
        for n, st in zip(self.nets[1:], self.streams[1:]):
            with torch.cuda.stream(st):
                n.copy_scales_from(n0)
        self._calibrated = True
        self._epochs = [n.scale_epoch for n in self.nets]

    def submit(self, frames: torch.Tensor, traj: torch.Tensor, gamma: float = 1.0, gauss_len: int = 1,
               loc_ref: Optional[str] = None) -> "torch.cuda.Event":
        """infer_packed(frames -> traj, loc_ref) on the next engine's stream, ordered after the work already on the caller's current stream.
        Returns the event recorded behind it (frames / traj may be reused once it has completed).  The first batch after
        load_weights / recalibrate / an overflow goes through EVERY engine first (calibrate), so all engines share its scales."""
        if self._calibrated and [n.scale_epoch for n in self.nets] != self._epochs:
            self._resync()                  # an engine was re-calibrated behind the pipeline's back (EvalSession shares engine 0)
        if not self._calibrated:
            self.calibrate(frames, gamma, gauss_len, loc_ref)
        i = self._next
        self._next = (i + 1) % len(self.nets)
        st = self.streams[i]
        st.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(st):
            self.nets[i].infer_packed(frames, traj, gamma, gauss_len, loc_ref=loc_ref)
            ev = torch.cuda.Event()
            ev.record(st)
        return ev

    def _resync(self):
        """Engines whose scales were touched individually (a synchronous forward on a shared engine overflowed and re-calibrated on its
        own batch): give every engine the widest headroom any of them has and calibrate all of them again on ONE batch -- the next
        one submitted -- so that which engine a batch lands on does not change a bit of its result."""
        target = max(n.widen_count for n in self.nets)
        for n in self.nets:
            while n.widen_count < target:
                n.widen()
            n.recalibrate()
        self._calibrated = False

    def join(self):
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            cur.wait_stream(st)

    def range_status(self) -> Tuple[bool, int]:
        """(any engine overflowed, calibrations of the first engine); an overflow on one engine widens ALL of them, so that they
        keep identical scales after the re-calibration (calibrate() again before re-running).  Waits for every engine's stream first:
        the flag is written by the range check at the end of each forward, on the engine's own (non-blocking) stream."""
        for st in self.streams:
            st.synchronize()
        res = [n.range_status() for n in self.nets]
        ov = any(r[0] for r in res)
        if ov:
            for n, r in zip(self.nets, res):
                if not r[0]:
                    n.widen()
            self._calibrated = False
        return ov, res[0][1]

    def recalibrate(self):
        for n in self.nets:
            n.recalibrate()
        self._calibrated = False

    def reset_scales(self):
        for n in self.nets:
            n.reset_scales()
        self._calibrated = False

    def widen(self):
        for n in self.nets:
            n.widen()
        self._calibrated = False


# ---------------------------------------------------------------------------------------
# stand-alone operators
# ---------------------------------------------------------------------------------------
def soft_argmax(scmap: torch.Tensor, gamma: float = 1.0, gauss_len: int = 2, want_pmap: bool = False):
    """HIP argmax_2d_from_cm (+ likelihood window).  scmap fp32 [B,H,W,C] on device."""
    lib = _lib.load()
    _need_cuda(scmap, torch.float32, "scmap")
    if scmap.dim() != 4:
        raise _lib.DgpError("scmap must be rank 4 [B,H,W,C]")      # fitdgp_util.py:357 assert rank == 4
    B, H, W, Cn = scmap.shape
    dev = scmap.device
    mu = torch.empty((B, Cn, 2), dtype=torch.float32, device=dev)
    conf = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    idx = torch.empty((B, Cn, 2), dtype=torch.int32, device=dev)
    pmap = torch.empty_like(scmap) if want_pmap else None
    if B * Cn == 0 and H > 0 and W > 0:                 # no frames or no joints: empty outputs
        return (mu, conf, idx, pmap) if want_pmap else (mu, conf, idx)
    _lib.check(lib.dgp_soft_argmax(_ptr(scmap), B, H, W, Cn, float(gamma), int(gauss_len), _ptr(mu), _ptr(conf),
                                   _ptr(idx), _ptr(pmap), _stream(dev)), "dgp_soft_argmax")
    return (mu, conf, idx, pmap) if want_pmap else (mu, conf, idx)


def soft_argmax_locref(scmap: torch.Tensor, locref: torch.Tensor, gamma: float = 1.0, gauss_len: int = 2, want_pmap: bool = False):
    """soft_argmax plus the location-refinement read-out in the same launch (dgp_soft_argmax_locref): locref fp32 [B,H,W,2C] on device
    -> (mu, conf, idx, offs[, pmap]); offs [B,C,2] = (dx, dy), the expectation of the raw locref field under the normalised blurred
    softmax (multiply by locref_stdev for pixels).  mu, conf, idx, pmap are soft_argmax's, bit for bit."""
    lib = _lib.load()
    _need_cuda(scmap, torch.float32, "scmap")
    if scmap.dim() != 4:
        raise _lib.DgpError("scmap must be rank 4 [B,H,W,C]")
    B, H, W, Cn = scmap.shape
    if locref is not None:
        _need_cuda(locref, torch.float32, "locref")
        if tuple(locref.shape) != (B, H, W, 2 * Cn):
            raise _lib.DgpError("locref must be [B,H,W,2*C]")
    dev = scmap.device
    mu = torch.empty((B, Cn, 2), dtype=torch.float32, device=dev)
    conf = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    idx = torch.empty((B, Cn, 2), dtype=torch.int32, device=dev)
    offs = torch.empty((B, Cn, 2), dtype=torch.float32, device=dev)
    pmap = torch.empty_like(scmap) if want_pmap else None
    if not (B * Cn == 0 and H > 0 and W > 0 and locref is not None):      # no frames or no joints: empty outputs
        _lib.check(lib.dgp_soft_argmax_locref(_ptr(scmap), _ptr(locref), B, H, W, Cn, float(gamma), int(gauss_len), _ptr(mu), _ptr(conf),
                                              _ptr(idx), _ptr(offs), _ptr(pmap), _stream(dev)), "dgp_soft_argmax_locref")
    return (mu, conf, idx, offs, pmap) if want_pmap else (mu, conf, idx, offs)


def pmap_threshold(pmap: torch.Tensor, th: float) -> torch.Tensor:
    """argmax_2d_from_cm's `th` branch (fitdgp_util.py:377-388): pmap [B,H,W,C] (normalised blurred softmax from soft_argmax) is
    thresholded at th * max per (frame, joint) map and renormalised IN PLACE; returns mu [B,C,2] (row, col) of the new maps."""
    lib = _lib.load()
    _need_cuda(pmap, torch.float32, "pmap")
    if pmap.dim() != 4 or not pmap.is_contiguous():
        raise _lib.DgpError("pmap must be a contiguous rank-4 tensor [B,H,W,C]")
    B, H, W, Cn = pmap.shape
    mu = torch.empty((B, Cn, 2), dtype=torch.float32, device=pmap.device)
    if B * Cn == 0 and H > 0 and W > 0:
        return mu
    _lib.check(lib.dgp_pmap_threshold(_ptr(pmap), B, H, W, Cn, float(th), _ptr(mu), _stream(pmap.device)), "dgp_pmap_threshold")
    return mu


def hard_argmax(scmap: torch.Tensor, locref: Optional[torch.Tensor] = None):
    """HIP DLC arg-max: idx [B,C,2] (row,col), prob [B,C], offs [B,C,2] (dx,dy raw locref)."""
    lib = _lib.load()
    _need_cuda(scmap, torch.float32, "scmap")
    B, H, W, Cn = scmap.shape
    if locref is not None:
        _need_cuda(locref, torch.float32, "locref")
        if tuple(locref.shape) != (B, H, W, 2 * Cn):
            raise _lib.DgpError("locref must be [B,H,W,2*C]")
    dev = scmap.device
    idx = torch.empty((B, Cn, 2), dtype=torch.int32, device=dev)
    prob = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    offs = torch.empty((B, Cn, 2), dtype=torch.float32, device=dev)
    if B * Cn == 0 and H > 0 and W > 0:
        return idx, prob, offs
    _lib.check(lib.dgp_hard_argmax(_ptr(scmap), _ptr(locref), B, H, W, Cn, _ptr(idx), _ptr(prob), _ptr(offs),
                                   _stream(dev)), "dgp_hard_argmax")
    return idx, prob, offs


def pack_conv_weights(w_hwio: np.ndarray) -> np.ndarray:
    lib = _lib.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    kh, kw, cin, cout = w.shape
    n = lib.dgp_packed_weight_floats(kh, kw, cin, cout)
    if n == 0:
        raise _lib.DgpError("unsupported conv weight shape %s (Cin must be 4*2^k)" % (w.shape,))
    out = np.empty(n, dtype=np.float32)
    _lib.check(lib.dgp_pack_conv_weights(w.ctypes.data_as(C.c_void_p), kh, kw, cin, cout,
                                         out.ctypes.data_as(C.c_void_p)), "dgp_pack_conv_weights")
    return out


ABSMAX_SLOTS = 256      # DGP_ABSMAX_SLOTS in include/dgp_hip.h


def conv2d(x: torch.Tensor, w_hwio: np.ndarray, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
           out_hw: Optional[Tuple[int, int]] = None, scale=None, bias=None, residual: Optional[torch.Tensor] = None,
           res_stride: int = 0, relu: bool = False, ranged: bool = False, return_range: bool = False,
           tail_slab: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """Single conv layer through the implicit-GEMM kernel (NHWC fp32).

    tail_slab: a float32 device tensor the launch may use for the K-split of its grid's tail (dgp_conv2d_ranged_slab; see
    conv2d_plan for whether it does); out: the caller's output tensor [N,Ho,Wo,Cout] (float32, contiguous) instead of a new one.

    ranged=True measures max |x| and max |w| on the device first (dgp_tensor_absmax) and passes them on, which lets
    the fp16 high/low split kernels run (dgp_conv2d_ranged); return_range=True also returns max |y| as tracked by the
    epilogue (a device tensor of DGP_ABSMAX_SLOTS floats whose maximum is the value)."""
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    N, H, W, Cin = x.shape
    kh, kw, cin2, cout = w_hwio.shape
    assert cin2 == Cin
    dev = x.device
    if out_hw is None:
        keh, kew = (kh - 1) * rate + 1, (kw - 1) * rate + 1
        out_hw = ((H + 2 * pad_t - keh) // stride + 1, (W + 2 * pad_l - kew) // stride + 1)
    Ho, Wo = out_hw
    wp = torch.from_numpy(pack_conv_weights(w_hwio)).to(dev)
    sc = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).contiguous().to(dev)
    bi = None if bias is None else torch.as_tensor(bias, dtype=torch.float32).contiguous().to(dev)
    y = _conv_out(out, (N, Ho, Wo, cout), dev)
    rh, rw = (residual.shape[1], residual.shape[2]) if residual is not None else (0, 0)
    d = _lib.DgpConvDesc(N, H, W, Cin, cout, kh, kw, stride, rate, pad_t, pad_l, Ho, Wo, int(relu),
                         res_stride if residual is not None else 0, rh, rw)
    if tail_slab is not None:
        _need_cuda(tail_slab, torch.float32, "tail_slab")
    if not (ranged or return_range or tail_slab is not None):
        _lib.check(lib.dgp_conv2d(C.byref(d), _ptr(x), _ptr(wp), _ptr(sc), _ptr(bi), _ptr(residual), _ptr(y),
                                  _stream(dev)), "dgp_conv2d")
        return y
    rng = torch.zeros((3, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    if ranged:
        _lib.check(lib.dgp_tensor_absmax(_ptr(x), x.numel(), _ptr(rng[0]), _stream(dev)), "dgp_tensor_absmax")
        _lib.check(lib.dgp_tensor_absmax(_ptr(wp), wp.numel(), _ptr(rng[1]), _stream(dev)), "dgp_tensor_absmax")
    if tail_slab is not None:
        _lib.check(lib.dgp_conv2d_ranged_slab(C.byref(d), _ptr(x), _ptr(wp), _ptr(sc), _ptr(bi), _ptr(residual), _ptr(y),
                                              _ptr(rng[0]) if ranged else None, _ptr(rng[1]) if ranged else None, _ptr(rng[2]),
                                              _ptr(tail_slab), tail_slab.numel() * 4, _stream(dev)), "dgp_conv2d_ranged_slab")
        return (y, rng[2]) if return_range else y
    _lib.check(lib.dgp_conv2d_ranged(C.byref(d), _ptr(x), _ptr(wp), _ptr(sc), _ptr(bi), _ptr(residual), _ptr(y),
                                     _ptr(rng[0]) if ranged else None, _ptr(rng[1]) if ranged else None, _ptr(rng[2]),
                                     _stream(dev)), "dgp_conv2d_ranged")
    return (y, rng[2]) if return_range else y


def _conv_out(out, shape, dev, dtype=torch.float32):
    """the output tensor of a layer call: the caller's (checked) or a new one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    _need_cuda(out, dtype, "out")
    if tuple(out.shape) != tuple(shape) or out.device != dev:
        raise _lib.DgpError("out must be a %s tensor of shape %s on %s" % (str(dtype).replace("torch.", ""), tuple(shape), dev))
    return out


def conv2d_plan(x_shape, w_shape, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0, out_hw=None, res_stride: int = 0,
                res_hw=(0, 0), in_fmt: int = 0, out_fmt: int = 0, res_fmt: int = 0, ranged: bool = True, cells: bool = False,
                slab_bytes: int = 0, tile: int = -1, n_cu: int = 0) -> dict:
    """What the launch layer would run for this layer (dgp_conv2d_plan): tile, kernel family and path, grid, tail K-split, supertile
    order.  Formats: 0 fp32, 1 H2, 2 H1.  n_cu > 0 plans for that many compute units and needs no GPU; 0 asks the current device."""
    lib = _lib.load()
    N, H, W, Cin = x_shape
    kh, kw, _, cout = w_shape
    if out_hw is None:
        keh, kew = (kh - 1) * rate + 1, (kw - 1) * rate + 1
        out_hw = ((H + 2 * pad_t - keh) // stride + 1, (W + 2 * pad_l - kew) // stride + 1)
    d = _lib.DgpConvDesc(N, H, W, Cin, cout, kh, kw, stride, rate, pad_t, pad_l, out_hw[0], out_hw[1], 0, res_stride, res_hw[0], res_hw[1])
    pl = _lib.DgpConvPlan()
    _lib.check(lib.dgp_conv2d_plan(C.byref(d), in_fmt, out_fmt, res_fmt, int(ranged), int(cells), int(slab_bytes), int(tile), int(n_cu),
                                   C.byref(pl)), "dgp_conv2d_plan")
    res = {n: int(getattr(pl, n)) for n, _ in _lib.DgpConvPlan._fields_ if n != "kernel_name"}
    res["kernel_name"] = pl.kernel_name.decode()
    return res


def _conv_desc(x_shape, w_shape, stride, rate, pad_t, pad_l, out_hw):
    N, H, W, Cin = x_shape
    kh, kw, _, cout = w_shape
    Ho, Wo = out_hw
    return _lib.DgpConvDesc(N, H, W, Cin, cout, kh, kw, stride, rate, pad_t, pad_l, Ho, Wo, 0, 0, 0, 0)


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, ksize: int, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
                 ranged: bool = True):
    """Weight gradient of one conv layer through the trainer's kernels: x [N,H,W,Cin], dy [N,Ho,Wo,Cout] ->
    (dW [k,k,Cin,Cout] HWIO, colsum [Cout]).  ranged: measure both operand ranges first (fp16-split kernel on 128 x 128 tiles)."""
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    _need_cuda(dy, torch.float32, "dy")
    dev = x.device
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    d = _conv_desc(x.shape, (ksize, ksize, Cin, Cout), stride, rate, pad_t, pad_l, (Ho, Wo))
    dw = torch.empty((ksize, ksize, Cin, Cout), dtype=torch.float32, device=dev)
    cs = torch.empty(2 * Cout, dtype=torch.float32, device=dev)
    rng = torch.zeros((2, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    if ranged:
        _lib.check(lib.dgp_tensor_absmax(_ptr(x), x.numel(), _ptr(rng[0]), _stream(dev)), "dgp_tensor_absmax")
        _lib.check(lib.dgp_tensor_absmax(_ptr(dy), dy.numel(), _ptr(rng[1]), _stream(dev)), "dgp_tensor_absmax")
    _lib.check(lib.dgp_conv2d_wgrad(C.byref(d), _ptr(x), _ptr(dy), _ptr(rng[0]) if ranged else None,
                                    _ptr(rng[1]) if ranged else None, _ptr(dw), _ptr(cs), _stream(dev)), "dgp_conv2d_wgrad")
    return dw, cs[:Cout]


def conv2d_wgrad_shadow(x: torch.Tensor, dy: torch.Tensor, ksize: int, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
                        prev_ratio: Tuple[float, float] = (1.0, 1.0)):
    """conv2d_wgrad through the training step's LDS-DMA tile: both operands are copied into fp16 high / low cells with the scales a
    "previous step" whose maxima were prev_ratio times this step's would predict (1.0: the steady state; 2^-6 or 2^8: the prediction
    fails and the kernel computes the tile from the fp32 tensors; 0: no previous range at all, the first step)."""
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    _need_cuda(dy, torch.float32, "dy")
    dev = x.device
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    d = _conv_desc(x.shape, (ksize, ksize, Cin, Cout), stride, rate, pad_t, pad_l, (Ho, Wo))
    dw = torch.empty((ksize, ksize, Cin, Cout), dtype=torch.float32, device=dev)
    cs = torch.empty(2 * Cout, dtype=torch.float32, device=dev)
    rng = torch.zeros((2, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    _lib.check(lib.dgp_tensor_absmax(_ptr(x), x.numel(), _ptr(rng[0]), _stream(dev)), "dgp_tensor_absmax")
    _lib.check(lib.dgp_tensor_absmax(_ptr(dy), dy.numel(), _ptr(rng[1]), _stream(dev)), "dgp_tensor_absmax")
    prev = torch.stack([rng[0] * float(prev_ratio[0]), rng[1] * float(prev_ratio[1])]).contiguous()
    scratch = torch.empty(x.numel() + dy.numel(), dtype=torch.float32, device=dev)
    _lib.check(lib.dgp_conv2d_wgrad_shadow(C.byref(d), _ptr(x), _ptr(dy), _ptr(rng[0]), _ptr(rng[1]), _ptr(prev[0]), _ptr(prev[1]),
                                           _ptr(scratch), _ptr(dw), _ptr(cs), _stream(dev)), "dgp_conv2d_wgrad_shadow")
    return dw, cs[:Cout]


def conv2d_dgrad(dy: torch.Tensor, w_hwio: torch.Tensor, x_hw: Tuple[int, int], stride: int = 1, rate: int = 1, pad_t: int = 0,
                 pad_l: int = 0, scale: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                 dx_add: Optional[torch.Tensor] = None, add_mode: int = 1, ranged: bool = True, mask_h2: bool = False) -> torch.Tensor:
    """Data gradient of one conv layer through the trainer's kernels: dy [N,Ho,Wo,Cout], w [k,k,Cin,Cout] (device) -> dx [N,H,W,Cin].
    mask_h2: hand the gate tensor over as H2 cells (the fast pass of the training step keeps its activations that way)."""
    lib = _lib.load()
    _need_cuda(dy, torch.float32, "dy")
    _need_cuda(w_hwio, torch.float32, "w_hwio")
    dev = dy.device
    N, Ho, Wo, Cout = dy.shape
    kh, kw, Cin, _ = w_hwio.shape
    H, W = x_hw
    d = _conv_desc((N, H, W, Cin), w_hwio.shape, stride, rate, pad_t, pad_l, (Ho, Wo))
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.dgp_conv2d_dgrad_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    flags = int(bool(ranged))
    if mask_h2 and mask is not None:
        mask = f32_to_h2(mask.contiguous(), h2_exp_for(float(mask.abs().max())))
        flags |= 2
    _lib.check(lib.dgp_conv2d_dgrad(C.byref(d), _ptr(dy), _ptr(w_hwio), _ptr(scale), _ptr(mask), _ptr(dx_add), add_mode, _ptr(dx),
                                    _ptr(scratch), flags, _stream(dev)), "dgp_conv2d_dgrad")
    return dx


# ---- layer-level entry points of the 16-bit tier's backward pass (tests): fp32 tensors in, H1 tensors made by the trainer's converter ----
def _slots(value: float, dev) -> torch.Tensor:
    """Range slots whose maximum is `value` (what a producer's epilogue leaves: here every slot the same)."""
    return torch.full((ABSMAX_SLOTS,), float(value), dtype=torch.float32, device=dev)


def _measured(x: torch.Tensor) -> torch.Tensor:
    rng = torch.zeros(ABSMAX_SLOTS, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dgp_tensor_absmax(_ptr(x), x.numel(), _ptr(rng), _stream(x.device)), "dgp_tensor_absmax")
    return rng


def h1_to_f32_pred(x_h1: torch.Tensor, prev_max: float, gate_h1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """H1 cells written with the scale a previous maximum `prev_max` predicts -> fp32 (zero where gate_h1's half is not positive)."""
    _need_cuda(x_h1, torch.float16, "x_h1")
    out = torch.empty(x_h1.shape, dtype=torch.float32, device=x_h1.device)
    prev = _slots(prev_max, x_h1.device)
    _lib.check(_lib.load().dgp_h1_to_f32_pred(_ptr(x_h1), x_h1.numel(), _ptr(prev), _ptr(gate_h1), _ptr(out), _stream(x_h1.device)),
               "dgp_h1_to_f32_pred")
    return out


def conv2d_wgrad_h1(x: torch.Tensor, dy: torch.Tensor, ksize: int, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
                    prev_max: Optional[Tuple[float, float]] = None):
    """conv2d_wgrad through wgrad_dma_h1.  prev_max: last step's maxima of (x, dy) that predict the scales (None: this step's).
    -> (dW [k,k,Cin,Cout], colsum [Cout], x cells, dy cells (float16, as the kernel read them), flag)."""
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    _need_cuda(dy, torch.float32, "dy")
    dev = x.device
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    d = _conv_desc(x.shape, (ksize, ksize, Cin, Cout), stride, rate, pad_t, pad_l, (Ho, Wo))
    dw = torch.empty((ksize, ksize, Cin, Cout), dtype=torch.float32, device=dev)
    cs = torch.empty(2 * Cout, dtype=torch.float32, device=dev)
    cur = (_measured(x), _measured(dy))
    if prev_max is None:
        prev_max = (float(cur[0].max()), float(cur[1].max()))
    prev = (_slots(prev_max[0], dev), _slots(prev_max[1], dev))
    scratch = torch.zeros(x.numel() + dy.numel(), dtype=torch.float16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.dgp_conv2d_wgrad_h1(C.byref(d), _ptr(x), _ptr(dy), _ptr(cur[0]), _ptr(cur[1]), _ptr(prev[0]), _ptr(prev[1]),
                                       _ptr(scratch), _ptr(dw), _ptr(cs), _ptr(flag), _stream(dev)), "dgp_conv2d_wgrad_h1")
    return dw, cs[:Cout], scratch[:x.numel()].view(x.shape), scratch[x.numel():].view(dy.shape), int(flag.item())


def conv2d_dgrad_h1(dy: torch.Tensor, w_hwio: torch.Tensor, x_hw: Tuple[int, int], stride: int = 1, rate: int = 1, pad_t: int = 0,
                    pad_l: int = 0, scale: Optional[torch.Tensor] = None, gate_h1: Optional[torch.Tensor] = None,
                    dx_add: Optional[torch.Tensor] = None, add_mode: int = 1, dy_prev: float = 0.0, dx_prev: float = 0.0,
                    add_prev: float = 0.0):
    """conv2d_dgrad as the 16-bit pass's H1 -> H1 launch.  *_prev: last step's maxima that predict the scales of dy, dx and dx_add;
    gate_h1: the gate as float16 cells (f32_to_h1).  -> dict(dx: float16 cells [N,H,W,Cin], dx_f32: the same through the pass's H1 -> fp32
    converter, dy / add: the cells the kernel read, flag)."""
    lib = _lib.load()
    _need_cuda(dy, torch.float32, "dy")
    _need_cuda(w_hwio, torch.float32, "w_hwio")
    dev = dy.device
    N, Ho, Wo, Cout = dy.shape
    kh, kw, Cin, _ = w_hwio.shape
    H, W = x_hw
    d = _conv_desc((N, H, W, Cin), w_hwio.shape, stride, rate, pad_t, pad_l, (Ho, Wo))
    base = int(lib.dgp_conv2d_dgrad_scratch_bytes(C.byref(d)))
    na = dx_add.numel() if dx_add is not None else 0
    nbytes = base + 2 * dy.numel() + 2 * na + (8 * dy.numel() if stride == 2 else 0)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    dx = torch.zeros((N, H, W, Cin), dtype=torch.float16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    prevs = (_slots(dy_prev, dev), _slots(dx_prev, dev), _slots(add_prev, dev))
    _lib.check(lib.dgp_conv2d_dgrad_h1(C.byref(d), _ptr(dy), _ptr(w_hwio), _ptr(scale), _ptr(gate_h1), _ptr(dx_add), add_mode,
                                       _ptr(prevs[0]), _ptr(prevs[1]), _ptr(prevs[2]) if dx_add is not None else None, _ptr(scratch),
                                       _ptr(dx), _ptr(flag), _stream(dev)), "dgp_conv2d_dgrad_h1")
    out = dict(dx=dx, dx_f32=h1_to_f32_pred(dx, dx_prev), flag=int(flag.item()))
    out["dy"] = scratch[base: base + 2 * dy.numel()].view(torch.float16).view(dy.shape)
    if dx_add is not None:
        out["add"] = scratch[base + 2 * dy.numel(): base + 2 * dy.numel() + 2 * na].view(torch.float16).view(dx_add.shape)
    if stride == 2:
        z0 = base + 2 * dy.numel() + 2 * na
        out["stuffed"] = scratch[z0: z0 + 8 * dy.numel()].view(torch.float16).view(N, 2 * Ho, 2 * Wo, Cout)
    return out


def stem_wgrad_h1(x_centred: torch.Tensor, dpool: torch.Tensor, idx: torch.Tensor, dpool_prev: float):
    """The fused stem weight gradient of the 16-bit pass: x_centred [B,H,W,4] fp32, dpool [B,HP,WP,64] fp32, idx uint8 first-maximum
    record.  -> (dw [7,7,4,64], colsum [64], dpool cells float16)."""
    lib = _lib.load()
    _need_cuda(x_centred, torch.float32, "x_centred")
    _need_cuda(dpool, torch.float32, "dpool")
    _need_cuda(idx, torch.uint8, "idx")
    dev = dpool.device
    B, H, W, _ = x_centred.shape
    H1, W1 = (H + 1) // 2, (W + 1) // 2
    HP, WP = (H1 + 1) // 2, (W1 + 1) // 2
    assert dpool.shape == (B, HP, WP, 64) and idx.shape == dpool.shape and x_centred.shape[3] == 4
    cells_bytes = (2 * dpool.numel() + 255) // 256 * 256
    rows = B * ((H1 + 3) // 4) * ((W1 + 31) // 32)
    scratch = torch.zeros(cells_bytes + rows * (196 * 64 + 64) * 4, dtype=torch.uint8, device=dev)
    dw = torch.empty((7, 7, 4, 64), dtype=torch.float32, device=dev)
    cs = torch.empty(64, dtype=torch.float32, device=dev)
    prev = _slots(dpool_prev, dev)
    _lib.check(lib.dgp_stem_wgrad_h1(_ptr(x_centred), _ptr(dpool), _ptr(prev), _ptr(idx), B, H, W, H1, W1, HP, WP, _ptr(scratch), _ptr(dw),
                                     _ptr(cs), _stream(dev)), "dgp_stem_wgrad_h1")
    return dw, cs, scratch[:2 * dpool.numel()].view(torch.float16).view(dpool.shape)


def heads_backward_h1(feat: torch.Tensor, dscmap: torch.Tensor, dlocref: torch.Tensor, w_part: torch.Tensor, w_locref: torch.Tensor,
                      ct: int, feat_prev: float, dph_prev: float, dfeat_prev: float):
    """Both heads' backward of the 16-bit pass.  w_*: [3,3,njt,Cin] (the trainer's layout); ct: columns of the merged gradient tensor
    (only to size and slice the scratch).  -> dict(dw_part, db_part, dw_locref, db_locref, dfeat: float16 cells, feat / merged: the cells
    the kernels read, flag)."""
    lib = _lib.load()
    for t, nm in ((feat, "feat"), (dscmap, "dscmap"), (dlocref, "dlocref"), (w_part, "w_part"), (w_locref, "w_locref")):
        _need_cuda(t, torch.float32, nm)
    dev = feat.device
    N, h, w, Cin = feat.shape
    nj = dscmap.shape[3]
    up = lambda b: (b + 255) // 256 * 256
    M = N * h * w
    nbytes = up(2 * M * Cin) + up(2 * M * ct) + 48 * Cin * ct + 16384
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    res = dict(dw_part=torch.empty((3, 3, nj, Cin), dtype=torch.float32, device=dev), db_part=torch.empty(nj, dtype=torch.float32, device=dev),
               dw_locref=torch.empty((3, 3, 2 * nj, Cin), dtype=torch.float32, device=dev),
               db_locref=torch.empty(2 * nj, dtype=torch.float32, device=dev), dfeat=torch.zeros((N, h, w, Cin), dtype=torch.float16, device=dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    prevs = (_slots(feat_prev, dev), _slots(dph_prev, dev), _slots(dfeat_prev, dev))
    _lib.check(lib.dgp_heads_backward_h1(_ptr(feat), _ptr(prevs[0]), _ptr(dscmap), _ptr(dlocref), _ptr(prevs[1]), _ptr(w_part), _ptr(w_locref),
                                         _ptr(prevs[2]), N, h, w, Cin, nj, _ptr(scratch), _ptr(res["dw_part"]), _ptr(res["db_part"]),
                                         _ptr(res["dw_locref"]), _ptr(res["db_locref"]), _ptr(res["dfeat"]), _ptr(flag), _stream(dev)),
               "dgp_heads_backward_h1")
    res["flag"] = int(flag.item())
    res["feat"] = scratch[:2 * M * Cin].view(torch.float16).view(N, h, w, Cin)
    o = up(2 * M * Cin)
    res["merged"] = scratch[o: o + 2 * M * ct].view(torch.float16).view(N, h, w, ct)
    return res


# ---- the root block's pool with its first-maximum record, and the fused root block, as layers (tests) ----
def _pool_hw(h1: int, w1: int) -> Tuple[int, int]:
    return (h1 + 1) // 2, (w1 + 1) // 2


def maxpool_fwd_idx(c1: torch.Tensor, prev_max: Optional[float] = None):
    """The training step's unfused pool as forward_root launches it: c1 [B,H1,W1,64] fp32 -> (pool fp32 [B,HP,WP,64], record uint8
    [B,HP,WP,64], H1 copy float16 at the scale prev_max predicts, or None without prev_max)."""
    lib = _lib.load()
    _need_cuda(c1, torch.float32, "c1")
    dev = c1.device
    B, H1, W1, Cn = c1.shape
    if Cn != 64:
        raise _lib.DgpError("c1 must have 64 channels")
    HP, WP = _pool_hw(H1, W1)
    pool = torch.empty((B, HP, WP, 64), dtype=torch.float32, device=dev)
    rec = torch.empty((B, HP, WP, 64), dtype=torch.uint8, device=dev)
    prev = None if prev_max is None else _slots(prev_max, dev)
    h1c = None if prev_max is None else torch.zeros((B, HP, WP, 64), dtype=torch.float16, device=dev)
    _lib.check(lib.dgp_maxpool_fwd_idx(_ptr(c1), B, H1, W1, HP, WP, _ptr(prev), _ptr(pool), _ptr(rec), _ptr(h1c), _stream(dev)),
               "dgp_maxpool_fwd_idx")
    return pool, rec, h1c


def maxpool_bwd_idx(c1: Optional[torch.Tensor], dpool: torch.Tensor, record: torch.Tensor,
                    hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The pool's backward as backward_root launches it: dpool [B,HP,WP,64] fp32, record uint8 -> dc1 [B,H1,W1,64] gated by c1 > 0.
    c1 None: the 16-bit tier's ungated form; hw = (H1, W1) then names the conv1 map (two sizes share one pool map)."""
    lib = _lib.load()
    _need_cuda(dpool, torch.float32, "dpool")
    _need_cuda(record, torch.uint8, "record")
    dev = dpool.device
    B, HP, WP, Cn = dpool.shape
    if c1 is not None:
        _need_cuda(c1, torch.float32, "c1")
        hw = (c1.shape[1], c1.shape[2])
        if c1.shape[0] != B or c1.shape[3] != 64:
            raise _lib.DgpError("c1 must be [B,H1,W1,64]")
    if hw is None:
        raise _lib.DgpError("maxpool_bwd_idx: without c1 the conv1 map's size hw = (H1, W1) is needed")
    if Cn != 64 or tuple(record.shape) != tuple(dpool.shape):
        raise _lib.DgpError("dpool and record must be [B,HP,WP,64]")
    H1, W1 = int(hw[0]), int(hw[1])
    dc1 = torch.empty((B, H1, W1, 64), dtype=torch.float32, device=dev)
    _lib.check(lib.dgp_maxpool_bwd_idx(_ptr(c1), _ptr(dpool), _ptr(record), B, H1, W1, HP, WP, _ptr(dc1), _stream(dev)),
               "dgp_maxpool_bwd_idx")
    return dc1


def root_block(frames_u8: torch.Tensor, w_hwio: torch.Tensor, bn_scale: torch.Tensor, bn_bias: torch.Tensor, mean_pixel=MEAN_PIXEL, *,
               cells: str, prev_max: Optional[float] = None, out_exp: Optional[int] = None, record: bool = False):
    """The fused root block (stem_pool_fused_kernel) as a layer: frames_u8 [B,H,W,3] uint8 (any byte alignment: a view into a larger
    buffer is fine as long as it is contiguous), w_hwio [7,7,3,64], bn_scale / bn_bias [64] -> (pool cells, record or None, tracked maximum).
    cells "h2": the parity tier's inference kernel, cells as f32_to_h2 lays them out (fp32-typed [B,HP,WP,64]) at 2^out_exp;
    cells "h1": the 16-bit tier's kernel, float16 [B,HP,WP,64] at 2^out_exp, or at the scale prev_max predicts; record=True (with prev_max)
    also returns the first-maximum record, as the training step launches it."""
    lib = _lib.load()
    _need_cuda(frames_u8, torch.uint8, "frames_u8")
    for t, nm in ((w_hwio, "w_hwio"), (bn_scale, "bn_scale"), (bn_bias, "bn_bias")):
        _need_cuda(t, torch.float32, nm)
    if tuple(w_hwio.shape) != (7, 7, 3, 64) or bn_scale.numel() != 64 or bn_bias.numel() != 64 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise _lib.DgpError("root_block: frames [B,H,W,3], w_hwio [7,7,3,64], bn_scale / bn_bias [64]")
    if cells not in ("h1", "h2"):
        raise _lib.DgpError("root_block: cells 'h1' or 'h2'")
    if (prev_max is None) == (out_exp is None) and not record:
        raise _lib.DgpError("root_block: exactly one of prev_max (predicted scale) and out_exp (fixed scale)")
    dev = frames_u8.device
    B, H, W, _ = frames_u8.shape
    HP, WP = _pool_hw((H + 1) // 2, (W + 1) // 2)
    out = torch.zeros((B, HP, WP, 64), dtype=torch.float16 if cells == "h1" else torch.float32, device=dev)
    rec = torch.zeros((B, HP, WP, 64), dtype=torch.uint8, device=dev) if record else None
    amax = torch.zeros(ABSMAX_SLOTS, dtype=torch.float32, device=dev)
    prev = None if prev_max is None else _slots(prev_max, dev)
    scratch = torch.zeros(int(lib.dgp_root_block_scratch_bytes()), dtype=torch.uint8, device=dev)
    m = (C.c_float * 3)(*mean_pixel)
    _lib.check(lib.dgp_root_block(_ptr(frames_u8), B, H, W, _ptr(w_hwio), _ptr(bn_scale), _ptr(bn_bias), m, 2 if cells == "h1" else 1,
                                  int(out_exp or 0), _ptr(prev), _ptr(rec), _ptr(scratch), _ptr(out), _ptr(amax), _stream(dev)),
               "dgp_root_block")
    return out, rec, float(amax.max())


def h2_exp_for(absmax: float, headroom_bits: int = 4) -> int:
    """The engine's scale rule: exponent e with absmax * 2^e in [2^(14 - headroom), 2^(15 - headroom))."""
    import math
    if not (absmax > 0) or not math.isfinite(absmax):
        return 0
    return (14 - headroom_bits) - (math.frexp(absmax)[1] - 1)


def f32_to_h2(x: torch.Tensor, scale_exp: int) -> torch.Tensor:
    """fp32 [..., C] (C % 8 == 0) -> H2 cells (fp16 high / low pairs per 8 channels, x * 2^scale_exp), same shape, viewed as fp32 bits."""
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    out = torch.empty_like(x)
    _lib.check(lib.dgp_f32_to_h2(_ptr(x), x.numel(), int(scale_exp), _ptr(out), _stream(x.device)), "dgp_f32_to_h2")
    return out


def h2_to_f32(x: torch.Tensor, scale_exp: int) -> torch.Tensor:
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    out = torch.empty_like(x)
    _lib.check(lib.dgp_h2_to_f32(_ptr(x), x.numel(), int(scale_exp), _ptr(out), _stream(x.device)), "dgp_h2_to_f32")
    return out


def conv2d_h2(x_h2: torch.Tensor, x_exp: int, w_hwio: np.ndarray, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
              out_hw: Optional[Tuple[int, int]] = None, scale=None, bias=None, residual: Optional[torch.Tensor] = None,
              res_stride: int = 0, res_is_h2: bool = False, res_exp: int = 0, relu: bool = False, y_is_h2: bool = True,
              y_exp: int = 0, tail_slab: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """One conv layer on H2 tensors through the engine's cell kernels.  -> (y, y_absmax_slots).  tail_slab, out: as in conv2d."""
    lib = _lib.load()
    _need_cuda(x_h2, torch.float32, "x_h2")
    N, H, W, Cin = x_h2.shape
    kh, kw, cin2, cout = w_hwio.shape
    assert cin2 == Cin
    dev = x_h2.device
    if out_hw is None:
        keh, kew = (kh - 1) * rate + 1, (kw - 1) * rate + 1
        out_hw = ((H + 2 * pad_t - keh) // stride + 1, (W + 2 * pad_l - kew) // stride + 1)
    Ho, Wo = out_hw
    wp = torch.from_numpy(pack_conv_weights(w_hwio)).to(dev)
    sc = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).contiguous().to(dev)
    bi = None if bias is None else torch.as_tensor(bias, dtype=torch.float32).contiguous().to(dev)
    y = _conv_out(out, (N, Ho, Wo, cout), dev)
    rh, rw = (residual.shape[1], residual.shape[2]) if residual is not None else (0, 0)
    d = _lib.DgpConvDesc(N, H, W, Cin, cout, kh, kw, stride, rate, pad_t, pad_l, Ho, Wo, int(relu),
                         res_stride if residual is not None else 0, rh, rw)
    rng = torch.zeros((2, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    _lib.check(lib.dgp_tensor_absmax(_ptr(wp), wp.numel(), _ptr(rng[0]), _stream(dev)), "dgp_tensor_absmax")
    cells = torch.empty(wp.numel(), dtype=torch.float32, device=dev)
    if tail_slab is not None:
        _need_cuda(tail_slab, torch.float32, "tail_slab")
        _lib.check(lib.dgp_conv2d_h2_slab(C.byref(d), _ptr(x_h2), int(x_exp), _ptr(wp), _ptr(rng[0]), _ptr(sc), _ptr(bi), _ptr(residual),
                                          int(res_is_h2), int(res_exp), _ptr(y), int(y_is_h2), int(y_exp), _ptr(rng[1]), _ptr(cells),
                                          _ptr(tail_slab), tail_slab.numel() * 4, _stream(dev)), "dgp_conv2d_h2_slab")
        return y, rng[1]
    _lib.check(lib.dgp_conv2d_h2(C.byref(d), _ptr(x_h2), int(x_exp), _ptr(wp), _ptr(rng[0]), _ptr(sc), _ptr(bi), _ptr(residual),
                                 int(res_is_h2), int(res_exp), _ptr(y), int(y_is_h2), int(y_exp), _ptr(rng[1]), _ptr(cells),
                                 _stream(dev)), "dgp_conv2d_h2")
    return y, rng[1]


def f32_to_h1(x: torch.Tensor, scale_exp: int) -> torch.Tensor:
    """fp32 [..., C] (C % 8 == 0) -> H1 cells (the 16-bit tier's activation format: fp16(x * 2^exp), 16 bytes per 8 channels), returned
    as a float16 tensor of x's shape -- the cells ARE plain NHWC fp16 with a per-tensor scale."""
    _need_cuda(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().dgp_f32_to_h1(_ptr(x), x.numel(), int(scale_exp), _ptr(out), _stream(x.device)), "dgp_f32_to_h1")
    return out


def h1_to_f32(x: torch.Tensor, scale_exp: int) -> torch.Tensor:
    _need_cuda(x, torch.float16, "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dgp_h1_to_f32(_ptr(x), x.numel(), int(scale_exp), _ptr(out), _stream(x.device)), "dgp_h1_to_f32")
    return out


def conv2d_h1(x_h1: torch.Tensor, x_exp: int, w_hwio: np.ndarray, stride: int = 1, rate: int = 1, pad_t: int = 0, pad_l: int = 0,
              out_hw: Optional[Tuple[int, int]] = None, scale=None, bias=None, residual: Optional[torch.Tensor] = None,
              res_stride: int = 0, res_exp: int = 0, relu: bool = False, y_is_h1: bool = True, y_exp: int = 0,
              out: Optional[torch.Tensor] = None):
    """One conv layer on H1 tensors (float16 NHWC with power-of-two scales) through the 16-bit tier's cell kernels.
    -> (y: float16 H1 cells or fp32, y_absmax_slots).  out: as in conv2d (float16 where y_is_h1)."""
    lib = _lib.load()
    _need_cuda(x_h1, torch.float16, "x_h1")
    N, H, W, Cin = x_h1.shape
    kh, kw, cin2, cout = w_hwio.shape
    assert cin2 == Cin
    dev = x_h1.device
    if out_hw is None:
        keh, kew = (kh - 1) * rate + 1, (kw - 1) * rate + 1
        out_hw = ((H + 2 * pad_t - keh) // stride + 1, (W + 2 * pad_l - kew) // stride + 1)
    Ho, Wo = out_hw
    wp = torch.from_numpy(pack_conv_weights(w_hwio)).to(dev)
    sc = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).contiguous().to(dev)
    bi = None if bias is None else torch.as_tensor(bias, dtype=torch.float32).contiguous().to(dev)
    y = _conv_out(out, (N, Ho, Wo, cout), dev, torch.float16 if y_is_h1 else torch.float32)
    if residual is not None:
        _need_cuda(residual, torch.float16, "residual")
    rh, rw = (residual.shape[1], residual.shape[2]) if residual is not None else (0, 0)
    d = _lib.DgpConvDesc(N, H, W, Cin, cout, kh, kw, stride, rate, pad_t, pad_l, Ho, Wo, int(relu),
                         res_stride if residual is not None else 0, rh, rw)
    rng = torch.zeros((2, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    _lib.check(lib.dgp_tensor_absmax(_ptr(wp), wp.numel(), _ptr(rng[0]), _stream(dev)), "dgp_tensor_absmax")
    cells = torch.empty(wp.numel(), dtype=torch.float16, device=dev)
    _lib.check(lib.dgp_conv2d_h1(C.byref(d), _ptr(x_h1), int(x_exp), _ptr(wp), _ptr(rng[0]), _ptr(sc), _ptr(bi), _ptr(residual),
                                 int(res_exp), _ptr(y), int(y_is_h1), int(y_exp), _ptr(rng[1]), _ptr(cells), _stream(dev)),
               "dgp_conv2d_h1")
    return y, rng[1]


def _xout_buffer(xout, shape, dt, dev) -> torch.Tensor:
    """x_out of chain_h2 / unit_h2: a fresh tensor, or the caller's (what it holds shows which pixels a launch left alone)"""
    if xout is None:
        return torch.empty(shape, dtype=dt, device=dev)
    _need_cuda(xout, dt, "xout")
    assert tuple(xout.shape) == tuple(shape) and xout.is_contiguous() and xout.device == dev
    return xout


def chain_h2(r2_h2: torch.Tensor, r2_exp: int, src2_h2: torch.Tensor, src2_exp: int, w3cat: np.ndarray, scale3, bias3,
             w1: np.ndarray, scale1, bias1, res_mode: int, xout_exp: int, r1_exp: int, h1: bool = False, xout_keep: int = 1,
             xout: Optional[torch.Tensor] = None):
    """The engine's chain kernel at layer level (include/dgp_hip.h, dgp_chain_h2): conv3 (+ shortcut, ReLU) of a bottleneck unit and
    conv1 of the next unit in one launch.  r2 [N, Ho, Wo, C]; src2: X [N, Ho, Wo, 4C] (res_mode 1), X [N, H, W, 4C] read at (2 ho, 2 wo)
    (res_mode 2) or the shortcut conv's input [N, Ho, Wo, CIN2] (res_mode 0; w3cat then has C + CIN2 rows).
    -> (x_out H2, r1 H2, x_out range slots, r1 range slots).  h1: every tensor is an H1 tensor (torch.float16 [N, H, W, C]; dgp_chain_h1).
    xout_keep=2 (dgp_chain_xkeep): x_out is written at [:, ::2, ::2] only, as by the engine's launch in front of a stride-2 subsample
    unit; the other pixels keep what `xout` (a caller's buffer of x_out's shape; default: a fresh one) held.  Ranges and r1 cover every pixel."""
    lib = _lib.load()
    dt = torch.float16 if h1 else torch.float32
    _need_cuda(r2_h2, dt, "r2_h2")
    _need_cuda(src2_h2, dt, "src2_h2")
    N, Ho, Wo, Cc = r2_h2.shape
    K, C4 = w3cat.shape
    C1 = w1.shape[1]
    assert C4 == 4 * Cc and w1.shape[0] == C4
    cin2 = K - Cc
    dev = r2_h2.device
    xo = _xout_buffer(xout, (N, Ho, Wo, C4), dt, dev)
    r1 = torch.empty((N, Ho, Wo, C1), dtype=dt, device=dev)
    rng = torch.zeros((2, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    w3c, s3, b3, w1c, s1, b1 = f(w3cat), f(scale3), f(bias3), f(w1), f(scale1), f(bias1)
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    args = (N, Ho, Wo, Cc, C1, cin2, int(res_mode), src2_h2.shape[1], src2_h2.shape[2], _ptr(r2_h2), int(r2_exp),
            _ptr(src2_h2), int(src2_exp), hp(w3c), hp(s3), hp(b3), hp(w1c), hp(s1), hp(b1), _ptr(xo), int(xout_exp),
            _ptr(r1), int(r1_exp), _ptr(rng[0]), _ptr(rng[1]), _stream(dev))
    if xout_keep == 1:
        _lib.check((lib.dgp_chain_h1 if h1 else lib.dgp_chain_h2)(*args), "dgp_chain_h2")
    else:
        _lib.check(lib.dgp_chain_xkeep(int(h1), int(xout_keep), *args), "dgp_chain_xkeep")
    return xo, r1, rng[0], rng[1]


def unit_h2(r1_h2: torch.Tensor, r1_exp: int, src2_h2: torch.Tensor, src2_exp: int, w2: np.ndarray, scale2, bias2, r2_exp: int,
            w3cat: np.ndarray, scale3, bias3, w1: np.ndarray, scale1, bias1, res_mode: int, xout_exp: int, r1out_exp: int, h1: bool = False,
            xout_keep: int = 1, xout: Optional[torch.Tensor] = None):
    """The engine's unit kernel at layer level (include/dgp_hip.h, dgp_unit_h2): conv2 (3x3, stride 1) + conv3 (+ shortcut, ReLU) of a
    bottleneck unit and conv1 of the next unit in one launch.  r1 [N, H, W, C] is conv2's input; w2 HWIO [3, 3, C, C].
    -> (x_out H2, r1_out H2, r2 range slots, x_out range slots, r1_out range slots).  h1: H1 tensors (torch.float16; dgp_unit_h1).
    xout_keep / xout: as for chain_h2 (dgp_unit_xkeep)."""
    lib = _lib.load()
    dt = torch.float16 if h1 else torch.float32
    _need_cuda(r1_h2, dt, "r1_h2")
    _need_cuda(src2_h2, dt, "src2_h2")
    N, H, W, Cc = r1_h2.shape
    K, C4 = w3cat.shape
    C1 = w1.shape[1]
    assert C4 == 4 * Cc and w1.shape[0] == C4 and w2.shape == (3, 3, Cc, Cc)
    cin2 = K - Cc
    dev = r1_h2.device
    xo = _xout_buffer(xout, (N, H, W, C4), dt, dev)
    r1o = torch.empty((N, H, W, C1), dtype=dt, device=dev)
    rng = torch.zeros((3, ABSMAX_SLOTS), dtype=torch.float32, device=dev)
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    arrs = [f(a) for a in (w2, scale2, bias2, w3cat, scale3, bias3, w1, scale1, bias1)]
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    args = (N, H, W, Cc, C1, cin2, int(res_mode), _ptr(r1_h2), int(r1_exp), _ptr(src2_h2), int(src2_exp),
            hp(arrs[0]), hp(arrs[1]), hp(arrs[2]), int(r2_exp), hp(arrs[3]), hp(arrs[4]), hp(arrs[5]), hp(arrs[6]),
            hp(arrs[7]), hp(arrs[8]), _ptr(xo), int(xout_exp), _ptr(r1o), int(r1out_exp), _ptr(rng[0]), _ptr(rng[1]),
            _ptr(rng[2]), _stream(dev))
    if xout_keep == 1:
        _lib.check((lib.dgp_unit_h1 if h1 else lib.dgp_unit_h2)(*args), "dgp_unit_h2")
    else:
        _lib.check(lib.dgp_unit_xkeep(int(h1), int(xout_keep), *args), "dgp_unit_xkeep")
    return xo, r1o, rng[0], rng[1], rng[2]


def maxpool_3x3s2_same(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need_cuda(x, torch.float32, "x")
    N, H, W, Cn = x.shape
    y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, Cn), dtype=torch.float32, device=x.device)
    _lib.check(lib.dgp_maxpool_3x3s2_same(_ptr(x), N, H, W, Cn, _ptr(y), _stream(x.device)), "dgp_maxpool")
    return y


def preprocess_u8(frames: torch.Tensor, mean=MEAN_PIXEL) -> torch.Tensor:
    lib = _lib.load()
    _need_cuda(frames, torch.uint8, "frames")
    out = torch.empty(tuple(frames.shape[:-1]) + (4,), dtype=torch.float32, device=frames.device)
    m = (C.c_float * 3)(*mean)
    _lib.check(lib.dgp_preprocess_u8(_ptr(frames), frames.numel() // 3, m, _ptr(out), _stream(frames.device)),
               "dgp_preprocess_u8")
    return out


def motion_energy(frames: torch.Tensor, prev: Optional[torch.Tensor] = None) -> np.ndarray:
    """Motion energy of a device-resident uint8 frame sequence [T, ...] (DGP/dataset.py:29-43):
    me[t] = mean over the frame of (f_t - f_{t-1}) mod 256 (the reference's uint8 subtraction wraps), me[0] = 0 unless `prev`
    (the last frame of the previous chunk) is given.  Integer sums on the device (dgp_motion_energy), float64 division here:
    bit-identical to the reference's np.mean."""
    lib = _lib.load()
    _need_cuda(frames, torch.uint8, "frames")
    frames = frames.contiguous()
    T = frames.shape[0]
    fb = frames.numel() // max(T, 1)
    if T == 0:
        return np.zeros(0, dtype=np.float64)
    if prev is not None:
        _need_cuda(prev, torch.uint8, "prev")
        prev = prev.contiguous()
        if prev.numel() != fb:
            raise _lib.DgpError("motion_energy: prev has %d bytes, a frame has %d" % (prev.numel(), fb))
    sums = torch.empty(T, dtype=torch.int64, device=frames.device)
    _lib.check(lib.dgp_motion_energy(_ptr(frames), fb, T, _ptr(prev), _ptr(sums), _stream(frames.device)), "dgp_motion_energy")
    return sums.cpu().numpy().astype(np.float64) / float(fb)


FLOW_OUTPUTS = ("magnitude", "flow", "both")


def optical_flow(frames: torch.Tensor, *, pyr_scale: float = 0.5, levels: int = 3, winsize: int = 15, iterations: int = 3,
                 poly_n: int = 5, poly_sigma: float = 1.2, output: str = "magnitude"):
    """Farneback flow between consecutive frames of a device uint8 BGR sequence [T, H, W, 3] (dgp_optical_flow; replaces
    cv2.calcOpticalFlowFarneback in learn_wt, DGP/models/fitdgp_util.py:454-467, whose parameters are the defaults here).
    output "magnitude": [T-1, H, W] fp32 = |dx| + |dy| (the temporal clique's vector_field); "flow": [T-1, H, W, 2] (dx, dy); "both": the
    pair (magnitude, flow).  Enqueued on the current stream, no host synchronisation; T < 2 gives empty tensors."""
    lib = _lib.load()
    if output not in FLOW_OUTPUTS:
        raise ValueError("optical_flow: output must be one of %s, not %r" % ("|".join(FLOW_OUTPUTS), output))
    _need_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise _lib.DgpError("optical_flow: frames must be [T, H, W, 3], got %s" % (tuple(frames.shape),))
    T, H, W = (int(v) for v in frames.shape[:3])
    P = max(T - 1, 0)
    dev = frames.device
    mag = torch.empty((P, H, W), dtype=torch.float32, device=dev) if output in ("magnitude", "both") else None
    flow = torch.empty((P, H, W, 2), dtype=torch.float32, device=dev) if output in ("flow", "both") else None
    if P > 0:
        prm = _lib.DgpFlowParams(float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n), float(poly_sigma), 0)
        nb, used = C.c_size_t(), C.c_int32()
        _lib.check(lib.dgp_optical_flow_scratch_bytes(T, H, W, C.byref(prm), C.byref(nb), C.byref(used)), "dgp_optical_flow_scratch_bytes")
        scratch = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        _lib.check(lib.dgp_optical_flow(_ptr(frames), T, H, W, C.byref(prm), _ptr(flow), _ptr(mag), _ptr(scratch), nb.value,
                                        _stream(dev)), "dgp_optical_flow")
    if output == "magnitude":
        return mag
    if output == "flow":
        return flow
    return mag, flow


# resize plans kept on the device: (device, H, W, rows, cols) -> (plan_x, plan_y, ksize_x, ksize_y); a project's videos share one frame size
_RESIZE_PLANS: Dict[tuple, tuple] = {}


def resize_plan(in_size: int, out_size: int) -> Tuple[int, np.ndarray, np.ndarray]:
    """Pillow's bicubic tables of one axis (dgp_resize_plan, host only): (ksize, bounds int32 [out, 2] = (first input, taps),
    coeffs int32 [out, ksize], zero-padded)."""
    lib = _lib.load()
    ks = C.c_int32()
    _lib.check(lib.dgp_resize_plan_size(int(in_size), int(out_size), C.byref(ks)), "dgp_resize_plan_size")
    bounds = np.empty((int(out_size), 2), np.int32)
    coeffs = np.empty((int(out_size), ks.value), np.int32)
    _lib.check(lib.dgp_resize_plan(int(in_size), int(out_size), bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p)),
               "dgp_resize_plan")
    return ks.value, bounds, coeffs


def _device_resize_plans(dev, H: int, W: int, rh: int, rw: int):
    key = (str(dev), H, W, rh, rw)
    if key not in _RESIZE_PLANS:
        plans = []
        for n_in, n_out in ((W, rw), (H, rh)):
            ks, bounds, coeffs = resize_plan(n_in, n_out)
            plans.append((torch.from_numpy(np.concatenate([bounds.ravel(), coeffs.ravel()])).to(dev), ks))
        if len(_RESIZE_PLANS) >= 16:               # a handful of sizes per process; never grows without bound
            # drop the oldest entry only.  Its tables were allocated on the default stream and a resize queued on any other stream may
            # still read them, so the device is drained before the block can go back to the allocator (the 17th size of a process: rare)
            old = next(iter(_RESIZE_PLANS))
            torch.cuda.synchronize(_RESIZE_PLANS[old][0].device)
            del _RESIZE_PLANS[old]
        _RESIZE_PLANS[key] = (plans[0][0], plans[1][0], plans[0][1], plans[1][1])
    return _RESIZE_PLANS[key]


def resize_output_shape(H: int, W: int, new_size=None, crop_size=None) -> Tuple[int, int]:
    """(rows, cols) of a frame after Image.resize(size=(new_size[1], new_size[0])) and Image.crop(crop_size)"""
    oh, ow = (int(new_size[0]), int(new_size[1])) if new_size is not None else (int(H), int(W))
    if crop_size is not None:
        l, u, r, b = (int(round(v)) for v in crop_size)
        oh, ow = b - u, r - l
    return oh, ow


def resize_frames(frames: torch.Tensor, new_size=None, crop_size=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Resize and / or crop a device uint8 RGB batch [B, H, W, 3] as estimate_pose's host preparation does per frame
    (DGP/models/eval.py:307-326): Image.resize(size=(new_size[1], new_size[0])) -- Pillow's antialiased BICUBIC -- then
    Image.crop(crop_size), crop_size = (left, upper, right, lower) in the resized image, zeros outside it.  One dgp_resize_crop_u8 launch
    on the current stream, no host synchronisation after the first call of a size (the tables are built on the host and uploaded once);
    the bytes are Pillow's.  Returns uint8 [B, oh, ow, 3]; `out` (that shape, contiguous) is filled in place and returned."""
    lib = _lib.load()
    _need_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise _lib.DgpError("resize_frames: frames must be [B, H, W, 3], got %s" % (tuple(frames.shape),))
    if new_size is not None and len(new_size) != 2:
        raise ValueError("resize_frames: new_size must be (rows, cols), not %r" % (new_size,))
    if crop_size is not None and len(crop_size) != 4:
        raise ValueError("resize_frames: crop_size must be (left, upper, right, lower), not %r" % (crop_size,))
    B, H, W = (int(v) for v in frames.shape[:3])
    rh, rw = (int(new_size[0]), int(new_size[1])) if new_size is not None else (H, W)
    oh, ow = resize_output_shape(H, W, new_size, crop_size)
    if min(rh, rw, oh, ow) <= 0:
        raise ValueError("resize_frames: empty result for new_size %r, crop_size %r" % (new_size, crop_size))
    dev = frames.device
    if out is None:
        out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
    else:
        _need_cuda(out, torch.uint8, "out")
        if tuple(out.shape) != (B, oh, ow, 3) or out.device != dev:
            raise _lib.DgpError("resize_frames: out must be %s on %s, got %s on %s" % ((B, oh, ow, 3), dev, tuple(out.shape), out.device))
    plan_x, plan_y, ksx, ksy = _device_resize_plans(dev, H, W, rh, rw)
    box = (C.c_int32 * 4)(*(int(round(v)) for v in crop_size)) if crop_size is not None else None
    _lib.check(lib.dgp_resize_crop_u8(_ptr(frames), B, H, W, rh, rw, box, _ptr(out), _ptr(plan_x), _ptr(plan_y), ksx, ksy, _stream(dev)),
               "dgp_resize_crop_u8")
    return out


RESIZE_FILTERS = {"box": 4, "bilinear": 2, "bicubic": 3}         # Pillow's Image.BOX / BILINEAR / BICUBIC (include/dgp_hip.h, DGP_FILTER_*)


def _filter_id(filter) -> int:
    if filter in RESIZE_FILTERS:
        return RESIZE_FILTERS[filter]
    if filter in RESIZE_FILTERS.values():
        return int(filter)
    raise ValueError("resize filter must be one of %s, not %r" % ("|".join(RESIZE_FILTERS), filter))


def resize_plan_f(in_size: int, out_size: int, filter) -> Tuple[int, np.ndarray, np.ndarray]:
    """Pillow's tables of one axis for the BOX, BILINEAR or BICUBIC filter (dgp_resize_plan_f, host only), as resize_plan returns them."""
    lib = _lib.load()
    fid = _filter_id(filter)
    ks = C.c_int32()
    _lib.check(lib.dgp_resize_plan_size_f(int(in_size), int(out_size), fid, C.byref(ks)), "dgp_resize_plan_size_f")
    bounds = np.empty((int(out_size), 2), np.int32)
    coeffs = np.empty((int(out_size), ks.value), np.int32)
    _lib.check(lib.dgp_resize_plan_f(int(in_size), int(out_size), fid, bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p)),
               "dgp_resize_plan_f")
    return ks.value, bounds, coeffs


def window_resize(image: torch.Tensor, window, out_hw, filter="box", mirror: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inclusive window (x0, y0, x1, y1) of ONE device uint8 RGB image [H, W, 3] (None: the whole image), resampled to out_hw =
    (rows, cols) with Pillow's `filter` ("box" | "bilinear" | "bicubic") and, with `mirror`, flipped left to right: what the step-0
    loader's crop_image + imresize (+ np.fliplr) give (dlc_dataset.py), the bytes Pillow's.  The window is read in place.  One
    dgp_window_resize_u8 launch on the current stream; the two tables are built on the host and uploaded in one small copy (samples
    differ in size from one to the next, so they are not kept).  Returns uint8 [rows, cols, 3]; `out` (that shape, contiguous, not
    overlapping the image) is filled in place and returned."""
    lib = _lib.load()
    _need_cuda(image, torch.uint8, "image")
    if image.dim() != 3 or image.shape[-1] != 3:
        raise _lib.DgpError("window_resize: image must be [H, W, 3], got %s" % (tuple(image.shape),))
    H, W = int(image.shape[0]), int(image.shape[1])
    x0, y0, x1, y1 = (0, 0, W - 1, H - 1) if window is None else (int(v) for v in window)
    rh, rw = int(out_hw[0]), int(out_hw[1])
    if not (0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H) or rh <= 0 or rw <= 0:
        raise _lib.DgpError("window_resize: window %r / output %r do not fit a %d x %d image" % (window, out_hw, H, W))
    fid = _filter_id(filter)
    dev = image.device
    ksx, bx, cx = resize_plan_f(x1 - x0 + 1, rw, fid)
    ksy, by, cy = resize_plan_f(y1 - y0 + 1, rh, fid)
    nx = bx.size + cx.size
    plans = torch.from_numpy(np.concatenate([bx.ravel(), cx.ravel(), by.ravel(), cy.ravel()])).to(dev)
    if out is None:
        out = torch.empty((rh, rw, 3), dtype=torch.uint8, device=dev)
    else:
        _need_cuda(out, torch.uint8, "out")
        if tuple(out.shape) != (rh, rw, 3) or out.device != dev:
            raise _lib.DgpError("window_resize: out must be %s on %s, got %s on %s" % ((rh, rw, 3), dev, tuple(out.shape), out.device))
    _lib.check(lib.dgp_window_resize_u8(_ptr(image), H, W, x0, y0, x1, y1, rh, rw, fid, 1 if mirror else 0, _ptr(out), _ptr(plans),
                                        C.c_void_p(plans.data_ptr() + 4 * nx), ksx, ksy, _stream(dev)), "dgp_window_resize_u8")
    return out


def _target_out(given, shape, dev, name):
    """an output of target_maps: None / False -> not computed, True -> allocated, a tensor -> filled in place"""
    if given is None or given is False:
        return None
    if given is True:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    _need_cuda(given, torch.float32, name)
    if tuple(given.shape) != tuple(shape) or given.device != dev:
        raise _lib.DgpError("target_maps: %s must be %s on %s, got %s on %s" % (name, tuple(shape), dev, tuple(given.shape), given.device))
    return given


def target_maps(entries, offsets, n: int, H: int, W: int, nj: int, *, pos_dist_thresh: float, stride: float = 8.0, scale: float = 1.0,
                locref_stdev: float = 7.2801, weigh_only_present_joints: bool = False, scmap=True, weights=True, lmap=True, lmask=True,
                device=None):
    """DLC's target maps of n frames on the device (dgp_target_maps; the host counterpart is dataset.compute_target_part_scoremap).
    entries: float64 [k, 3] = (joint id, x, y) in the host function's person-then-joint order; offsets: int32 [n + 1], frame f owns
    entries[offsets[f]:offsets[f + 1]].  -> (scmap [n, H, W, nj], weights [n, H, W, nj], lmap [n, H, W, 2 nj], lmask [n, H, W, 2 nj]),
    fp32 device tensors written on the current stream: the host function's float64 values cast to fp32, every cell written.  Each of
    the four keywords selects its output: True allocates it, a tensor of that shape is filled in place, None leaves it out (its place in
    the result is None).  Bad entries or offsets raise before anything is launched."""
    lib = _lib.load()
    ent = np.ascontiguousarray(np.asarray(entries, dtype=np.float64).reshape(-1, 3))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32).reshape(-1))
    n, H, W, nj = int(n), int(H), int(W), int(nj)
    if off.size != n + 1 or n <= 0:
        raise _lib.DgpError("target_maps: offsets must have n + 1 = %d values, got %d" % (n + 1, off.size))
    if int(off[-1]) != ent.shape[0]:
        raise _lib.DgpError("target_maps: offsets end at %d but there are %d entries" % (int(off[-1]), ent.shape[0]))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    host = np.concatenate([ent.ravel().view(np.uint8), off.view(np.uint8)])      # one small copy: the doubles first (8-byte aligned)
    packed = torch.from_numpy(host).to(dev)
    outs = [_target_out(g, (n, H, W, c), dev, name) for g, c, name in
            ((scmap, nj, "scmap"), (weights, nj, "weights"), (lmap, 2 * nj, "lmap"), (lmask, 2 * nj, "lmask"))]
    _lib.check(lib.dgp_target_maps(_ptr(packed), C.c_void_p(packed.data_ptr() + ent.nbytes), ent.ctypes.data_as(C.c_void_p),
                                   off.ctypes.data_as(C.c_void_p), n, H, W, nj, float(stride), float(pos_dist_thresh), float(scale),
                                   float(locref_stdev), 1 if weigh_only_present_joints else 0, *(_ptr(t) for t in outs), _stream(dev)),
               "dgp_target_maps")
    return tuple(outs)


class FrameSlots(NamedTuple):
    """Frames kept on the device for gather_frames: `data` uint8 [n_slots, slot_stride], slot s holds one [H, W, 3] frame in its first
    H * W * 3 bytes; slot_stride (bytes) is a multiple of 16.  `shape` = (H, W)."""
    data: torch.Tensor
    shape: Tuple[int, int]


def gather_frames(store, src, patch: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A batch of frames assembled on the device (dgp_gather_frames_u8): out[f] = slot src[f] of `store` (a FrameSlots, or any
    (data, (H, W)) pair) when src[f] >= 0, frame -1 - src[f] of `patch` (uint8 [m, H, W, 3]: the frames uploaded for this batch) otherwise.
    `src` is a HOST sequence of nt ints; every entry is checked against the store's slots and the patch's frames HERE and a bad one
    raises DgpError before anything is launched; the table then travels inside the launch arguments, so no copy is issued for it.
    -> uint8 [nt, H, W, 3] (`out` when given: contiguous, that shape), written by one launch on the current stream; nt == 0 returns an
    empty batch without a launch."""
    lib = _lib.load()
    data, (H, W) = store
    H, W = int(H), int(W)
    frame_bytes = H * W * 3
    _need_cuda(data, torch.uint8, "store")
    if data.dim() != 2 or H <= 0 or W <= 0:
        raise _lib.DgpError("gather_frames: the store must be [n_slots, slot_stride] with a positive frame shape, got %s, %r"
                            % (tuple(data.shape), (H, W)))
    n_slots, stride = int(data.shape[0]), int(data.shape[1])
    if stride % 16 != 0 or stride < frame_bytes:
        raise _lib.DgpError("gather_frames: slot_stride %d must be a multiple of 16 and hold a %d-byte frame" % (stride, frame_bytes))
    dev = data.device
    m = 0
    if patch is not None:
        _need_cuda(patch, torch.uint8, "patch")
        if patch.dim() != 4 or tuple(patch.shape[1:]) != (H, W, 3) or patch.device != dev:
            raise _lib.DgpError("gather_frames: patch must be [m, %d, %d, 3] on %s, got %s on %s" % (H, W, dev, tuple(patch.shape), patch.device))
        m = int(patch.shape[0])
    table = np.asarray(src, dtype=np.int64).reshape(-1)
    nt = int(table.size)
    bad = np.nonzero((table >= n_slots) | (table < -m))[0]
    if bad.size:
        raise _lib.DgpError("gather_frames: src[%d] = %d is outside the store's %d slots and the patch's %d frames"
                            % (int(bad[0]), int(table[bad[0]]), n_slots, m))
    if out is None:
        out = torch.empty((nt, H, W, 3), dtype=torch.uint8, device=dev)
    else:
        _need_cuda(out, torch.uint8, "out")
        if tuple(out.shape) != (nt, H, W, 3) or out.device != dev:
            raise _lib.DgpError("gather_frames: out must be %s on %s, got %s on %s" % ((nt, H, W, 3), dev, tuple(out.shape), out.device))
    if nt == 0:
        return out
    table = np.ascontiguousarray(table, dtype=np.int32)
    _lib.check(lib.dgp_gather_frames_u8(_ptr(data) if n_slots else None, n_slots, stride, _ptr(patch) if m else None, m,
                                        table.ctypes.data_as(C.c_void_p), nt, frame_bytes, _ptr(out), _stream(dev)),
               "dgp_gather_frames_u8")
    return out


# ---- frame selection (csrc/dgp_select.hip): thumbnails of device frames and the three k-means kernels; frame_selection.py drives them

from .frame_selection import KMEANS_MAX_K, KMEANS_MAX_D, feature_geometry  # noqa: E402  (torch-free: the limits and the thumbnail geometry)


def frame_features(frames_u8: torch.Tensor, resizewidth: int = 30, color: bool = False, crop=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Area-averaged thumbnails of device uint8 frames [N, H, W, 3] (dgp_frame_features_u8; the resize of
    KmeansbasedFrameselectioncv2, frameselectiontools.py:173-228): float32 [N, D], geometry as feature_geometry, grey = the box mean over
    pixels and channels laid out [oh, ow], color = one mean per channel laid out [oh, 3, ow] (the reference's hstack, :188).  Integer sums,
    one division: float32(float64(sum) / count), bit for bit frame_selection.features_host.  `frames_u8` may be a view: each frame
    contiguous, frames any stride >= H W 3 apart, at any byte offset.  `out`: float32 [N, D] whose rows may be a view into a wider buffer
    (unit column stride); only the N x D values are written.  One launch on the current stream, no host synchronisation."""
    lib = _lib.load()
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8:
        raise _lib.DgpError("frame_features: frames must be a device uint8 tensor")
    if frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise _lib.DgpError("frame_features: frames must be [N, H, W, 3], got %s" % (tuple(frames_u8.shape),))
    N, H, W = (int(v) for v in frames_u8.shape[:3])
    if H < 1 or W < 1:
        raise ValueError("frame_features: empty frames %s" % (tuple(frames_u8.shape),))
    x1, x2, y1, y2, oh, ow, D = feature_geometry(H, W, resizewidth, color, crop)
    if N and not frames_u8[0].is_contiguous():
        raise _lib.DgpError("frame_features: each frame must be contiguous")
    fstride = int(frames_u8.stride(0)) if N > 1 else H * W * 3
    if fstride < H * W * 3:
        raise _lib.DgpError("frame_features: frames overlap (stride %d < %d bytes)" % (fstride, H * W * 3))
    dev = frames_u8.device
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
    else:
        if not out.is_cuda or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (N, D):
            raise _lib.DgpError("frame_features: out must be float32 %s on %s, got %s %s on %s" % ((N, D), dev, out.dtype, tuple(out.shape), out.device))
        if (D > 1 and out.stride(1) != 1) or (N > 1 and out.stride(0) < D):
            raise _lib.DgpError("frame_features: out needs unit column stride and a row stride >= %d, got %s" % (D, tuple(out.stride())))
    if N == 0:
        return out
    ostride = int(out.stride(0)) if N > 1 else D
    _lib.check(lib.dgp_frame_features_u8(_ptr(frames_u8), N, H, W, fstride, x1, x2, y1, y2, ow, oh, int(bool(color)), _ptr(out), ostride,
                                         _stream(dev)), "dgp_frame_features_u8")
    return out


def _kmeans_matrix(X: torch.Tensor, who: str, k: Optional[int] = None) -> Tuple[int, int]:
    _need_cuda(X, torch.float32, "X")
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("%s: X must be a non-empty [N, D] matrix, got %s" % (who, tuple(X.shape)))
    N, D = int(X.shape[0]), int(X.shape[1])
    if D > KMEANS_MAX_D:
        raise ValueError("%s: D = %d is above the limit of %d columns" % (who, D, KMEANS_MAX_D))
    if N * D >= 1 << 31:
        raise ValueError("%s: N x D = %d must stay below 2^31" % (who, N * D))
    if k is not None and not 1 <= k <= KMEANS_MAX_K:
        raise ValueError("%s: k = %d is outside 1 .. %d" % (who, k, KMEANS_MAX_K))
    return N, D


def _kmeans_scratch(lib, N: int, D: int, k: int, dev) -> torch.Tensor:
    return torch.empty((int(lib.dgp_kmeans_scratch_bytes(N, D, k)) + 7) // 8, dtype=torch.float64, device=dev)


def kmeans_center(X: torch.Tensor) -> torch.Tensor:
    """X float32 [N, D] on the device, centred IN PLACE: DATA - DATA.mean(axis=0) (frameselectiontools.py:231).  Column sums in double
    over fixed slabs of rows combined in slab order, the mean rounded once to fp32, then float32(x - mean32).  -> mean float32 [D].
    Enqueued on the current stream (dgp_kmeans_center)."""
    lib = _lib.load()
    N, D = _kmeans_matrix(X, "kmeans_center")
    mean = torch.empty(D, dtype=torch.float32, device=X.device)
    scratch = _kmeans_scratch(lib, N, D, 0, X.device)
    _lib.check(lib.dgp_kmeans_center(_ptr(X), N, D, _ptr(mean), _ptr(scratch), scratch.numel() * 8, _stream(X.device)), "dgp_kmeans_center")
    return mean


def kmeans_assign(X: torch.Tensor, C_: torch.Tensor, labels: torch.Tensor, dist: torch.Tensor) -> int:
    """Nearest centre of every row of X [N, D] among C_ [k, D] (dgp_kmeans_assign): labels int32 [N] is read (the previous labels) and
    overwritten, dist float32 [N] gets the squared distance to the chosen centre, fp32 sums of (x - c)^2 in a fixed order; the lowest
    index wins a tie.  -> the number of rows whose label changed (an exact integer; reading it synchronises)."""
    lib = _lib.load()
    _need_cuda(C_, torch.float32, "C")
    if C_.dim() != 2:
        raise ValueError("kmeans_assign: C must be [k, D], got %s" % (tuple(C_.shape),))
    N, D = _kmeans_matrix(X, "kmeans_assign", int(C_.shape[0]))
    _need_cuda(labels, torch.int32, "labels")
    _need_cuda(dist, torch.float32, "dist")
    if int(C_.shape[1]) != D or tuple(labels.shape) != (N,) or tuple(dist.shape) != (N,):
        raise ValueError("kmeans_assign: X %s, C %s, labels %s and dist %s do not belong together"
                         % (tuple(X.shape), tuple(C_.shape), tuple(labels.shape), tuple(dist.shape)))
    changed = torch.empty(1, dtype=torch.int32, device=X.device)
    _lib.check(lib.dgp_kmeans_assign(_ptr(X), N, D, _ptr(C_), int(C_.shape[0]), _ptr(labels), _ptr(dist), _ptr(changed), _stream(X.device)),
               "dgp_kmeans_assign")
    return int(changed.item())


def kmeans_update(X: torch.Tensor, labels: torch.Tensor, C_: torch.Tensor, counts: torch.Tensor) -> None:
    """Every centre of C_ [k, D] becomes the mean of its members in place (dgp_kmeans_update): double sums in a fixed order, so two calls
    give the same bits; an empty cluster keeps its centre.  counts int32 [k + 1]: the members of each cluster, and in counts[k] the
    labels outside [0, k) -- those rows are skipped, and a non-zero count raises ValueError here (which synchronises)."""
    lib = _lib.load()
    _need_cuda(C_, torch.float32, "C")
    if C_.dim() != 2:
        raise ValueError("kmeans_update: C must be [k, D], got %s" % (tuple(C_.shape),))
    k = int(C_.shape[0])
    N, D = _kmeans_matrix(X, "kmeans_update", k)
    _need_cuda(labels, torch.int32, "labels")
    _need_cuda(counts, torch.int32, "counts")
    if int(C_.shape[1]) != D or tuple(labels.shape) != (N,) or tuple(counts.shape) != (k + 1,):
        raise ValueError("kmeans_update: X %s, C %s, labels %s and counts %s do not belong together"
                         % (tuple(X.shape), tuple(C_.shape), tuple(labels.shape), tuple(counts.shape)))
    scratch = _kmeans_scratch(lib, N, D, k, X.device)
    _lib.check(lib.dgp_kmeans_update(_ptr(X), N, D, _ptr(labels), _ptr(C_), k, _ptr(counts), _ptr(scratch), scratch.numel() * 8,
                                     _stream(X.device)), "dgp_kmeans_update")
    bad = int(counts[k].item())
    if bad:
        raise ValueError("kmeans_update: %d labels are outside [0, %d)" % (bad, k))


# ---- the augmenters of the DGP drivers' labeled frames (csrc/dgp_augment.hip): one frame, one stage, one launch on the current stream

def _aug_pair(src: torch.Tensor, dst: torch.Tensor, who: str):
    _need_cuda(src, torch.uint8, "src")
    _need_cuda(dst, torch.uint8, "dst")
    if src.dim() != 3 or src.shape[-1] != 3 or src.shape != dst.shape or src.device != dst.device:
        raise _lib.DgpError("%s: src and dst must be [H, W, 3] frames of one shape on one device, got %s and %s"
                            % (who, tuple(src.shape), tuple(dst.shape)))
    return int(src.shape[0]), int(src.shape[1])


def aug_affine(src: torch.Tensor, dst: torch.Tensor, coef) -> torch.Tensor:
    """dst = Image.transform(AFFINE, coef, BILINEAR) of src, Pillow's bytes (dgp_aug_affine_u8).  coef: Pillow's six coefficients;
    (-1, 0, W, 0, 1, 0) is np.fliplr.  src, dst: device uint8 [H, W, 3], distinct."""
    H, W = _aug_pair(src, dst, "aug_affine")
    coef = [float(v) for v in coef]
    if len(coef) != 6:
        raise _lib.DgpError("aug_affine: six coefficients, got %d" % len(coef))
    _lib.check(_lib.load().dgp_aug_affine_u8(_ptr(src), _ptr(dst), H, W, (C.c_double * 6)(*coef), _stream(src.device)), "dgp_aug_affine_u8")
    return dst


def aug_blur3(src: torch.Tensor, dst: torch.Tensor, kernel) -> torch.Tensor:
    """dst = the host motion blur of src with the 3 x 3 fp32 `kernel` (augment.apply_motion_blur's bytes; dgp_aug_blur3_u8)"""
    H, W = _aug_pair(src, dst, "aug_blur3")
    k = np.ascontiguousarray(kernel, dtype=np.float32).reshape(-1)
    if k.size != 9:
        raise _lib.DgpError("aug_blur3: a 3 x 3 kernel, got %d weights" % k.size)
    _lib.check(_lib.load().dgp_aug_blur3_u8(_ptr(src), _ptr(dst), H, W, (C.c_float * 9)(*k.tolist()), _stream(src.device)), "dgp_aug_blur3_u8")
    return dst


def aug_dropout(src: torch.Tensor, dst: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """dst = src with the pixels under the coarse mask zeroed (augment.apply_coarse_dropout's bytes; dgp_aug_dropout_u8).  mask: device
    uint8 [h, w], non-zero = dropped, 1 <= h <= H and 1 <= w <= W."""
    H, W = _aug_pair(src, dst, "aug_dropout")
    _need_cuda(mask, torch.uint8, "mask")
    if mask.dim() != 2 or mask.device != src.device:
        raise _lib.DgpError("aug_dropout: mask must be [h, w] on %s, got %s on %s" % (src.device, tuple(mask.shape), mask.device))
    _lib.check(_lib.load().dgp_aug_dropout_u8(_ptr(src), _ptr(dst), H, W, _ptr(mask), int(mask.shape[0]), int(mask.shape[1]),
                                              _stream(src.device)), "dgp_aug_dropout_u8")
    return dst


def aug_elastic(src: torch.Tensor, dst: torch.Tensor, field: torch.Tensor) -> torch.Tensor:
    """dst[p] = src[p + d(p)], bilinear with zeros outside, d the 4 x bilinear upsampling of the coarse field (dgp_aug_elastic_u8).
    field: device fp32 [2, hc, wc] (dx, dy), hc = ceil((H - 1) / 4) + 1 and wc alike (augment.draw_elastic's)."""
    H, W = _aug_pair(src, dst, "aug_elastic")
    _need_cuda(field, torch.float32, "field")
    if field.dim() != 3 or field.shape[0] != 2 or field.device != src.device:
        raise _lib.DgpError("aug_elastic: field must be [2, hc, wc] on %s, got %s on %s" % (src.device, tuple(field.shape), field.device))
    _lib.check(_lib.load().dgp_aug_elastic_u8(_ptr(src), _ptr(dst), H, W, _ptr(field), int(field.shape[1]), int(field.shape[2]),
                                              _stream(src.device)), "dgp_aug_elastic_u8")
    return dst


def aug_noise(src: torch.Tensor, dst: torch.Tensor, scale: float, per_channel: bool, key: int) -> torch.Tensor:
    """dst = clip(rint(src + scale z)), z standard normal from Philox4x32-10 under the 64-bit `key`, addressed by the element index
    (one z per pixel without per_channel): the same key gives the same bytes whatever the launch shape (dgp_aug_noise_u8)"""
    H, W = _aug_pair(src, dst, "aug_noise")
    key = int(key)
    if not 0 <= key < 2 ** 64:
        raise _lib.DgpError("aug_noise: key must be a uint64, got %r" % (key,))
    _lib.check(_lib.load().dgp_aug_noise_u8(_ptr(src), _ptr(dst), H, W, float(scale), 1 if per_channel else 0, key, _stream(src.device)),
               "dgp_aug_noise_u8")
    return dst


# two scratch frames per (device, H, W): the stages of a plan run from one into the other
_AUG_SCRATCH: Dict[tuple, torch.Tensor] = {}


def _aug_scratch(dev, H: int, W: int) -> torch.Tensor:
    key = (str(dev), H, W)
    if key not in _AUG_SCRATCH:
        if len(_AUG_SCRATCH) >= 16:                # as _RESIZE_PLANS: drop the oldest, after whatever stream still reads it
            old = next(iter(_AUG_SCRATCH))
            torch.cuda.synchronize(_AUG_SCRATCH[old].device)
            del _AUG_SCRATCH[old]
        _AUG_SCRATCH[key] = torch.empty((2, H, W, 3), dtype=torch.uint8, device=dev)
    scratch = _AUG_SCRATCH[key]
    scratch.record_stream(torch.cuda.current_stream(dev))
    return scratch


def _aug_crop_and_pad(src: torch.Tensor, dst: torch.Tensor, params) -> None:
    """CropAndPad(keep_size=True): the core of src, inside zeros where a side pads, resized back by window_resize (Pillow's BILINEAR)"""
    from .augment import crop_geometry
    H, W = int(src.shape[0]), int(src.shape[1])
    x0, x1, y0, y1, pt, pb, pl, pr = crop_geometry(params, H, W)
    if pt or pb or pl or pr:
        padded = torch.zeros((y1 - y0 + pt + pb, x1 - x0 + pl + pr, 3), dtype=torch.uint8, device=src.device)
        padded[pt:pt + y1 - y0, pl:pl + x1 - x0] = src[y0:y1, x0:x1]
        window_resize(padded, None, (H, W), "bilinear", out=dst)
    else:
        window_resize(src, (x0, y0, x1 - 1, y1 - 1), (H, W), "bilinear", out=dst)


def augment_frames(frames: torch.Tensor, plans, positions) -> torch.Tensor:
    """Apply host-drawn augmentation plans (augment.NumpyAugPipeline.plan(H, W, noise="key")) to frames of a device batch, in place:
    plans[i] is the plan of frames[positions[i]].  frames: uint8 [n, H, W, 3].  A plan's stages run one launch each on the current
    stream, chained through two scratch frames kept per (device, H, W); the last one writes frames[position].  The plans' tables (dropout
    masks, elastic fields) go up in one small pinned copy per call.  fliplr, rotate, motion_blur, coarse_dropout and crop_and_pad give
    the bytes of augment.apply_<stage>; elastic is within rounding of the float64 value like the host's fp32 stage; gaussian_noise is a
    different stream from the same distribution as the host's (Philox4x32-10 under the plan's key).  Everything is checked before the
    first launch; a plan built with noise="field" is a ValueError.  An empty plan launches nothing.  Returns `frames`."""
    from .augment import ELASTIC_STEP, STAGES
    _need_cuda(frames, torch.uint8, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise _lib.DgpError("augment_frames: frames must be [n, H, W, 3], got %s" % (tuple(frames.shape),))
    n, H, W = (int(v) for v in frames.shape[:3])
    positions = [int(p) for p in positions]
    plans = list(plans)
    if len(plans) != len(positions):
        raise _lib.DgpError("augment_frames: %d plans for %d positions" % (len(plans), len(positions)))
    if len(set(positions)) != len(positions) or any(not 0 <= p < n for p in positions):
        raise _lib.DgpError("augment_frames: positions %r must be distinct frames of a batch of %d" % (positions, n))
    hc, wc = -(-(H - 1) // ELASTIC_STEP) + 1, -(-(W - 1) // ELASTIC_STEP) + 1
    fields, masks, work = [], [], []
    for plan in plans:                                               # ---- check everything, collect the tables
        ops = []
        for stage, params in plan:
            if stage not in STAGES:
                raise _lib.DgpError("augment_frames: unknown stage %r" % (stage,))
            if stage == "fliplr" and not params["flip"]:
                continue
            table = None
            if stage == "gaussian_noise" and params.get("key") is None:
                raise ValueError("augment_frames: this plan carries the host's noise field; build plans for the device with "
                                 "plan(H, W, noise=\"key\")")
            if stage == "coarse_dropout":
                m = np.ascontiguousarray(params["mask"]).astype(np.uint8)
                if m.ndim != 2 or not (1 <= m.shape[0] <= H and 1 <= m.shape[1] <= W):
                    raise _lib.DgpError("augment_frames: a dropout mask of shape %s does not belong to a %d x %d frame" % (m.shape, H, W))
                table = ("mask", len(masks))
                masks.append(m)
            if stage == "elastic":
                f = np.ascontiguousarray(params["field"], dtype=np.float32)
                if f.shape != (2, hc, wc):
                    raise _lib.DgpError("augment_frames: an elastic field of shape %s does not belong to a %d x %d frame (2, %d, %d)"
                                        % (f.shape, H, W, hc, wc))
                table = ("field", len(fields))
                fields.append(f)
            ops.append((stage, params, table))
        work.append(ops)
    if min(H, W) < 2 and any(work):
        raise _lib.DgpError("augment_frames: frames must be at least 2 x 2, got %d x %d" % (H, W))
    dev = frames.device
    dev_fields, dev_masks = [], []
    if fields or masks:                                              # ---- one pinned copy: the fp32 fields first, then the masks
        host = np.concatenate([f.ravel().view(np.uint8) for f in fields] + [m.ravel() for m in masks])
        pinned = torch.empty(host.size, dtype=torch.uint8).pin_memory()
        pinned.numpy()[...] = host
        packed = pinned.to(dev, non_blocking=True)
        at = 0
        for f in fields:
            dev_fields.append(packed[at:at + f.nbytes].view(torch.float32).view(f.shape))
            at += f.nbytes
        for m in masks:
            dev_masks.append(packed[at:at + m.size].view(m.shape))
            at += m.size
    scratch = _aug_scratch(dev, H, W) if any(work) else None
    for ops, pos in zip(work, positions):                            # ---- the launches
        frame = frames[pos]
        src = frame
        if len(ops) == 1:                                            # no stage runs in place: a lone stage reads a copy
            src = scratch[0].copy_(frame)
        for i, (stage, params, table) in enumerate(ops):
            dst = frame if i == len(ops) - 1 else scratch[i % 2]
            if stage == "fliplr":
                aug_affine(src, dst, (-1.0, 0.0, float(W), 0.0, 1.0, 0.0))
            elif stage == "rotate":
                aug_affine(src, dst, params["coef"])
            elif stage == "motion_blur":
                aug_blur3(src, dst, params["kernel"])
            elif stage == "coarse_dropout":
                aug_dropout(src, dst, dev_masks[table[1]])
            elif stage == "elastic":
                aug_elastic(src, dst, dev_fields[table[1]])
            elif stage == "gaussian_noise":
                aug_noise(src, dst, params["scale"], params["per_channel"], params["key"])
            else:
                _aug_crop_and_pad(src, dst, params)
            src = dst
    return frames


# ---- baseline JPEG frames (csrc/dgp_jpeg_host.h + csrc/dgp_jpeg.hip): the host half lives in jpeg.py (no torch), re-exported here
from .jpeg import probe as jpeg_probe, entropy_decode as jpeg_entropy_decode, SAMPLING_NAMES as JPEG_SAMPLING_NAMES  # noqa: E402


def jpeg_block_count(H: int, W: int, sampling: int) -> Tuple[int, int]:
    """(total_blocks, ncomp) of a frame: coefficients are int16 [total_blocks, 64], tables uint16 [ncomp, 64]"""
    hs, vs = (2 if sampling in (2, 3) else 1), (2 if sampling == 3 else 1)
    mx, my = -(-int(W) // (8 * hs)), -(-int(H) // (8 * vs))
    return (mx * my * hs * vs, 1) if sampling == 0 else (mx * my * (hs * vs + 2), 3)


def jpeg_reconstruct(coef: torch.Tensor, qt: torch.Tensor, H: int, W: int, sampling: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dgp_jpeg_reconstruct_u8: B frames of ONE geometry from their entropy-decoded coefficients.  coef: device int16
    [B, total_blocks, 64] (or flat per frame), qt: device int16 / uint16 [B, ncomp, 64] (the bits of jpeg_entropy_decode's uint16
    tables), both contiguous.  -> uint8 [B, H, W, 3], Pillow's bytes; `out` (that shape, each frame contiguous, frames any whole number
    of bytes >= H W 3 apart: a slice of a larger buffer) is written in place and nothing around it is touched.  Two launches on the
    current stream; the planar scratch comes from torch's allocator on that stream."""
    lib = _lib.load()
    H, W, sampling = int(H), int(W), int(sampling)
    if not (0 <= sampling <= 3) or not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise _lib.DgpError("jpeg_reconstruct: H, W must be in 1..65535 and sampling in 0..3, got %d, %d, %d" % (H, W, sampling))
    _need_cuda(coef, torch.int16, "coef")
    if qt.dtype not in (torch.int16, torch.uint16):
        raise _lib.DgpError("qt must have dtype int16 or uint16, got %s" % qt.dtype)
    _need_cuda(qt, qt.dtype, "qt")
    B = int(coef.shape[0])
    nblk, ncomp = jpeg_block_count(H, W, sampling)
    if coef.numel() != B * nblk * 64 or qt.numel() != B * ncomp * 64 or qt.device != coef.device:
        raise _lib.DgpError("jpeg_reconstruct: %d frames of %d x %d, sampling %s, need coef [%d, %d, 64] and qt [%d, %d, 64], got %s and %s"
                            % (B, H, W, JPEG_SAMPLING_NAMES[sampling], B, nblk, B, ncomp, tuple(coef.shape), tuple(qt.shape)))
    dev = coef.device
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    else:
        if not out.is_cuda or out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (B, H, W, 3):
            raise _lib.DgpError("jpeg_reconstruct: out must be uint8 %s on %s, got %s %s on %s" % ((B, H, W, 3), dev, out.dtype, tuple(out.shape), out.device))
        if B and (tuple(out.stride()[1:]) != (W * 3, 3, 1) or (B > 1 and out.stride(0) < H * W * 3)):
            raise _lib.DgpError("jpeg_reconstruct: every frame of out must be contiguous and the frames must not overlap (strides %s)" % (tuple(out.stride()),))
    if B == 0:
        return out
    need = int(lib.dgp_jpeg_scratch_bytes(B, H, W, sampling))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    stride = int(out.stride(0)) if B > 1 else H * W * 3
    _lib.check(lib.dgp_jpeg_reconstruct_u8(_ptr(coef), _ptr(qt), B, H, W, sampling, _ptr(out), stride, _ptr(scratch), need, _stream(dev)),
               "dgp_jpeg_reconstruct_u8")
    return out


def jpeg_decode(frames, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """A list of baseline JPEG byte strings of ONE geometry -> uint8 [n, H, W, 3] on the device: jpeg_probe + jpeg_entropy_decode per
    frame on the host (this thread), one upload, jpeg_reconstruct.  A frame whose size or sampling differs from the first frame's is a
    ValueError naming it; a stream the decoder does not take is a DgpError."""
    frames = list(frames)
    if not frames:
        raise ValueError("jpeg_decode: no frames")
    infos = [jpeg_probe(f) for f in frames]
    i0 = infos[0]
    for i, inf in enumerate(infos):
        if (inf.width, inf.height, inf.sampling) != (i0.width, i0.height, i0.sampling):
            raise ValueError("jpeg_decode: frame %d is %d x %d %s, frame 0 is %d x %d %s" % (
                i, inf.width, inf.height, JPEG_SAMPLING_NAMES[inf.sampling], i0.width, i0.height, JPEG_SAMPLING_NAMES[i0.sampling]))
    n = len(frames)
    coef = np.empty((n, i0.total_blocks, 64), np.int16)
    qt = np.empty((n, i0.ncomp, 64), np.uint16)
    for i, f in enumerate(frames):
        jpeg_entropy_decode(f, infos[i], coef[i], qt[i])
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return jpeg_reconstruct(torch.from_numpy(coef).to(dev), torch.from_numpy(qt.view(np.int16)).to(dev), i0.height, i0.width, i0.sampling, out=out)


# ---- the other way (dgp_jpeg_forward_u8 + dgp_jpeg_entropy_encode): frames, with markers drawn over them, to Pillow's JPEG bytes
from .jpeg import (quality_tables as jpeg_quality_tables, encode_bound as jpeg_encode_bound, entropy_encode as jpeg_entropy_encode,  # noqa: E402
                   sampling_id as jpeg_sampling_id)

_JPEG_QT_CACHE: Dict[Tuple[str, int], torch.Tensor] = {}


def _jpeg_device_tables(dev, quality: int) -> torch.Tensor:
    """the table pair of `quality` on the device, int16 [2, 64] holding jpeg_quality_tables' uint16 bits (uploaded once per device)"""
    key = (str(dev), int(quality))
    t = _JPEG_QT_CACHE.get(key)
    if t is None:
        t = _JPEG_QT_CACHE[key] = torch.from_numpy(jpeg_quality_tables(quality).view(np.int16)).to(dev)
    return t


def jpeg_forward(frames: torch.Tensor, quality: int = 90, subsampling="4:2:0", markers=None, dotsize: int = 3,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dgp_jpeg_forward_u8: B RGB frames of one size -> the quantised DCT coefficients libjpeg's baseline encoder makes of them, device
    int16 [B, total_blocks, 64] in the layout jpeg_entropy_decode writes (jpeg_entropy_encode makes Pillow's stream of a frame's).
    frames: device uint8 [B, H, W, 3], each frame contiguous, frames any whole number of bytes >= H W 3 apart (a slice of a larger
    buffer is read in place; it is never written).  quality 1..100 and subsampling "4:4:4" | "4:2:2" | "4:2:0" as Pillow's save takes
    them.  markers: None, or int32 [B, n, 6] = row, col, r, g, b, on (a device tensor, or a numpy array that is uploaded): squares of
    half-width dotsize drawn over the pixels as they are read, the highest index on top, clipped to the frame (models/render.py's
    marker_table makes one, draw_markers_host is the numpy statement).  Two launches on the current stream."""
    lib = _lib.load()
    sampling = jpeg_sampling_id(subsampling)
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise _lib.DgpError("jpeg_forward: frames must be a device uint8 [B, H, W, 3] tensor, got %s %s" % (frames.dtype, tuple(frames.shape)))
    B, H, W = (int(v) for v in frames.shape[:3])
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise _lib.DgpError("jpeg_forward: H, W must be in 1..65535, got %d, %d" % (H, W))
    if B and (tuple(frames.stride()[1:]) != (W * 3, 3, 1) or (B > 1 and frames.stride(0) < H * W * 3)):
        raise _lib.DgpError("jpeg_forward: every frame must be contiguous and the frames must not overlap (strides %s)" % (tuple(frames.stride()),))
    dev = frames.device
    qt = _jpeg_device_tables(dev, quality)
    if isinstance(dotsize, bool) or not isinstance(dotsize, (int, np.integer)) or not 0 <= int(dotsize) <= 65535:
        raise _lib.DgpError("jpeg_forward: dotsize must be an integer in 0..65535, got %r" % (dotsize,))
    nblk, _ = jpeg_block_count(H, W, sampling)
    n_markers = 0
    if markers is not None:
        if isinstance(markers, np.ndarray):
            if markers.dtype != np.int32:
                raise _lib.DgpError("jpeg_forward: markers must be int32, got %s" % markers.dtype)
            markers = torch.from_numpy(np.ascontiguousarray(markers)).to(dev)
        _need_cuda(markers, torch.int32, "markers")
        if markers.dim() != 3 or markers.shape[0] != B or markers.shape[2] != 6 or markers.device != dev:
            raise _lib.DgpError("jpeg_forward: markers must be int32 [%d, n, 6] on %s, got %s on %s" % (B, dev, tuple(markers.shape), markers.device))
        n_markers = int(markers.shape[1])
        if n_markers == 0:
            markers = None
    if out is None:
        out = torch.empty((B, nblk, 64), dtype=torch.int16, device=dev)
    else:
        _need_cuda(out, torch.int16, "out")
        if out.numel() != B * nblk * 64 or out.device != dev:
            raise _lib.DgpError("jpeg_forward: out must be int16 [%d, %d, 64] on %s, got %s on %s" % (B, nblk, dev, tuple(out.shape), out.device))
    if B == 0:
        return out
    need = int(lib.dgp_jpeg_forward_scratch_bytes(B, H, W, sampling))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    stride = int(frames.stride(0)) if B > 1 else H * W * 3
    _lib.check(lib.dgp_jpeg_forward_u8(_ptr(frames), B, H, W, stride, sampling, _ptr(qt), _ptr(markers), n_markers, int(dotsize), _ptr(out),
                                       _ptr(scratch), need, _stream(dev)), "dgp_jpeg_forward_u8")
    return out


def jpeg_encode(frames: torch.Tensor, quality: int = 90, subsampling="4:2:0", markers=None, dotsize: int = 3) -> list:
    """jpeg_forward, one download, jpeg_entropy_encode per frame on this thread -> a list of byte strings: what Pillow's
    save(quality=, subsampling=) writes for each frame with its markers drawn.  For tests and small jobs: models/render.py's
    write_annotated_movie runs the same three steps as a pipeline."""
    coef = jpeg_forward(frames, quality, subsampling, markers, dotsize).cpu().numpy()
    B, H, W = (int(v) for v in frames.shape[:3])
    sampling = jpeg_sampling_id(subsampling)
    qt = jpeg_quality_tables(quality)
    buf = np.empty(jpeg_encode_bound(H, W, sampling), np.uint8)
    out = []
    for i in range(B):
        n = jpeg_entropy_encode(coef[i], H, W, sampling, qt, buf)
        out.append(buf[:n].tobytes())
    return out
