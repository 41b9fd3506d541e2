"""The host half of the JPEG path (csrc/dgp_jpeg_host.h through the C-ABI): parse a baseline JPEG frame and Huffman-decode it into
quantised coefficients, and the other way (quality_tables, encode_bound, entropy_encode: coefficients to the complete stream, for
models/render.py's movie writer and its encode threads).  No torch and no GPU in here -- models/staging.py calls it from its decode threads (ctypes releases the GIL for
the duration of a call, and the C functions keep no state), engine.py re-exports it beside the device half (engine.jpeg_reconstruct)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

SAMPLING_NAMES = ("gray", "4:4:4", "4:2:2", "4:2:0")        # DGP_JPEG_GRAY, _444, _422, _420 (include/dgp_hip.h)


def _buffer(data):
    """(what ctypes passes as the pointer, byte count) of bytes / bytearray / memoryview / uint8 array, without a copy where possible"""
    if isinstance(data, bytes):
        return data, len(data)
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    return a.ctypes.data_as(C.c_void_p), int(a.size)


def probe(data) -> _lib.DgpJpegInfo:
    """dgp_jpeg_probe: the geometry of one baseline JPEG stream (width, height, ncomp, sampling, the block counts, restart_interval,
    scan_offset); DgpError naming the reason for anything the decoder does not take (include/dgp_hip.h lists what it takes)."""
    lib = _lib.load()
    info = _lib.DgpJpegInfo()
    p, n = _buffer(data)
    _lib.check(lib.dgp_jpeg_probe(p, n, C.byref(info)), "dgp_jpeg_probe")
    return info


def entropy_decode(data, info: _lib.DgpJpegInfo, coef_out: np.ndarray, qt_out: np.ndarray) -> None:
    """dgp_jpeg_entropy_decode into caller memory (pinned views in the pipeline): coef_out int16 with at least total_blocks * 64
    elements, qt_out uint16 with at least ncomp * 64, both C-contiguous and writable.  Thread-safe; the GIL is released meanwhile."""
    lib = _lib.load()
    if coef_out.dtype != np.int16 or not coef_out.flags.c_contiguous or not coef_out.flags.writeable or coef_out.size < info.total_blocks * 64:
        raise _lib.DgpError("jpeg_entropy_decode: coef_out must be writable contiguous int16 with at least %d elements" % (info.total_blocks * 64))
    if qt_out.dtype != np.uint16 or not qt_out.flags.c_contiguous or not qt_out.flags.writeable or qt_out.size < info.ncomp * 64:
        raise _lib.DgpError("jpeg_entropy_decode: qt_out must be writable contiguous uint16 with at least %d elements" % (info.ncomp * 64))
    p, n = _buffer(data)
    _lib.check(lib.dgp_jpeg_entropy_decode(p, n, C.byref(info), coef_out.ctypes.data_as(C.c_void_p), qt_out.ctypes.data_as(C.c_void_p)),
               "dgp_jpeg_entropy_decode")


def sampling_id(subsampling) -> int:
    """DGP_JPEG_444 / _422 / _420 from what Pillow's save(subsampling=) takes ("4:4:4" | "4:2:2" | "4:2:0", or 0 | 1 | 2) -- NOT from a
    DGP_JPEG_* value; anything else (grey included) is a ValueError"""
    if isinstance(subsampling, str) and subsampling in SAMPLING_NAMES[1:]:
        return SAMPLING_NAMES.index(subsampling)
    if isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) and 0 <= int(subsampling) <= 2:
        return int(subsampling) + 1
    raise ValueError("subsampling must be '4:4:4', '4:2:2' or '4:2:0' (or Pillow's 0, 1, 2), got %r: grey and other samplings are not written"
                     % (subsampling,))


def quality_tables(quality: int) -> np.ndarray:
    """dgp_jpeg_quality_tables: libjpeg's table pair for quality 1..100, uint16 [2, 64] (luminance, chrominance) in natural order"""
    lib = _lib.load()
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)):
        raise _lib.DgpError("jpeg quality must be an integer in 1..100, got %r" % (quality,))
    qt = np.zeros((2, 64), np.uint16)
    _lib.check(lib.dgp_jpeg_quality_tables(int(quality), qt.ctypes.data_as(C.c_void_p)), "dgp_jpeg_quality_tables")
    return qt


def encode_bound(H: int, W: int, sampling: int) -> int:
    """dgp_jpeg_encode_bound: a buffer size that holds the stream of any H x W frame"""
    n = int(_lib.load().dgp_jpeg_encode_bound(int(H), int(W), int(sampling)))
    if n <= 0:
        raise _lib.DgpError("jpeg_encode_bound: H, W must be in 1..65535 and sampling DGP_JPEG_444, _422 or _420, got %d, %d, %d" % (H, W, sampling))
    return n


def entropy_encode(coef: np.ndarray, H: int, W: int, sampling: int, qt: np.ndarray, out: np.ndarray, cap=None) -> int:
    """dgp_jpeg_entropy_encode from caller memory into caller memory: coef C-contiguous int16 with the frame's total_blocks * 64
    elements (a pinned view in the pipeline), qt contiguous uint16 [2, 64], out a writable contiguous uint8 array of which at most `cap`
    (default: all) bytes are written -> the stream's length.  Thread-safe; the GIL is released meanwhile."""
    lib = _lib.load()
    if sampling not in (1, 2, 3):
        raise _lib.DgpError("jpeg_entropy_encode: sampling must be DGP_JPEG_444, _422 or _420 (grey is not written), got %r" % (sampling,))
    if not (0 < H <= 65535 and 0 < W <= 65535):
        raise _lib.DgpError("jpeg_entropy_encode: H, W must be in 1..65535, got %d, %d" % (H, W))
    hs, vs = (2 if sampling >= 2 else 1), (2 if sampling == 3 else 1)
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    need = mcus * (hs * vs + 2) * 64
    if coef.dtype != np.int16 or not coef.flags.c_contiguous or coef.size != need:
        raise _lib.DgpError("jpeg_entropy_encode: coef must be contiguous int16 with %d elements, got %s %s" % (need, coef.dtype, coef.shape))
    if qt.dtype != np.uint16 or not qt.flags.c_contiguous or qt.size != 128:
        raise _lib.DgpError("jpeg_entropy_encode: qt must be contiguous uint16 [2, 64]")
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise _lib.DgpError("jpeg_entropy_encode: out must be a writable contiguous uint8 array")
    cap = out.size if cap is None else int(cap)
    if not 0 <= cap <= out.size:
        raise _lib.DgpError("jpeg_entropy_encode: cap %d is outside the %d bytes of out" % (cap, out.size))
    n = C.c_int64(0)
    _lib.check(lib.dgp_jpeg_entropy_encode(coef.ctypes.data_as(C.c_void_p), int(H), int(W), int(sampling), qt.ctypes.data_as(C.c_void_p),
                                           out.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "dgp_jpeg_entropy_encode")
    return int(n.value)


def same_geometry(a: _lib.DgpJpegInfo, b: _lib.DgpJpegInfo) -> bool:
    return (a.width, a.height, a.sampling) == (b.width, b.height, b.sampling)
