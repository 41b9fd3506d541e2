"""The host half of the JPEG path (csrc/dgp_jpeg_host.h through the C-ABI): parse a baseline JPEG frame and Huffman-decode it into
quantised coefficients.  No torch and no GPU in here -- models/staging.py calls it from its decode threads (ctypes releases the GIL for
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


def same_geometry(a: _lib.DgpJpegInfo, b: _lib.DgpJpegInfo) -> bool:
    return (a.width, a.height, a.sampling) == (b.width, b.height, b.sampling)
