"""In-tree build of libdgp_hip.so (hipcc, gfx950 only).  `python -m deepgraphpose_amd.build`.

Every source is compiled to its own object (in parallel) and the objects are linked into the shared library.  Whether a
step can be skipped is decided by CONTENT: the sha256 of the source, of every header and of the command line is stored
next to each object (`build/*.o.sha`) and next to the library (`libdgp_hip.so.sha`); file times play no role, so a
snapshot copied to another machine rebuilds exactly what changed there and nothing else.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJDIR = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libdgp_hip.so")
# the same sources with -DDGP_TUNING (the A/B switches read from the environment, the opt-in paths that measured slower): loaded only
# through DGP_HIP_LIB, by the tests of those paths
TUNING_LIB = os.path.join(HERE, "libdgp_hip_tuning.so")
SOURCES = ["dgp_conv_split.hip", "dgp_conv_f32.hip", "dgp_kernels.hip", "dgp_ops.hip", "dgp_chain.hip", "dgp_loss.hip", "dgp_net.hip", "dgp_train.hip", "dgp_wgrad.hip", "dgp_train_pack.hip",
           "dgp_optim.hip", "dgp_train_layers.hip", "dgp_flow.hip", "dgp_resize.hip", "dgp_targets.hip", "dgp_frames.hip", "dgp_augment.hip", "dgp_jpeg.hip", "dgp_select.hip"]
HEADERS = ["dgp_internal.h", "dgp_device.h", "dgp_conv.h", "dgp_engine.h", "dgp_train.h", "dgp_jpeg_host.h", os.path.join("..", "..", "include", "dgp_hip.h")]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm with gfx950 support)")


def _sha(paths, extra: str = "") -> str:
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as f:
            h.update(hashlib.sha256(f.read()).digest())
    return h.hexdigest()


def _read(path: str) -> str:
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return ""


def _extra_flags() -> list:
    return os.environ.get("DGP_BUILD_FLAGS", "").split()


def _variant(tuning: bool):
    """(object directory, library, compile flags) of the product build or of the -DDGP_TUNING one"""
    if tuning:
        return os.path.join(OBJDIR, "tuning"), TUNING_LIB, FLAGS + _extra_flags() + ["-DDGP_TUNING"]
    return OBJDIR, LIB, FLAGS + _extra_flags()


def source_hash(tuning: bool = False) -> str:
    """sha256 over every source, every header and the compile flags: what libdgp_hip.so.sha must hold for the library to be current"""
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return _sha(deps, " ".join(_variant(tuning)[2]))


def needs_build(tuning: bool = False) -> bool:
    lib = _variant(tuning)[1]
    return not os.path.exists(lib) or _read(lib + ".sha") != source_hash(tuning)


def build(force: bool = False, verbose: bool = True, tuning: bool = False) -> str:
    objdir, lib, flags = _variant(tuning)
    if not force and not needs_build(tuning):
        return lib
    hipcc = _hipcc()
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]

    def compile_one(src: str) -> str:
        path = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src + ".o")
        want = _sha([path] + hdrs, " ".join(flags))
        if not force and os.path.exists(obj) and _read(obj + ".sha") == want:
            return obj
        cmd = [hipcc] + flags + ["-c", path, "-o", obj]
        if verbose:
            print("[dgp build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(obj + ".sha", "w") as f:
            f.write(want)
        return obj

    jobs = max(1, min(len(SOURCES), os.cpu_count() or 1))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", lib] + objs
    if verbose:
        print("[dgp build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(lib + ".sha", "w") as f:
        f.write(source_hash(tuning))
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, tuning="--tuning" in sys.argv))
