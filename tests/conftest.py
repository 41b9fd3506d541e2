import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def lib_built():
    """Make sure libdgp_hip.so exists (hipcc cross-compiles without a GPU)."""
    from deepgraphpose_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="session")
def tuning_lib(lib_built):
    """The -DDGP_TUNING build of the same sources (deepgraphpose_amd/libdgp_hip_tuning.so), for child processes (DGP_HIP_LIB): the A/B
    switches read from the environment and the opt-in paths that measured slower.  A child process checks that it reports itself as one."""
    from deepgraphpose_amd import build
    path = build.build(verbose=False, tuning=True)
    r = subprocess.run([sys.executable, "-c", "import sys; from deepgraphpose_amd import _lib; sys.exit(0 if _lib.load().dgp_tuning_build() else 3)"],
                       env=dict(os.environ, DGP_HIP_LIB=path, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, ("not a tuning build", path, r.stderr[-1000:])
    return path


@pytest.fixture
def tuning_build(request, lib_built):
    """Tests of the opt-in paths that measured slower (256-row tile, the trainer's fast pass): they exist only in a library built with
    -DDGP_TUNING.  True: this process runs such a library, the test body runs here.  On the product library the test runs again in a
    child pytest process on the tuning library (tuning_lib), must pass there, and the fixture returns False: the body returns at once."""
    from deepgraphpose_amd import _lib, build
    if _lib.load().dgp_tuning_build():
        return True
    assert os.environ.get("DGP_HIP_LIB") != build.TUNING_LIB, "%s is not a -DDGP_TUNING build" % build.TUNING_LIB
    lib = request.getfixturevalue("tuning_lib")
    node = "%s::%s" % (request.node.path, request.node.name)
    env = dict(os.environ, DGP_HIP_LIB=lib, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pytest", node, "-q", "-rA", "-p", "no:cacheprovider"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    return False
