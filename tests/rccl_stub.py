"""The stub collective of tests/stub/fake_rccl.cpp, built once per test session, and the way every test starts a child process
that uses it.  pt_comm.cpp resolves PT_RCCL_PATH once per process, so whatever runs with the stub (or, on a multi-GPU box, with
the real library) runs in a child."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

ROCM = "/opt/rocm"


@functools.lru_cache(maxsize=None)
def stub_path():
    """Path of libfake_rccl.so (compiled on first use); skips the calling test when g++ or the RCCL header is missing."""
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(ROCM, "include", "rccl", "rccl.h")):
        pytest.skip("g++ or the RCCL header is missing")
    d = tempfile.mkdtemp(prefix="fake_rccl_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    stub = os.path.join(d, "libfake_rccl.so")
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-o", stub,
                           os.path.join(ROOT, "tests", "stub", "fake_rccl.cpp"), "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROCM, "lib")])
    return stub


def stub_env(**extra):
    """os.environ + PT_RCCL_PATH = the stub (+ extra)."""
    return dict(os.environ, PT_RCCL_PATH=stub_path(), **extra)


def run_child(argv, env, timeout, cwd=None):
    """One child process under a time limit; a child that outlives it is killed and the test fails there (nothing else is started
    on the GPU by that test, nothing is tried again).  Returns the CompletedProcess-like (returncode, stdout, stderr)."""
    p = subprocess.Popen(argv, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, 9)  # the whole session: launchers such as torch.distributed.run have children of their own
        except OSError:
            pass
        p.kill()
        out, err = p.communicate()
        pytest.fail("child exceeded its time limit of %d s and was killed: %s\n%s" % (timeout, " ".join(argv[:6]), (err or "")[-3000:]))
    return p.returncode, out, err
