"""libkgpu's routing plan (kubernetes-1_amd/csrc/kgpu_route.h: pod kinds, the call-level gates and the
run segmentation run_batch_once issues from) under AddressSanitizer + UndefinedBehaviorSanitizer on the
CPU.  tests/csrc/route_check.cpp walks every kind sequence up to six pods against every gate set: the
walk partitions the batch, each run holds only what its route may carry, the caps split runs, and the
documented routings of test_norm_persistent come out as written."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "route_check.cpp")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "kubernetes-1_amd", "csrc"), SRC, "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_route_plan_under_asan_ubsan(checker):
    env = dict(os.environ)
    # the environment may preload a library ahead of the ASan runtime: ASan tolerates that with
    # verify_asan_link_order=0 (the environment itself is left as it is)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:verify_asan_link_order=0"
    out = subprocess.run([checker], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    assert "route ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
