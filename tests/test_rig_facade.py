"""The reference's RigBundleAdjuster tests (src/optim/bundle_adjustment_test.cc:
755-969) and CameraRig checks rerun in C++ through the colmap_amd facade
(include/colmap_amd/camera_rig.h, tests/cpp/rig_bundle_adjustment_test.cc):
CameraRig's CHECKs, ComputeAbsolutePose (a shared rig pose returned exactly,
a hand-computed AverageQuaternions case) and the structural counts on the
host; full Solve with the CheckVariableCameraRig / CheckConstantCameraRig
expectations on the MI355X."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd")


def build():
    """The flags of tests/cpp/Makefile's bundle_adjustment_test (host compiler only)."""
    exe, src = os.path.join(CPP, "rig_bundle_adjustment_test"), os.path.join(CPP, "rig_bundle_adjustment_test.cc")
    deps = [src, os.path.join(ROOT, "include", "mi_ba.h"), os.path.join(LIBDIR, "libmi_ba.so")] + [
        os.path.join(ROOT, "include", "colmap_amd", h) for h in ("camera_rig.h", "bundle_adjustment.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, src, "-L" + LIBDIR, "-lmi_ba", "-Wl,-rpath," + LIBDIR], check=True)
    return exe


def run(mode):
    out = subprocess.run([build(), mode], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failure(s)" in out.stdout
    return out.stdout


def test_rig_facade_host():
    assert run("host").count("PASS") == 5


@pytest.mark.gpu
def test_rig_facade_solve_gpu(gpu):
    assert run("gpu").count("PASS") == 4
