"""CPU: which captured solves may overlap when their graph is replayed (csrc/uavqp_capture.h) -- conflict edges, dead status stores,
lane edges, barriers, the lane count.  tests/cpp/test_capture_deps.cpp includes the header without the HIP runtime and checks them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capture_dependency_rules(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / "test_capture_deps")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uav_motion_planning_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_capture_deps.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "capture_deps OK" in cp.stdout, cp.stdout
