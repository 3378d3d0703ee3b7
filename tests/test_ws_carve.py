"""CPU: the slot carver every device workspace and the host staging are laid out with (csrc/uavqp_ws.h) -- alignment, order, no
overlap, absent slots, the capacity.  tests/cpp/test_ws_carve.cpp includes the header without the HIP runtime and checks them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_carve_layout_rules(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / "test_ws_carve")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uav_motion_planning_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ws_carve.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "ws_carve OK" in cp.stdout, cp.stdout
