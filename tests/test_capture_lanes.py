"""CPU: the lane layout a capture is replayed with (csrc/uavqp_capture.h: lay_out) -- a solve follows the solve it conflicts with into
that solve's lane, the lanes meet only in front of a solve with predecessors in two of them, a barrier is a stage of its own.
tests/cpp/test_capture_lanes.cpp includes the header without the HIP runtime, pins a handful of captures and checks 500 random ones against
the brute-force rule (every conflicting pair: different stages, or one lane).  The same program runs a second time under the address and
undefined-behaviour sanitizers: host code with its own main."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "uav_motion_planning_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_capture_lanes.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(cp.stdout)
    assert cp.returncode == 0 and "capture_lanes OK" in cp.stdout, cp.stdout
    return cp.stdout


def test_capture_lane_layout(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_lanes", ["-O1"])
    assert "random captures:" in out


def test_capture_lane_layout_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_lanes_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out
