"""CPU: what the sampling kernels share (csrc/qp_poly.h) -- the segment rule of PolyTraj::evaluatePos in its two forms (bit-identical on
100 000 seeded inputs, the knot and end-point cases), Horner on a derivative and the body frame against the code the kernels carried
before.  tests/cpp/test_poly_rule.cpp includes the header without the HIP runtime and checks them; the second test builds the same
stand-alone program with the address and undefined-behaviour sanitizers and runs it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "uav_motion_planning_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_poly_rule.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "poly_rule OK" in cp.stdout, cp.stdout


def test_poly_rule_horner_frame(tmp_path):
    _build_and_run(tmp_path, "test_poly_rule", [])


def test_poly_rule_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "test_poly_rule_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
