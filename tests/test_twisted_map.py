"""CPU: the piece map of the specialised kernel's copy-out in its latency shapes (csrc/qp_twisted_map.h), which the kernel and this test
read from the same header.  tests/cpp/test_twisted_map.cpp includes it without the HIP runtime and checks, for every instantiated
(r, M): the kept pieces of all steps cover every (trajectory, axis) row exactly once, none lies outside the tile, the dropped ones are
exactly those of lanes without a segment in that step (and the padding column of a 48-byte chunk); with 16 lanes per trajectory, r = 4
and even M >= 4 every store instruction writes whole 128-byte lines from eight adjacent lanes wherever both lane pairs of a side have a
segment (the last step of M = 6 and 10 writes the middle line only: whole within the one instruction, from two groups of four lanes), and for
r = 3 adjacent chunks form one 96-byte run.
The second test builds the same stand-alone program with the address and undefined-behaviour sanitizers and runs it."""
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
                           os.path.join(ROOT, "tests", "cpp", "test_twisted_map.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "twisted_map OK" in cp.stdout, cp.stdout


def test_twisted_map(tmp_path):
    _build_and_run(tmp_path, "test_twisted_map", [])


def test_twisted_map_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "test_twisted_map_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
