"""CPU: the piece map of solve_twisted_group8_kernel's copy-out (csrc/qp_twisted_map8.h), which the kernel and this test read from the same
header, and the host rule that decides which kernel a group's node gets (csrc/uavqp_capture.h: group_kernel_choice).
tests/cpp/test_twisted_group8_map.cpp includes both without the HIP runtime and checks, for all 20 (r, M): the kept pieces of all steps
cover every coefficient of the wave's eight trajectories exactly once and none lies outside the tile; the dropped ones are exactly those
whose producer has no such segment (and the padding column of a 48-byte chunk); every piece is read from the staging row its producer
wrote; each of the six stores of a step is the 16-lane map's store of one axis of four trajectories -- whole 128-byte lines from eight
adjacent lanes for r = 4 and even M >= 4, 96-byte runs for r = 3.  The rule: a group of one is the launch as captured, a batch that is no
whole number of eights and every launch at tile 8 keep the group kernel of their own tile (or none: (4, 8) at tile 8 still has no group).
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
                           os.path.join(ROOT, "tests", "cpp", "test_twisted_group8_map.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "twisted_group8_map OK" in cp.stdout, cp.stdout
    return exe


def test_twisted_group8_map(tmp_path):
    exe = _build_and_run(tmp_path, "test_twisted_group8_map", [])
    # the question the GPU test asks: members r M tile n_traj num_cus -> 0 as captured, 1 own tile's group kernel, 2 eight per wave
    ask = lambda *a: int(subprocess.check_output([exe, "choose"] + [str(v) for v in a], text=True))
    assert ask(2, 4, 8, 4, 4096, 256) == 2 and ask(1, 4, 8, 4, 4096, 256) == 0 and ask(2, 4, 8, 4, 12, 256) == 1
    assert ask(8, 4, 8, 8, 4096, 256) == 0 and ask(2, 4, 2, 8, 8, 256) == 1 and ask(2, 4, 7, 4, 8, 256) == 0


def test_twisted_group8_map_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "test_twisted_group8_map_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
