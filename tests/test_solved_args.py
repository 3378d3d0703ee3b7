"""CPU: what the entries that evaluate a batch of solved trajectories share (csrc/uavqp_solved.h) -- the refusal precedence of
solved_args_check under the per-trajectory and the swarm rule, and the staging slots of SolvedStage.  tests/cpp/test_solved_args.cpp
includes the header without the HIP runtime and checks them against hand-written tables."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solved_args_precedence_and_stage_slots(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / "test_solved_args")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uav_motion_planning_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_solved_args.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cp.returncode == 0 and "solved_args OK" in cp.stdout, cp.stdout
