"""CPU: how many solves a launch of a replay may carry when UAVQP_CAPTURE_FUSE names no count (csrc/uavqp_capture.h: fuse_cap,
member_waves, fuse_waves_from_env, fuse_named_from_env, and fuse_groups with one cap per node) -- a budget of waves per launch divided by
the waves one member adds in the kernel its group runs, between 2 and 8.  tests/cpp/test_capture_fuse_waves.cpp includes the header
without the HIP runtime and checks the edges of that arithmetic, the two parsers, the waves of a member against group_kernel_choice, the
per-node grouping against the int-F form and against the brute-force statement of the rule on 500 random captures, and the benchmark's
rotation (13 + 13 launches at a budget of 4096 waves and 512 waves per member).  The same program runs a second time under the address
and undefined-behaviour sanitizers: host code with its own main.  tests/cpp/capture_fuse_waves_plan.cpp, the program the GPU test asks
for plans, is run here on three small captures."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")


def _build(tmp_path, name, source, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", source), "-o", exe])
    return exe


def _build_and_run(tmp_path, name, flags):
    exe = _build(tmp_path, name, "test_capture_fuse_waves.cpp", flags)
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(cp.stdout)
    assert cp.returncode == 0 and "capture_fuse_waves OK" in cp.stdout, cp.stdout
    return cp.stdout


def test_capture_fuse_waves(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_fuse_waves", ["-O1"])
    assert "random captures:" in out


def test_capture_fuse_waves_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_fuse_waves_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out


def test_plan_program_on_small_rotations(tmp_path):
    """Nine min-snap solves of 8 segments over five buffer sets on one lane, as the GPU test captures them: n = 8 is one wave per member
    in the eight-per-wave kernel, n = 16 two, n = 12 (no whole number of eights) three waves of the 16-lane group kernel."""
    exe = _build(tmp_path, "capture_fuse_waves_plan", "capture_fuse_waves_plan.cpp", ["-O1"])

    def plan(n, budget, r=4, M=8, solves=9, sets=5):
        stride = 1 << 20
        lines = [f"1 1 {budget} 256 {solves}"]
        for i in range(solves):
            base = (1 << 30) + (i % sets) * 5 * stride
            lines.append(f"{r} {M} 4 {n} {base} {base + stride} {base + 2 * stride} {base + 3 * stride} {base + 4 * stride}")
        out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        rows = [[int(v) for v in line.split()] for line in out.splitlines()]
        assert sorted(k for row in rows for k in row[3:]) == list(range(solves))
        return [row[2] for row in rows], [len(row) - 3 for row in rows]

    assert plan(8, "4") == ([4, 4, 4], [4, 4, 1])
    assert plan(8, "8") == ([8, 8], [5, 4])                      # the lane meets set 0 again after five solves
    assert plan(8, "-") == ([8, 8], [5, 4])
    assert plan(8, "junk") == plan(8, "-")
    assert plan(16, "4") == ([2] * 5, [2, 2, 2, 2, 1])
    assert plan(16, "8") == ([4, 4, 4], [4, 4, 1])
    assert plan(12, "4") == ([2] * 5, [2, 2, 2, 2, 1])           # the lower bound
    assert plan(12, "8") == ([2] * 5, [2, 2, 2, 2, 1])
    assert plan(12, "12") == ([4, 4, 4], [4, 4, 1])
    assert plan(8, "8", solves=17, sets=9)[1] == [8, 8, 1]
    assert plan(8, "8", r=4, M=7)[1] == [1] * 9                  # (4, 7) has no group kernel: every solve its own launch
