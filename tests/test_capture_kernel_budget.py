"""CPU: the eight-per-wave kernel's own default budget of waves (csrc/uavqp_capture.h: FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT,
fuse_waves_named_from_env, fuse_budget, group_cap -- the function rebuild_captured asks for the cap of every captured launch).
tests/cpp/test_capture_kernel_budget.cpp includes the header without the HIP runtime and checks the parser at its edges, the cap of a
group with nothing named / a budget named / a count named for tile 4 with and without the kernel, a batch that is no whole number of
eights and tile 8, the benchmark's rotation (200 solves over 35 sets on 2 lanes: 26 + 25 launches under the defaults, 13 + 13 at a named budget of 4096) and `--batch 4092`
(its 101 launches), and on 500 random captures that a named budget or count gives exactly the plan of the rule before.  The same
program runs a second time under the address and undefined-behaviour sanitizers: host code with its own main.
tests/cpp/capture_kernel_budget_plan.cpp, the program the GPU test asks for plans, is run here on small captures."""
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
    exe = _build(tmp_path, name, "test_capture_kernel_budget.cpp", flags)
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(cp.stdout)
    assert cp.returncode == 0 and "capture_kernel_budget OK" in cp.stdout, cp.stdout
    return cp.stdout


def test_capture_kernel_budget(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_kernel_budget", ["-O1"])
    assert "random captures:" in out


def test_capture_kernel_budget_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_kernel_budget_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out


def test_plan_program_on_small_captures(tmp_path):
    """Min-snap solves of 8 segments over buffer sets of their own, one lane: the caps the plan program prints under the three settings."""
    exe = _build(tmp_path, "capture_kernel_budget_plan", "capture_kernel_budget_plan.cpp", ["-O1"])
    old = _build(tmp_path, "capture_fuse_waves_plan", "capture_fuse_waves_plan.cpp", ["-O1"])

    def lines(n, solves, sets, r=4, M=8):
        stride = 1 << 26
        out = []
        for i in range(solves):
            base = (1 << 32) + (i % sets) * 5 * stride
            out.append(f"{r} {M} 4 {n} {base} {base + stride} {base + 2 * stride} {base + 3 * stride} {base + 4 * stride}")
        return out

    def run(program, head, body):
        out = subprocess.run([program], input="\n".join([head] + body) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        rows = [[int(v) for v in line.split()] for line in out.splitlines()]
        assert sorted(k for row in rows for k in row[3:]) == list(range(len(body)))
        return [row[2] for row in rows], [len(row) - 3 for row in rows]

    def plan(n, fuse, budget, solves=17, sets=9, **kw):
        return run(exe, f"1 1 {fuse} {budget} 256 {solves}", lines(n, solves, sets, **kw))

    assert plan(4096, "-", "-") == ([4] * 5, [4, 4, 4, 4, 1])           # the eight-per-wave kernel's own default: 2048 waves / 512 per member
    assert plan(4096, "-", "4096") == ([8, 8, 8], [8, 8, 1])
    assert plan(4096, "-", "2048") == ([4] * 5, [4, 4, 4, 4, 1])        # a named budget, as before
    assert plan(4096, "-", "3072") == ([6, 6, 6], [6, 6, 5])
    assert plan(4096, "2", "-") == ([2] * 9, [2] * 8 + [1])             # a named count overrides both
    assert plan(4096, "2", "4096") == plan(4096, "2", "-")
    assert plan(4092, "-", "-") == ([2] * 9, [2] * 8 + [1])             # no whole number of eights: the 16-lane group kernel at 2048
    assert plan(4096, "-", "-", M=7)[1] == [1] * 17                     # (4, 7) has no group kernel: every solve its own launch
    assert plan(4096, "junk", "junk") == plan(4096, "-", "-")
    # small members: the plans of the one-budget program (tests/test_gpu_capture_fuse_waves.py) are the library's, named or not
    for n in (8, 16, 24, 2048, 12):
        for budget in ("-", "4", "8", "2048"):
            body = lines(n, 17, 9)
            assert run(exe, f"1 1 - {budget} 256 17", body) == run(old, f"1 1 {budget} 256 17", body), (n, budget)
