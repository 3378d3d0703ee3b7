"""CPU: which captured solves are replayed as ONE launch (csrc/uavqp_capture.h: fuse_groups) -- in capture order a solve joins the open
group of its lane only if it has the group's shape, takes the one-tile-per-wave instantiation, conflicts with no member and the group has
room; a barrier is alone.  tests/cpp/test_capture_fuse.cpp includes the header without the HIP runtime, pins the groupings of the
benchmark's rotation and of a handful of small captures and checks 500 random ones against the brute-force statement of the rule.  The same
program runs a second time under the address and undefined-behaviour sanitizers: host code with its own main.

The group kernel itself (csrc/qp_twisted.h: solve_twisted_group_kernel) is cross-compiled to gfx950 with the flags its units get and its
resource usage is read: no scratch and at most 168 VGPRs in every instantiation, i.e. three waves fit a SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")


def _build_and_run(tmp_path, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_capture_fuse.cpp"), "-o", exe])
    cp = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(cp.stdout)
    assert cp.returncode == 0 and "capture_fuse OK" in cp.stdout, cp.stdout
    return cp.stdout


def test_capture_fuse_groups(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_fuse", ["-O1"])
    assert "random captures:" in out


def test_capture_fuse_groups_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "test_capture_fuse_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out


def _make(*args):
    return subprocess.check_output(["make", "-s", "-C", CSRC, *args], text=True).strip()


def test_group_kernels_fit_three_waves_per_simd(tmp_path):
    hipcc = _make("print-hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} is missing: the library cannot be built here either")
    units = ("k_twisted3_group", "k_twisted4_group")
    procs = []
    for unit in units:   # the two units side by side: each is some twenty instantiations
        flags = _make("unit-flags", f"UNIT={unit}").split()
        procs.append(subprocess.Popen([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / f"{unit}.o"),
                                       os.path.join(CSRC, f"{unit}.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True))
    n_kernels = 0
    for unit, p in zip(units, procs):
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
        name = None
        seen = {}
        for line in err.splitlines():
            m = re.search(r"remark: .*Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                seen[name] = {}
            for key, pat in (("vgprs", r"remark: .*\bVGPRs: (\d+)"), ("scratch", r"remark: .*ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occupancy", r"remark: .*Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and name is not None:
                    seen[name][key] = int(m.group(1))
        groups = {k: v for k, v in seen.items() if "solve_twisted_group_kernel" in k}
        assert groups and len(groups) == len(seen), sorted(seen)
        for k, v in sorted(groups.items()):
            print(f"{unit} {k}: {v}")
            assert v["scratch"] == 0 and v["vgprs"] <= 168 and v["occupancy"] >= 3, (k, v)
        n_kernels += len(groups)
    assert n_kernels == 28   # kernel_instances.h: 6 + 4 min-snap and 10 + 8 min-jerk shapes
