"""CPU: the resource usage of solve_twisted_group8_kernel (csrc/qp_twisted.h), read from a cross-compile of its two units to gfx950 with the
flags the library's build gives them, as tests/test_capture_fuse.py reads the group kernel's: no scratch and at least two waves per
SIMD (at most 256 VGPRs) in every instantiation, 16 of them -- every shape of the tile-4 group lists (csrc/kernel_instances.h) -- and
nothing else in the units."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")


def _make(*args):
    return subprocess.check_output(["make", "-s", "-C", CSRC, *args], text=True).strip()


def test_group8_kernels_fit_two_waves_per_simd(tmp_path):
    hipcc = _make("print-hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} is missing: the library cannot be built here either")
    units = ("k_twisted3_group8", "k_twisted4_group8")
    procs = []
    for unit in units:
        flags = _make("unit-flags", f"UNIT={unit}").split()
        procs.append(subprocess.Popen([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / f"{unit}.o"),
                                       os.path.join(CSRC, f"{unit}.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True))
    counts = {}
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
                             ("occupancy", r"remark: .*Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"remark: .*LDS Size \[bytes/block\]: (\d+)")):
                m = re.search(pat, line)
                if m and name is not None:
                    seen[name][key] = int(m.group(1))
        mine = {k: v for k, v in seen.items() if "solve_twisted_group8_kernel" in k}
        assert mine and len(mine) == len(seen), sorted(seen)
        for k, v in sorted(mine.items()):
            print(f"{unit} {k}: {v}")
            assert v["scratch"] == 0 and v["vgprs"] <= 256 and v["occupancy"] >= 2, (k, v)
            assert v["lds"] * 8 <= 160 * 1024, (k, v)      # two waves per SIMD are eight workgroups per CU
        counts[unit] = len(mine)
    assert counts == {"k_twisted3_group8": 10, "k_twisted4_group8": 6}   # kernel_instances.h: UAVQP_GROUP8_PAIRS3 / UAVQP_GROUP8_PAIRS4
