"""CPU: every instantiation of solve_twisted_group8_kernel (csrc/qp_twisted.h) fits THREE waves per SIMD -- no scratch, at most 168
VGPRs (512 / 3 rounded down to the allocation granule of 8), the compiler's own occupancy figure at least 3, and twelve workgroups of
its LDS in the 160 KiB of a CU.  Read, as tests/test_twisted_group8_resources.py reads its bound of two, from a cross-compile of the two
units to gfx950 with the flags `make unit-flags` reports; that those are the flags the library's build gives the units is checked
against the command lines `make -n` prints for their objects.

Before the copy-out decode of qp_twisted_body.h (EMIT2) was taken out of the elimination's live range, (4, 8) took 182 VGPRs and
(3, 16) 226: two waves per SIMD.  (3, 16) is also the one shape whose input tile and full staging area (14336 bytes) are more than a
twelfth of the LDS; its idle lane pairs do not write and their rows are not allocated (TwistedCfg::IDLE_ROWS2): 13056 bytes.

The LDS bound counts bytes as the kernel declares them, as the compiler's occupancy figure does.  In what granule the hardware allocates
LDS to a workgroup is not known here (qp_twisted.h, at IDLE_ROWS2): if it rounds up to 1280 bytes, (3, 12) and (3, 16) hold eleven
workgroups per CU, not twelve, and this test does not see it."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")
UNITS = ("k_twisted3_group8", "k_twisted4_group8")
VGPR_MAX = 512 // 3 // 8 * 8
LDS_PER_CU = 160 * 1024


def _make(*args):
    return subprocess.check_output(["make", "-s", "-C", CSRC, *args], text=True).strip()


def test_vgpr_bound_is_the_third_of_the_file():
    assert VGPR_MAX == 168 and 3 * VGPR_MAX <= 512 < 3 * (VGPR_MAX + 8)


def test_unit_flags_are_the_flags_of_the_build(tmp_path):
    """`make -n` with an object directory of its own prints the compile line of every unit without running it."""
    lines = subprocess.check_output(["make", "-n", "-C", CSRC, f"OBJDIR={tmp_path}/obj", f"OUT={tmp_path}/libuavqp.so"], text=True).splitlines()
    for unit in UNITS:
        flags = _make("unit-flags", f"UNIT={unit}").split()
        mine = [ln for ln in lines if re.search(r"-c -o \S+/%s\.o %s\.hip\s*$" % (unit, unit), ln)]
        assert len(mine) == 1, (unit, mine)
        words = shlex.split(mine[0])
        build = [w for w in words[1:] if not w.startswith("-DUAVQP_SRC_HASH=")]
        build = build[:build.index("-c")]
        assert build == flags, (unit, build, flags)


def test_group8_kernels_fit_three_waves_per_simd(tmp_path):
    hipcc = _make("print-hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} is missing: the library cannot be built here either")
    procs = []
    for unit in UNITS:
        flags = _make("unit-flags", f"UNIT={unit}").split()
        procs.append(subprocess.Popen([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / f"{unit}.o"),
                                       os.path.join(CSRC, f"{unit}.hip")], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True))
    counts = {}
    for unit, p in zip(UNITS, procs):
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
            assert v["scratch"] == 0 and v["vgprs"] <= VGPR_MAX and v["occupancy"] >= 3, (k, v)
            assert v["lds"] * 12 <= LDS_PER_CU, (k, v)      # three waves per SIMD are twelve one-wave workgroups per CU
        counts[unit] = len(mine)
    assert counts == {"k_twisted3_group8": 10, "k_twisted4_group8": 6}   # kernel_instances.h: UAVQP_GROUP8_PAIRS3 / UAVQP_GROUP8_PAIRS4
