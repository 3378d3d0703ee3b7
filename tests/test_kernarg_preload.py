"""CPU: the solve_twisted_kernel units are built with their leading arguments preloaded into scalar registers (csrc/Makefile:
TWISTED_FLAGS), which works only for a flat argument list -- a struct passed by value is not preloaded.  One instantiation of the
one-tile-per-wave kernel and one of the general kernel are cross-compiled to gfx950 assembly with exactly the flags their unit gets
(`make unit-flags`, so the flag is not repeated here) and the assembly is read:
  * .amdhsa_user_sgpr_kernarg_preload_length >= 10 (five pointers; the batch size makes 11) in both;
  * in the one-tile kernel no s_load stands between the preloaded entry and the first global_load_lds: a wave issues its input loads
    without having fetched anything from the kernarg segment.
The preloaded entry is the second 256-byte block of the kernel: in front of it sits the prologue for firmware that does not preload
(it loads the same registers from the kernarg segment and branches to the entry), closed by `.p2align 8`."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")

# (unit whose flags are taken, template arguments)
ONE = ("k_twisted4_one", "4, 8, 4, 16, true")
GENERAL = ("k_twisted4", "4, 8, 32, 2")


def _make(*args):
    return subprocess.check_output(["make", "-s", "-C", CSRC, *args], text=True).strip()


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    hipcc = _make("print-hipcc")
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} is missing: the library cannot be built here either")
    tmp = tmp_path_factory.mktemp("preload")
    memo = {}

    def get(unit, targs):
        if (unit, targs) not in memo:
            src = tmp / f"{unit}_inst.hip"
            src.write_text('#include "qp_twisted.h"\n'
                           f"template __global__ void uavqp::solve_twisted_kernel<{targs}>(UAVQP_TWISTED_SIG);\n")
            out = tmp / f"{unit}_inst.s"
            flags = _make("unit-flags", f"UNIT={unit}").split()
            subprocess.check_call([hipcc, *flags, "-I", CSRC, "--cuda-device-only", "-S", "-o", str(out), str(src)],
                                  stderr=subprocess.DEVNULL)
            memo[(unit, targs)] = out.read_text().splitlines()
        return memo[(unit, targs)]
    return get


def _preload_length(lines):
    found = [int(m.group(1)) for m in (re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", l) for l in lines) if m]
    assert len(found) == 1, "one kernel, one descriptor"
    return found[0]


def _instructions(lines):
    """(line index, mnemonic) of every instruction line."""
    for i, l in enumerate(lines):
        m = re.match(r"\s+([a-z][a-z0-9_]+)\b", l)
        if m and not l.lstrip().startswith("."):
            yield i, m.group(1)


def test_the_units_get_the_flag_and_no_other_unit_does():
    common = _make("unit-flags", "UNIT=uavqp").split()
    for unit in ("k_twisted3", "k_twisted3_one", "k_twisted4", "k_twisted4_one"):
        flags = _make("unit-flags", f"UNIT={unit}").split()
        assert flags[:len(common)] == common
        assert any(f.startswith("-amdgpu-kernarg-preload-count=") for f in flags[len(common):]), flags
    for unit in ("k_generic", "k_corridor", "k_rows_dual"):
        assert _make("unit-flags", f"UNIT={unit}").split() == common


@pytest.mark.parametrize("unit,targs", [ONE, GENERAL])
def test_leading_arguments_are_preloaded(assembly, unit, targs):
    n = _preload_length(assembly(unit, targs))
    print(f"solve_twisted_kernel<{targs}>: kernarg preload length {n}")
    assert n >= 10


def test_one_tile_kernel_issues_its_loads_without_a_kernarg_fetch(assembly):
    lines = assembly(*ONE)
    label = next(i for i, l in enumerate(lines) if re.match(r"_ZN5uavqp20solve_twisted_kernel\S*:", l))
    entry = next(i for i in range(label + 1, len(lines)) if re.match(r"\s+\.p2align\s+8\b", lines[i]))
    prologue = [op for i, op in _instructions(lines) if label < i < entry]
    assert any(op.startswith("s_load") for op in prologue) and prologue[-1] == "s_branch", prologue   # this IS the compatibility prologue
    body = [(i, op) for i, op in _instructions(lines) if i > entry]
    first_dma = next(k for k, (_, op) in enumerate(body) if op.startswith("global_load_lds"))
    before = [op for _, op in body[:first_dma]]
    print(f"{len(before)} instructions between the preloaded entry and the first global_load_lds")
    assert not [op for op in before if op.startswith("s_load") or op.startswith("s_buffer_load")], before
    # and none anywhere in front of the LAST of the tile's three loads either: every pointer the DMA needs arrived in registers
    last_dma = max(k for k, (_, op) in enumerate(body) if op.startswith("global_load_lds"))
    assert not [op for _, op in body[:last_dma] if op.startswith("s_load")]
