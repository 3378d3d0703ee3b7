"""The (r, M) lists of the register-resident solve, read from csrc/kernel_instances.h: the one source of truth the tests parametrise
over, so that a shape added to a list is covered without editing a test.  A list is a function-like macro of X(r, M) items; it may be
defined through another list (`#define UAVQP_GROUP_PAIRS3_T4(X) UAVQP_TWISTED_PAIRS3(X)`), which is expanded.

    TWISTED          solve_twisted_kernel<R, M, TILE>, every tile, and its ONE instantiation at tiles 4 and 8
    GROUP[tile]      solve_twisted_group_kernel at tile 4 / 8
    GROUP8           solve_twisted_group8_kernel
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")
HEADER = os.path.join(CSRC, "kernel_instances.h")
TILES = (4, 8, 16, 32)                # UAVQP_TWISTED_SHAPES
ONE_TILES = (4, 8)                    # UAVQP_TWISTED_SHAPES_ONE

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)\(X\)[ \t]+(.*)$", re.M)
_ITEM = re.compile(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)|(\w+)\(X\)")


def _logical_lines(text):
    return re.sub(r"\\\r?\n", " ", text)


def read_lists(path=HEADER):
    """{macro name: body} of every `#define NAME(X) ...` of the header."""
    with open(path) as f:
        return dict(_DEFINE.findall(_logical_lines(f.read())))


def expand(name, bodies=None, _seen=()):
    """The (r, M) pairs of list macro `name`, in the order written, lists named in its body expanded in place."""
    bodies = read_lists() if bodies is None else bodies
    if name not in bodies:
        raise KeyError(f"{name}(X) is not defined in kernel_instances.h")
    if name in _seen:
        raise ValueError(f"{name}(X) is defined through itself")
    body = re.sub(r"//.*$", "", bodies[name])
    pairs, left = [], _ITEM.sub("", body)
    if left.strip():
        raise ValueError(f"{name}(X): cannot read {left.strip()!r}")
    for r, M, inner in _ITEM.findall(body):
        pairs.extend(expand(inner, bodies, _seen + (name,)) if inner else [(int(r), int(M))])
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"{name}(X) lists a pair twice")
    return pairs


_B = read_lists()
TWISTED3 = expand("UAVQP_TWISTED_PAIRS3", _B)
TWISTED4 = expand("UAVQP_TWISTED_PAIRS4", _B)
TWISTED = TWISTED4 + TWISTED3
GROUP = {tile: expand(f"UAVQP_GROUP_PAIRS4_T{tile}", _B) + expand(f"UAVQP_GROUP_PAIRS3_T{tile}", _B) for tile in (4, 8)}
GROUP8 = expand("UAVQP_GROUP8_PAIRS4", _B) + expand("UAVQP_GROUP8_PAIRS3", _B)


def has_twisted(r, M):
    return (r, M) in TWISTED


def find_twisted_cases(path=os.path.join(CSRC, "uavqp.hip")):
    """The UAVQP_CASE(r, M) items typed out inside find_twisted() of the host translation unit, from the source text."""
    with open(path) as f:
        text = f.read()
    m = re.search(r"\bfind_twisted\s*\([^)]*\)\s*\{(.*?)\n\}", text, re.S)
    if m is None:
        raise ValueError("find_twisted() not found in uavqp.hip")
    return [(int(r), int(M)) for r, M in re.findall(r"\bUAVQP_CASE\(\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]


def alias(r, M, tile):
    """TwistedCfg<R, M, TILE, LPT>::ALIAS of csrc/qp_twisted.h recomputed: do the staging rows of the emission overwrite the current input
    buffer?  LPT is 2 at tiles 16 and 32 (UAVQP_TWISTED_SHAPES)."""
    lpt = {4: 16, 8: 8, 16: 2, 32: 2}[tile]
    nd, nc, nk = r - 1, 2 * r, M + 1
    in_d = tile * nk * 3 + tile * M + tile * 2 * nd * 3
    ch = 2 if (nc * 8) % 64 == 0 else 4
    stride0 = ch * nc + 2
    stride = stride0 if (stride0 * 2) % 8 == 4 else stride0 + 2
    stage_d = 64 * stride
    return lpt == 2 and r == 3 and (2 * in_d + stage_d) * 8 > 40448
