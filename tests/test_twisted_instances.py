"""CPU: the lists tests/twisted_instances.py reads from csrc/kernel_instances.h are the lists the code goes by.  The header's own
predicates (compiled with g++, no HIP runtime), the hand-typed UAVQP_CASE list of find_twisted() in csrc/uavqp.hip, the tables other tests
hard-code, and the set of instances whose staging rows alias the input buffer (TwistedCfg::ALIAS, csrc/qp_twisted.h) must all agree with
them: tests/test_gpu_twisted_every_instance.py parametrises over these lists and names the ALIAS set."""
import os
import shutil
import subprocess

import pytest

import twisted_instances as TI


def test_the_lists_have_the_instances_the_header_documents():
    assert len(TI.TWISTED3) == 10 and len(TI.TWISTED4) == 10 and len(set(TI.TWISTED)) == 20
    assert all(r == 3 for r, _ in TI.TWISTED3) and all(r == 4 for r, _ in TI.TWISTED4)
    assert len(TI.GROUP[4]) == 16 and len(TI.GROUP[8]) == 12 and len(TI.GROUP8) == 16
    # a list defined through another list is expanded: UAVQP_GROUP_PAIRS3_T4(X) is UAVQP_TWISTED_PAIRS3(X)
    assert [p for p in TI.GROUP[4] if p[0] == 3] == TI.TWISTED3
    # every group kernel replays launches of a one-tile-per-wave kernel of its shape
    assert set(TI.GROUP[4]) <= set(TI.TWISTED) and set(TI.GROUP[8]) <= set(TI.TWISTED) and set(TI.GROUP8) <= set(TI.GROUP[4])


def test_expansion_of_nested_and_malformed_lists():
    bodies = {"A": "X(4, 2) X(3,5)", "B": "A(X) X(4, 9)   // trailing words (4, 7)", "C": "B(X) A(X)", "D": "D(X)", "E": "X(4, 2) Y(4, 3)"}
    assert TI.expand("A", bodies) == [(4, 2), (3, 5)]
    assert TI.expand("B", bodies) == [(4, 2), (3, 5), (4, 9)]
    for bad, err in (("C", ValueError), ("D", ValueError), ("E", ValueError), ("F", KeyError)):
        with pytest.raises(err):
            TI.expand(bad, bodies)


def test_predicates_of_the_header_agree_with_the_parsed_lists(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp_path / "twisted_instances_exist")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", TI.CSRC,
                           os.path.join(TI.ROOT, "tests", "cpp", "twisted_instances_exist.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert [(r, M) for r, M, *_ in rows] == [(r, M) for r in (3, 4) for M in range(1, 25)]
    for r, M, g4, g8, eight in rows:
        assert bool(g4) == ((r, M) in TI.GROUP[4]), (r, M, "uavqp_twisted_group_exists at tile 4")
        assert bool(g8) == ((r, M) in TI.GROUP[8]), (r, M, "uavqp_twisted_group_exists at tile 8")
        assert bool(eight) == ((r, M) in TI.GROUP8), (r, M, "uavqp_twisted_group8_exists")
    # nothing of the lists lies outside the range asked about
    assert all(r in (3, 4) and 1 <= M <= 24 for r, M in TI.GROUP[4] + TI.GROUP[8] + TI.GROUP8)


def test_find_twisted_cases_are_exactly_the_compiled_pairs():
    """A pair only in find_twisted() is instantiated by the host translation unit, unseen; a pair only in the lists is compiled and never launched."""
    cases = TI.find_twisted_cases()
    assert len(cases) == len(set(cases)), "a pair is typed twice"
    assert set(cases) - set(TI.TWISTED) == set(), "launched, but in no instance list"
    assert set(TI.TWISTED) - set(cases) == set(), "compiled, but never launched"


def test_hard_coded_tables_of_other_tests_agree_with_the_parsed_lists():
    import test_gpu_capture_fuse as F
    import test_gpu_twisted_group8 as G
    assert G.HAS_GROUP8 and F.HAS_GROUP
    for (r, M), has in G.HAS_GROUP8.items():
        assert has == ((r, M) in TI.GROUP8), (r, M)
    for (r, M, tile), has in F.HAS_GROUP.items():
        assert has == ((r, M) in TI.GROUP[tile]), (r, M, tile)


def test_alias_set_is_the_one_the_gpu_test_names():
    """TwistedCfg::ALIAS recomputed from the formulas of qp_twisted.h over every compiled instance.  If the LDS budget changes and with
    it this set, ALIAS of tests/test_gpu_twisted_every_instance.py has to follow."""
    got = {(r, M, tile) for r, M in TI.TWISTED for tile in TI.TILES if TI.alias(r, M, tile)}
    assert got == {(3, 10, 32), (3, 12, 32), (3, 16, 32)}
    with open(os.path.join(TI.CSRC, "qp_twisted.h")) as f:
        text = " ".join(f.read().split())
    # the formulas recomputed are the ones in the header (TI.alias has to follow an edit of these lines)
    assert "ALIAS = LPT == 2 && R == 3 && (2 * IN_D + STAGE_D) * 8 > 40448;" in text
    assert "CH = (NC * 8) % 64 == 0 ? 2 : 4;" in text and "STAGE_D = 64 * STAGE_STRIDE;" in text
    assert "STAGE_STRIDE0 = CH * NC + 2;" in text and "STAGE_STRIDE = (STAGE_STRIDE0 * 2) % 8 == 4 ? STAGE_STRIDE0 : STAGE_STRIDE0 + 2;" in text
    assert "IN_D = WP_D + T_D + BC_D;" in text
