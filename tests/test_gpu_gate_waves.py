"""The wave form of the finishing gated count (x-search_amd/csrc/xsg_kernels.hip: gated_pass_waves): a wave owns a sketch
group of 64 tiles from its sketch words to its text, and no wave waits for another before the kernel's end.  The bindings
and the dealing they aim at are in tests/gate_wave_cases.py (proved on the CPU by tests/test_gate_wave_cases.py); here
every case compares count, three back-to-back count_async calls, count_async_status and count_begin / count_end with the
oracle (helpers of tests/test_gpu_gate_spans.py and tests/test_gpu_gated_finish.py) and asserts that the name carries the
wave tag.  A barrier left on a path that one wave takes alone would hang the unbalanced cases; they are small, and what is
asserted is their result.
"""
import os

import pytest

import gate_wave_cases as gw
import xsg
from gate_wave_cases import WAVE_TAG
from test_gpu_gate_spans import SPANS_FIN, oracle_wanted, run_binding
from test_gpu_gated_finish import FIN, every_count_call
from test_gpu_sketch import Sketched

pytestmark = pytest.mark.gpu
WAVES_FIN = WAVE_TAG + SPANS_FIN
ENV = ("XSG_SKETCH", "XSG_GATE_GRID", "XSG_GATE_SPANS", "XSG_GATE_WAVES", "XSG_HOT")


@pytest.fixture(scope="module")
def text():
    return gw.make_text()


def sketched():
    s = Sketched()
    s.status = s.torch.zeros(1, dtype=s.torch.int64, device="cuda:0")
    return s


@pytest.fixture
def sk():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    s = sketched()
    yield s
    s.close()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def nbytes_of(blocks):
    return sum(int(b.size) for b in blocks)


@pytest.mark.parametrize("chunked", (False, True), ids=("one_chunk", "chunks"))
@pytest.mark.parametrize("ntiles", gw.GROUP_EDGE_TILES)
def test_group_edges(sk, oracle, text, ntiles, chunked):
    """the needle in the first and the last tile of every group and in the binding's last tile: a lane at or beyond
    ntiles does not pass, a partial last group loses nothing"""
    blocks, pat, flags = gw.group_edges(text, ntiles, chunked)
    n = run_binding(sk, oracle, blocks, pat, flags, ("group edges", ntiles, chunked), WAVES_FIN)
    assert n == len(gw.edge_spots(ntiles))


@pytest.mark.parametrize("grid", (1, 3))
def test_more_groups_than_waves(sk, oracle, text, grid):
    blocks, pat, flags = gw.many_groups(text)
    os.environ["XSG_GATE_GRID"] = str(grid)
    assert run_binding(sk, oracle, blocks, pat, flags, ("many groups", grid), WAVES_FIN) == 2 * gw.ngroups(gw.MANY_GROUPS_TILES)


@pytest.mark.parametrize("name", ("one_busy_wave", "three_busy_waves"))
def test_all_the_work_in_some_waves_of_a_workgroup(sk, oracle, text, name):
    """256 (tile, span) pairs in each busy wave while the others of the workgroup have none"""
    blocks, pat, flags = gw.BINDINGS[name](text)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, name, WAVES_FIN)
    assert n == 4 * gw.GROUP * (1 if name == "one_busy_wave" else 3)


@pytest.mark.parametrize("plen", (28, 32, 40))
def test_long_needles_verified_by_waves_1_2_3_against_the_staged_pattern(sk, oracle, text, plen):
    blocks, pat, flags = gw.long_staged(text, plen)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, ("long", plen), WAVES_FIN) == 18


@pytest.mark.parametrize("plen", (4, 8, 32))
def test_zone_looks_by_two_waves_in_the_same_round(sk, oracle, text, plen):
    blocks, pat, flags = gw.zone_pairs(text, plen)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, ("zones", plen), WAVES_FIN)
    assert n == 8  # zone only, ahead only, both: 1 + 1 + 2 per chunk of a pair
    os.environ.pop("XSG_GATE_GRID")
    every_count_call(sk, n, nbytes_of(blocks), ("zones", plen, "default grid"), WAVES_FIN)


@pytest.mark.parametrize("hot", ("0", "1"))
def test_several_spans_of_one_tile_in_one_wave(oracle, text, hot):
    """one span each, all four, two in one span, one occurrence straddling spans 1 and 2 -- under both hot filters"""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(XSG_SKETCH="1", XSG_HOT=hot)
    s = sketched()  # (the context reads XSG_HOT when it is made)
    try:
        blocks, pat, flags = gw.BINDINGS["span_patterns"](text)
        assert run_binding(s, oracle, blocks, pat, flags, ("span patterns", hot), WAVES_FIN) == 11
        assert s.name().split("stagger")[0].rstrip().endswith("true>" if hot == "1" else "false>")
    finally:
        s.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_the_switches_keep_the_workgroup_form_in_the_same_build(sk, oracle, text):
    blocks, pat, flags = gw.many_groups(text)
    nbytes = nbytes_of(blocks)
    n = run_binding(sk, oracle, blocks, pat, flags, "waves on", WAVES_FIN)
    os.environ["XSG_GATE_WAVES"] = "0"  # (re-read at every use under the test hooks)
    assert sk.name().endswith(SPANS_FIN) and WAVE_TAG not in sk.name()
    every_count_call(sk, n, nbytes, "waves off", SPANS_FIN)
    assert WAVE_TAG not in sk.name()
    os.environ.pop("XSG_GATE_WAVES")
    every_count_call(sk, n, nbytes, "waves on again", WAVES_FIN)
    for waves in (None, "0", "1"):  # without the locator: the workgroup form, whatever XSG_GATE_WAVES says
        os.environ["XSG_GATE_SPANS"] = "0"
        os.environ.pop("XSG_GATE_WAVES", None)
        if waves is not None:
            os.environ["XSG_GATE_WAVES"] = waves
        assert sk.name().endswith(FIN) and WAVE_TAG not in sk.name() and "spans" not in sk.name(), (waves, sk.name())
        every_count_call(sk, n, nbytes, ("spans off", waves), FIN)
    os.environ.pop("XSG_GATE_SPANS")
    os.environ.pop("XSG_GATE_WAVES", None)
    # the storing form (a count with newline totals, a list) never carries the tag
    assert WAVE_TAG not in sk.name(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES) and WAVE_TAG not in sk.name(xsg.MATCH_BYTE_OFFSETS)
    assert sk.name().endswith(WAVES_FIN)
    n2, _ = oracle_wanted(oracle, blocks, pat, flags)
    assert n2 == n
