"""The batches of the wave form of the finishing gated count (x-search_amd/csrc/xsg_kernels.hip: gated_pass_waves): a wave
selects its next B groups together, locates the batch's candidates in one round trip from a wave-private row of 64 entries
and scans them.  The bindings and the places they aim at are in tests/gate_batch_cases.py (proved on the CPU by tests/
test_gate_batch_cases.py for B = 2, 4 and 8; B here is the build's, read from the kernel's name).  Every case compares count,
three back-to-back count_async calls, count_async_status and count_begin / count_end with the oracle (run_binding /
every_count_call) and asserts that the name carries the batch tag in front of the wave tags, so that a case that fell to
another route fails.
"""
import os
import re

import pytest

import gate_batch_cases as gb
import gate_wave_cases as gw
import xsg
from gate_wave_cases import WAVE_TAG
from test_gpu_gate_spans import SPANS_FIN, oracle_wanted, run_binding
from test_gpu_gate_waves import ENV as WAVE_ENV
from test_gpu_gate_waves import WAVES_FIN, nbytes_of, sketched
from test_gpu_gated_finish import FIN, every_count_call

pytestmark = pytest.mark.gpu
ENV = WAVE_ENV + ("XSG_GATE_BATCH",)


@pytest.fixture(scope="module")
def text():
    return gw.make_text()


def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    return saved


def restore_env(saved):
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.fixture
def sk():
    saved = clean_env()
    s = sketched()
    yield s
    s.close()
    restore_env(saved)


@pytest.fixture(scope="module")
def B(text):
    """the build's batch size, from the name of the wave form on a small binding"""
    saved = clean_env()
    s = sketched()
    try:
        blocks, pat, _ = gw.group_edges(text, 65, False)
        s.bind(blocks)
        s.ctx.set_pattern(pat)
        s.count()
        m = re.search(r" in batches of (\d+)" + re.escape(WAVES_FIN) + "$", s.name())
        assert m, s.name()
        return int(m.group(1))
    finally:
        s.close()
        restore_env(saved)


def batched(B):
    return gb.batch_tag(B) + WAVES_FIN


@pytest.mark.parametrize("k", (0, 1, 2))
def test_round_counts_and_a_batch_that_reaches_past_the_last_group(sk, oracle, text, B, k):
    """exactly B rounds, B + 1, a partial last batch; the last group partial, the needle in the binding's last tile; the
    groups of a batch in different chunks"""
    blocks, pat, flags = gb.BINDINGS[f"rounds{k}"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, ("rounds", B, k), batched(B))
    assert n == len(gb.rounds_spots(sum(gw.tiles_of(blocks))))


@pytest.mark.parametrize("grid", (1, 3))
def test_some_waves_have_an_empty_last_batch_while_others_scan(sk, oracle, text, B, grid):
    blocks, pat, flags = gw.many_groups(text)
    os.environ["XSG_GATE_GRID"] = str(grid)
    assert run_binding(sk, oracle, blocks, pat, flags, ("many groups", grid), batched(B)) == 2 * gw.ngroups(gw.MANY_GROUPS_TILES)


def test_batches_of_0_1_63_64_and_65_candidates(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["counts"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, ("counts", B), batched(B))
    assert n == sum(sum(v) for v in gb.count_plan(B).values())


def test_a_batch_of_64_B_candidates_all_four_spans_set(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["full"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, ("full", B), batched(B)) == 4 * 64 * B


@pytest.mark.parametrize("plen", (4, 8, 32))
def test_two_zone_looks_by_one_wave_inside_one_batch(sk, oracle, text, B, plen):
    blocks, pat, flags = gb.BINDINGS[f"zones{plen}"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, ("zones", plen), batched(B)) == 8


def test_a_long_needle_with_more_sketch_words_than_a_lane_requests_at_once(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["long32"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, "long32", batched(B)) == 18


@pytest.mark.parametrize("hot", ("0", "1"))
def test_both_hot_filters_on_a_binding_of_several_batches(oracle, text, B, hot):
    saved = clean_env()
    os.environ.update(XSG_HOT=hot, XSG_GATE_GRID="1")
    s = sketched()  # (the context reads XSG_HOT when it is made)
    try:
        blocks, pat, flags = gb.BINDINGS["rounds2"](text, B)
        n = run_binding(s, oracle, blocks, pat, flags, ("rounds2", hot), batched(B))
        assert n == len(gb.rounds_spots(sum(gw.tiles_of(blocks))))
        assert s.name().split("stagger")[0].rstrip().endswith("true>" if hot == "1" else "false>")
    finally:
        s.close()
        restore_env(saved)


def test_the_switch_keeps_one_group_at_a_time_in_the_same_build(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["rounds1"](text, B)
    nbytes = nbytes_of(blocks)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, "batches on", batched(B))
    os.environ["XSG_GATE_BATCH"] = "1"  # (re-read at every use under the test hooks)
    assert sk.name().endswith(WAVES_FIN) and "batches" not in sk.name()
    every_count_call(sk, n, nbytes, "batches off", WAVES_FIN)
    assert "batches" not in sk.name()
    os.environ.pop("XSG_GATE_BATCH")
    every_count_call(sk, n, nbytes, "batches on again", batched(B))
    os.environ["XSG_GATE_WAVES"] = "0"  # the workgroup form, as before: no wave tag, no batch tag
    assert sk.name().endswith(SPANS_FIN) and WAVE_TAG not in sk.name() and "batches" not in sk.name()
    every_count_call(sk, n, nbytes, "waves off", SPANS_FIN)
    os.environ.pop("XSG_GATE_WAVES")
    os.environ["XSG_GATE_SPANS"] = "0"  # without the locator: whole-tile reads by the workgroup form
    assert sk.name().endswith(FIN) and "spans" not in sk.name() and "batches" not in sk.name()
    every_count_call(sk, n, nbytes, "spans off", FIN)
    os.environ.pop("XSG_GATE_SPANS")
    # the storing form (a count with newline totals, a list) never carries the tag
    assert "batches" not in sk.name(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES) and "batches" not in sk.name(xsg.MATCH_BYTE_OFFSETS)
    every_count_call(sk, n, nbytes, "everything on again", batched(B))
    assert oracle_wanted(oracle, blocks, pat, flags)[0] == n
