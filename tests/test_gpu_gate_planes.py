"""The select from bit planes in the wave form of the finishing gated count (x-search_amd/csrc/xsg_kernels.hip:
k_sketch_planes, gated_pass_waves; the layout: xsg_sketch.h, tests/test_plane_layout.py).  A binding with a span locator
also holds its sketch transposed -- one 64-bit word per (bit, group of 64 tiles) -- and a wave selects a group's candidates as
the AND of one word per gram of the needle; a candidate's chunk number is read in the locate phase.  The bindings are those
of tests/gate_wave_cases.py and tests/gate_batch_cases.py, which aim at the dealing, the row and the rounds; every case
compares count, three back-to-back count_async calls, count_async_status and count_begin / count_end with the oracle
(run_binding / every_count_call) and asserts that the name carries the plane tag in front of the batch and wave tags, so
that a case that fell back to the select from sketch words fails.
"""
import os

import numpy as np
import pytest

import gate_batch_cases as gb
import gate_wave_cases as gw
import xsg
from gate_wave_cases import WAVE_TAG
from test_gpu_gate_batch import B  # noqa: F401  (fixture: the build's batch size)
from test_gpu_gate_batch import ENV as BATCH_ENV
from test_gpu_gate_batch import batched
from test_gpu_gate_spans import SPANS_FIN, oracle_wanted, run_binding
from test_gpu_gate_waves import nbytes_of, sketched
from test_gpu_gated_finish import FIN, count_with_status, every_count_call
from test_gpu_sketch_select import async_many, build_with_absent_needle

pytestmark = pytest.mark.gpu
PLANE_TAG = " from bit planes"
ENV = BATCH_ENV + ("XSG_GATE_PLANES",)
EDGE_TILES = (1, 63, 64, 65, 1023, 1024, 1025)  # a lane behind ntiles, a partial last group, the 16-group line and staging block


def planed(B):
    return PLANE_TAG + batched(B)


@pytest.fixture(scope="module")
def text():
    return gw.make_text()


@pytest.fixture(scope="module")
def big(text):
    """filler for the bindings of more tiles than the text has"""
    t = gb.long_text(text, max(EDGE_TILES) + 1)
    t.setflags(write=False)
    return t


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


# ---- group and line edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunked", (False, True), ids=("one_chunk", "chunks"))
@pytest.mark.parametrize("ntiles", EDGE_TILES)
def test_group_and_line_edges(sk, oracle, big, B, ntiles, chunked):
    """the needle in the first and the last tile of every group and in the binding's last tile; 1023 .. 1025 tiles end
    at, one short of and one behind the 16th group: the plane line and the transposer's staging block"""
    blocks, pat, flags = gw.group_edges(big, ntiles, chunked)
    want = len(gw.edge_spots(ntiles))
    if ntiles >= gw.GROUP - 1:
        assert run_binding(sk, oracle, blocks, pat, flags, ("group edges", ntiles, chunked), planed(B)) == want
        return
    # One tile, and it holds the needle: a synchronous count's verdict (a quarter of the sampled tiles or more pass) would
    # switch the gate off, so this binding is counted by the stream-ordered calls, which gate without a verdict.
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    assert oracle_wanted(oracle, blocks, pat, flags)[0] == want
    sk.ctx.set_pattern(pat)
    assert sk.name().endswith(planed(B)), sk.name()
    assert async_many(sk) == [want] * 3
    assert count_with_status(sk) == ([want, 0, 0, nbytes_of(blocks)], 0)
    assert sk.name().endswith(planed(B)), sk.name()


# ---- the dealing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", (1, 3))
def test_more_groups_than_waves(sk, oracle, text, B, grid):
    blocks, pat, flags = gw.many_groups(text)
    os.environ["XSG_GATE_GRID"] = str(grid)
    assert run_binding(sk, oracle, blocks, pat, flags, ("many groups", grid), planed(B)) == 2 * gw.ngroups(gw.MANY_GROUPS_TILES)


# ---- row sizes and rounds ------------------------------------------------------------------------------------------------
def test_rows_of_0_1_63_64_and_65_candidates(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["counts"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, ("counts", B), planed(B))
    assert n == sum(sum(v) for v in gb.count_plan(B).values())


def test_a_batch_of_64_B_candidates_takes_its_groups_one_at_a_time(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["full"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, ("full", B), planed(B)) == 4 * 64 * B


@pytest.mark.parametrize("k", (0, 1, 2))
def test_round_counts_with_the_groups_of_a_batch_in_different_chunks(sk, oracle, text, B, k):
    """the candidate's chunk number, read in the locate phase, decides its geometry: chunks of 1 .. 7 tiles"""
    blocks, pat, flags = gb.BINDINGS[f"rounds{k}"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, ("rounds", B, k), planed(B))
    assert n == len(gb.rounds_spots(sum(gw.tiles_of(blocks))))


# ---- a 32-byte needle: 29 grams, two of them in one sketch word ----------------------------------------------------------
def test_all_29_grams_of_a_32_byte_needle_go_through_the_planes(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["long32"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, "long32", planed(B)) == 18


# ---- zones and hot filters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plen", (4, 8, 32))
def test_zone_looks_of_candidates_selected_from_the_planes(sk, oracle, text, B, plen):
    blocks, pat, flags = gb.BINDINGS[f"zones{plen}"](text, B)
    os.environ["XSG_GATE_GRID"] = "1"
    assert run_binding(sk, oracle, blocks, pat, flags, ("zones", plen), planed(B)) == 8


@pytest.mark.parametrize("hot", ("0", "1"))
def test_both_hot_filters(oracle, text, B, hot):
    saved = clean_env()
    os.environ.update(XSG_HOT=hot, XSG_GATE_GRID="1")
    s = sketched()  # (the context reads XSG_HOT when it is made)
    try:
        blocks, pat, flags = gb.BINDINGS["rounds2"](text, B)
        n = run_binding(s, oracle, blocks, pat, flags, ("rounds2", hot), planed(B))
        assert n == len(gb.rounds_spots(sum(gw.tiles_of(blocks))))
        assert s.name().split("stagger")[0].rstrip().endswith("true>" if hot == "1" else "false>")
    finally:
        s.close()
        restore_env(saved)


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_the_switch_keeps_the_select_from_sketch_words_in_the_same_build(sk, oracle, text, B):
    blocks, pat, flags = gb.BINDINGS["rounds1"](text, B)
    nbytes = nbytes_of(blocks)
    os.environ["XSG_GATE_GRID"] = "1"
    n = run_binding(sk, oracle, blocks, pat, flags, "planes on", planed(B))
    os.environ["XSG_GATE_PLANES"] = "0"  # (re-read at every use under the test hooks)
    assert sk.name().endswith(batched(B)) and PLANE_TAG not in sk.name()
    every_count_call(sk, n, nbytes, "planes off", batched(B))
    assert PLANE_TAG not in sk.name()
    os.environ.pop("XSG_GATE_PLANES")
    every_count_call(sk, n, nbytes, "planes on again", planed(B))
    os.environ["XSG_GATE_WAVES"] = "0"  # the workgroup form reads the sketch words: no plane tag
    assert sk.name().endswith(SPANS_FIN) and WAVE_TAG not in sk.name() and PLANE_TAG not in sk.name()
    every_count_call(sk, n, nbytes, "waves off", SPANS_FIN)
    os.environ.pop("XSG_GATE_WAVES")
    os.environ["XSG_GATE_SPANS"] = "0"  # without the locator: no wave form, no plane tag
    assert sk.name().endswith(FIN) and "spans" not in sk.name() and PLANE_TAG not in sk.name()
    every_count_call(sk, n, nbytes, "spans off", FIN)
    os.environ.pop("XSG_GATE_SPANS")
    os.environ["XSG_GATE_BATCH"] = "1"  # one group at a time still selects from the planes
    every_count_call(sk, n, nbytes, "batches off", PLANE_TAG + gw.WAVE_TAG + SPANS_FIN)
    os.environ.pop("XSG_GATE_BATCH")
    # the storing form (a count with newline totals, a list) never carries the tag
    assert PLANE_TAG not in sk.name(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES) and PLANE_TAG not in sk.name(xsg.MATCH_BYTE_OFFSETS)
    every_count_call(sk, n, nbytes, "everything on again", planed(B))
    assert oracle_wanted(oracle, blocks, pat, flags)[0] == n


# ---- re-binding ----------------------------------------------------------------------------------------------------------
def test_the_planes_are_rebuilt_with_the_sketch_on_a_second_binding(sk, oracle, text, big, B):
    """the same object bound to other bytes, the needle in other tiles of other groups: planes left over from the first
    binding would select the wrong tiles and lose occurrences"""
    first, pat, flags = gw.many_groups(text)
    n1 = run_binding(sk, oracle, first, pat, flags, "first binding", planed(B))
    second, pat2, flags2 = gw.group_edges(big, 1025, True)
    assert pat2 == pat
    n2 = run_binding(sk, oracle, second, pat2, flags2, "second binding", planed(B))
    assert (n1, n2) == (2 * gw.ngroups(gw.MANY_GROUPS_TILES), len(gw.edge_spots(1025)))
    # and back, on fewer tiles than the buffers hold
    third = [np.ascontiguousarray(b) for b in first[:2]]
    n3 = run_binding(sk, oracle, third, pat, flags, "third binding", planed(B))
    assert n3 == oracle_wanted(oracle, third, pat, flags)[0] > 0


# ---- one chunk: no tile_chunk ---------------------------------------------------------------------------------------------
def test_a_binding_of_one_chunk_has_no_chunk_numbers_to_read(sk, oracle, text, B):
    blocks, pat, flags = gw.group_edges(text, 257, False)
    assert len(blocks) == 1
    for grid in ("1", None):
        os.environ.pop("XSG_GATE_GRID", None)
        if grid:
            os.environ["XSG_GATE_GRID"] = grid
        assert run_binding(sk, oracle, blocks, pat, flags, ("one chunk", grid), planed(B)) == len(gw.edge_spots(257))
