"""The literal-list route at its grid, walk, fold, hash and NUL edges (tests/set_edge_cases.py; tests/test_set_edge_cases.py
proves without a GPU that every case reaches its edge).  Every case compares all seven tags, the split-phase count, both
views and XSG_MATCHES (set_gpu_util.list_all_modes / check_matches) with set_cases.expected: exact equality throughout."""
from functools import lru_cache

import numpy as np
import pytest

import set_cases as SC
import set_edge_cases as E
import set_model
from gpu_util import GpuSearch
from set_gpu_util import IC, bind_tight, check, check_matches, list_all_modes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    g = GpuSearch()
    yield g
    g.ctx.close()


def search_and_check(gs, oracle, blocks, lits, flags, what, want=None):
    blocks = list(blocks)
    want = want or SC.expected(oracle, blocks, lits, bool(flags & IC))
    check(list_all_modes(gs, lits, flags), want, what)
    check_matches(gs, blocks, lits, flags, what)
    return want


# ---- A. the bounded grid of k_set_scan loops ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    import torch
    return E.GRID_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("layout", ["upload", "tight"])
def test_grid_stride(gs, oracle, grid, layout):
    """more than 2 * grid tiles, so every workgroup of k_set_scan takes a second tile and a quarter of them a third: hit
    and no-hit tiles alternate per workgroup in both orders, consecutive tiles of a workgroup lie in different chunks,
    some tiles hold candidates and no match; plain and ignore-case; once packed tightly with stale matches and the
    completing bytes behind the chunk ends"""
    case = E.grid_case(grid)
    tiles = E.tiles_of(case.blocks)
    if layout == "tight":
        bind_tight(gs, case.blocks, E.grid_fill(case))
    else:
        gs.bind(list(case.blocks))
    for flags in (0, IC):
        want = search_and_check(gs, oracle, case.blocks, E.GRID_LITS, flags, (layout, flags))
        starts = np.asarray(want["match_byte_offsets"], dtype=np.int64)
        at = np.cumsum([0] + [int(b.size) for b in case.blocks])
        lo = np.array([at[c] + o for c, o in tiles], dtype=np.int64)
        hi = np.array([at[c] + min(o + E.TILE, int(case.blocks[c].size)) for c, o in tiles], dtype=np.int64)
        hit = (np.searchsorted(starts, lo) < np.searchsorted(starts, hi)).tolist()
        E.grid_conditions(case, grid, hit)  # the case built for the device's own grid meets its conditions


# ---- B. the walk past 2^19 candidates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,blocks,lits", [("periodic", E.walk_periodic, E.PERIODIC_LITS), ("long-cover", E.walk_long_cover, E.COVER_LITS)],
                         ids=["periodic", "long-cover"])
def test_walk_blocks(gs, oracle, name, blocks, lits):
    """more than 524 288 + 2048 candidates in one chunk: k_rx_block_max_scan's second iteration with its carry, heads,
    covered candidates and kept non-heads as the first of a thread's items, of a wave, of a block and of a scan iteration;
    a second chunk whose candidates lie below the first one's last end"""
    blocks = blocks()
    gs.bind(list(blocks))
    want = search_and_check(gs, oracle, blocks, lits, 0, name)
    assert want["count_matches"] > 300_000


# ---- C. fold4 against set_fold -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,gi", E.FOLD_CASES, ids=["g%d-%s" % (g, E.FOLD_GROUPS[gi].name) for g, gi in E.FOLD_CASES])
def test_fold(gs, oracle, g, gi):
    """every byte value but '\\n' at every gram position and behind the gram, verbatim, case-swapped and replaced by its
    false partner, at every byte of a lane's w[0..4], under XSG_FLAG_IGNORE_CASE; four of the lists also without it"""
    case = E.fold_case(g, gi)
    gs.bind(list(case.blocks))
    want = search_and_check(gs, oracle, case.blocks, case.lits, IC, case.name)
    assert want["count_matches"] >= 16 * len(case.lits) - 2
    if (g, gi) in E.FOLD_PLAIN:
        search_and_check(gs, oracle, case.blocks, case.lits, 0, (case.name, "plain"))


# ---- D. false positives of the hashed filter, and the list's limits ---------------------------------------------------------------------
@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [3, 4])
def test_hash_collisions(gs, oracle, g, icase):
    """grams with a literal gram's filter bit that are not that gram, followed by the literal's rest: candidates that
    k_set_verify must answer with 0 (the `keys[lo] != v` test behind its binary search)"""
    lits, blocks, fakes = E.collision_case(g)
    gs.bind(list(blocks))
    want = search_and_check(gs, oracle, blocks, lits, IC if icase else 0, (g, icase))
    assert want["count_matches"] >= 4 * len(lits) + 4


@lru_cache(maxsize=None)
def limit_expected(oracle, name):
    """computed once for both rounds.  The list of 4096 distinct grams comes from tests/set_model.py: the oracle's reader
    compiles its 4096 alternatives at once but tries them at every position, four seconds for this text;
    test_set_edge_cases.py::test_limit_texts_hold_the_planted_literals pins the model to the reader on this very case"""
    blocks, lits = list(E.limit_blocks().blocks), dict(E.LIMIT_LISTS)[name]()
    return set_model.all_modes(blocks, lits) if name == "distinct" else SC.expected(oracle, blocks, lits)


def test_list_limits_on_one_context(gs, oracle):
    """small list, 4096 literals under one gram, one 255-byte literal, 4096 literals under 4096 grams -- twice in that
    order on one context, so d_pat grows, shrinks in use and is reused: the repeats must equal the first round.  The text
    holds the first-listed, a middle and the last-listed literal of each list; the shared-gram list meets a chunk end with
    5 bytes of room, where the 7-byte literals listed first do not fit (the bytes that complete one lie behind the end)
    and the 5-byte literal listed behind them does"""
    case = E.limit_blocks()
    bind_tight(gs, case.blocks, E.limit_fill(case))
    first = {}
    for rnd in (0, 1):
        for name, lits in E.LIMIT_LISTS:
            lits = lits()
            want = limit_expected(oracle, name)
            got = list_all_modes(gs, lits)
            check(got, want, (rnd, name))
            check_matches(gs, list(case.blocks), lits, 0, (rnd, name))
            m = gs.shard.search_matches()
            if rnd == 0:
                first[name] = (got, m[0], m[1].tolist())
            else:
                assert (got, m[0], m[1].tolist()) == first[name], name
    assert E.ROOM_SHORT in first["shared"][1]


# ---- E. NUL bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["upload", "tight"])
@pytest.mark.parametrize("k", range(len(E.NUL_LISTS)))
def test_nul_bytes(gs, oracle, k, layout):
    """literals of NUL bytes: the zeros that k_set_scan substitutes for units behind the padded end, the zero pads of
    gpu_util.upload and of a tight packing, and the chunk of NULs that follows are exactly the bytes that would complete
    an occurrence cut at a chunk's end"""
    blocks = E.nul_blocks()
    if layout == "tight":
        bind_tight(gs, blocks, lambda i, n: np.zeros(n, dtype=np.uint8))
    else:
        gs.bind(blocks)
    for flags in (0, IC):
        search_and_check(gs, oracle, blocks, E.NUL_LISTS[k], flags, (k, layout, flags))
