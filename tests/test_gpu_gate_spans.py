"""The span locator in the finishing form of the gated count: k_scan_fin reads, of a candidate tile, only the 4 KiB spans
whose own bits hold the needle's grams (x-search_amd/csrc/xsg_sketch.h: span_hash, span_entries; xsg_kernels.hip:
gated_pass<..., FIN>, scan_tile_at's span_on).  A span that is skipped wrongly loses its matches, so every case compares
count, three back-to-back count_async calls, count_async_status and count_begin / count_end with the oracle, and asserts the
name of the form that ran.

XSG_SKETCH=1 and XSG_SKETCH_MIN_BYTES=0; helpers of tests/test_gpu_gated_finish.py (Sketched, plant, check,
every_count_call) are reused.  Every binding is made by a function of the module's text alone, so that a fresh child
process -- where XSG_GATE_SPANS=0 is read once -- rebuilds the same bindings and reports its numbers for whole-tile reads.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import span_sketch_model as spm
import test_gpu_sketch as base
import xsg
from test_gpu_gated_finish import FIN, LETTERS, check, count_with_status, every_count_call, wanted
from test_gpu_sketch import GATED, TILE, Sketched
from test_gpu_sketch_select import async_many, build_with_absent_needle, plant

pytestmark = pytest.mark.gpu
SPAN = 4096
SPANS_FIN = " by 4 KiB spans finishing (xsg::k_scan_fin)" + GATED
TEXT_TILES = 700


def make_text():
    rng = np.random.Generator(np.random.PCG64(4096))
    t = base._text(rng, TEXT_TILES * TILE)
    t.setflags(write=False)
    return t


def needle(plen):
    return LETTERS[:plen]


def flags_of(plen):
    """a needle beyond the wave walk's reach finishes in its pass only without a zone: exact tail (kLong with koff > 0)"""
    return xsg.FLAG_EXACT_TAIL if plen > 33 else 0


# ---- the bindings: name -> (blocks, pattern, flags) --------------------------------------------------------------------
def quiet(text, tiles, salt=0):
    """a chunk without a needle that keeps the share of passing tiles under the verdict's quarter"""
    return text[(salt * 131 % 50) * TILE:][:tiles * TILE + 3].copy()


def borders(text, plen):
    """window starts at tile-relative 4095/4096, 8191/8192, 12287/12288, 16383/16384 for every filter window offset a
    needle of this length can have (the occurrence starts koff bytes ahead of its window), and needles straddling each
    border; every occurrence in a tile of its own, two tiles apart"""
    pat = needle(plen)
    back = range(0, plen - 6) if plen > 8 else (0,)  # koff: 0 .. plen - 8
    rel = sorted({-1 - d for d in back} | {-d for d in back} | {-(plen // 2), -(plen - 1), -3})
    spots = [(2 * k + 1) * TILE + b + r for k, (b, r) in enumerate((b, r) for b in (SPAN, 2 * SPAN, 3 * SPAN, TILE) for r in rel)]
    assert spots[-1] + 2 * TILE < (TEXT_TILES - 60) * TILE
    a = text[:spots[-1] + 2 * TILE + 77].copy()
    plant(a, pat, spots)
    return [a, quiet(text, min(8 * len(spots), TEXT_TILES - 60), plen)], pat, flags_of(plen)


def span_patterns(text):
    """a tile with an occurrence in exactly one span, for each of the four; one with an occurrence in all four; one with two
    in the same span; one whose only occurrence straddles spans 1 and 2"""
    pat = needle(8)
    a = text[:40 * TILE + 5].copy()
    spots = [(2 + 3 * s) * TILE + s * SPAN + 1000 + 17 * s for s in range(4)]
    spots += [20 * TILE + s * SPAN + 300 + s for s in range(4)]
    spots += [26 * TILE + 2 * SPAN + 64, 26 * TILE + 2 * SPAN + 3000]
    spots += [30 * TILE + 2 * SPAN - 4]
    plant(a, pat, spots)
    return [a, quiet(text, 200, 3)], pat, 0


def chunk_ends(text, plen):
    """chunks of k * TILE + r bytes that end inside span 0, 1, 2 and 3 of their last tile, r around each span border and
    around plen + 31 (the zone's length): the needle in the zone only, ahead of the zone only, in both"""
    pat = needle(plen)
    rs = sorted({s * SPAN + d for s in range(4) for d in (-1, 0, 1, plen + 30, plen + 31, plen + 32) if s * SPAN + d >= 1} | {TILE - 1})
    blocks = []
    for i, r in enumerate(rs):
        L = 2 * TILE + r
        Z = L - plen - 31
        for j, spots in enumerate(([L - plen], [Z - 2 * plen - 3], [Z - 2 * plen - 3, L - plen], [Z, Z - plen - 1])):
            b = text[((7 * i + j) % 40) * TILE + 11 * i:][:L].copy()
            plant(b, pat, spots)
            blocks.append(b)
    tiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    blocks.append(quiet(text, min(4 * tiles, TEXT_TILES - 60), plen))
    return blocks, pat, 0


def tiny_chunks(text):
    """many chunks of less than a tile (tile_chunk is in play) between larger ones, more than 2 x 256 tiles in all: several
    units per workgroup under a small grid, the unit's LDS words rewritten between them"""
    pat = needle(8)
    blocks = []
    for i in range(330):
        L = (37 * i * i + 11 * i + 9) % (TILE - 1) + 1
        b = text[(i % 90) * TILE + 5 * i:][:L].copy()
        if i % 9 == 0 and L >= 8:
            plant(b, pat, [(i * 977) % (L - 7)])
        blocks.append(b)
        if i % 40 == 0:
            big = text[(i % 50) * TILE:][:12 * TILE + 100 * i + 1].copy()
            plant(big, pat, [5 * TILE + (i // 40 % 4) * SPAN + 9, big.size - 8])
            blocks.append(big)
    blocks.append(quiet(text, 200, 5))
    tiles = sum((b.size + TILE - 1) // TILE for b in blocks)
    assert tiles > 2 * 256 + 60
    return blocks, pat, 0


def decoy(text):
    """every gram of the needle in ONE span, never the needle: its head and its tail next to one another"""
    pat = needle(8)
    a = text[:30 * TILE + 9].copy()
    for t, s in ((3, 0), (9, 2), (14, 3)):
        plant(a, pat[:6], [t * TILE + s * SPAN + 500])
        plant(a, pat[2:], [t * TILE + s * SPAN + 700])
    return [a, quiet(text, 100, 7)], pat, 0


BINDINGS = {
    "borders4": lambda t: borders(t, 4), "borders8": lambda t: borders(t, 8), "borders28": lambda t: borders(t, 28),
    "borders32": lambda t: borders(t, 32), "borders40": lambda t: borders(t, 40),
    "span_patterns": span_patterns,
    "chunk_ends4": lambda t: chunk_ends(t, 4), "chunk_ends8": lambda t: chunk_ends(t, 8), "chunk_ends32": lambda t: chunk_ends(t, 32),
    "tiny_chunks": tiny_chunks, "decoy": decoy,
}


# ---- fixtures and checks ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text():
    return make_text()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return spm.load(tmp_path_factory.mktemp("gate_spans_model"))


@pytest.fixture
def sk():
    saved = {k: os.environ.pop(k, None) for k in ("XSG_SKETCH", "XSG_GATE_GRID", "XSG_GATE_SPANS")}
    os.environ["XSG_SKETCH"] = "1"  # a synchronous call builds the sketch before its first eligible pass
    s = Sketched()
    s.status = s.torch.zeros(1, dtype=s.torch.int64, device="cuda:0")
    yield s
    s.close()
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def oracle_wanted(oracle, blocks, pat, flags):
    oracle.set_exact(bool(flags & xsg.FLAG_EXACT_TAIL))
    try:
        return wanted(oracle, blocks, pat)
    finally:
        oracle.set_exact(False)


def run_binding(sk, oracle, blocks, pat, flags, where, name=SPANS_FIN):
    """bind, build the sketch and the locator, then every count call on the expected form; -> the count"""
    sk.bind(blocks)
    build_with_absent_needle(sk, oracle, blocks)
    if not flags:
        return check(sk, oracle, blocks, pat, where, name)  # ... a list call and every count call again
    n, _ = oracle_wanted(oracle, blocks, pat, flags)
    sk.ctx.set_pattern(pat, flags)
    assert sk.name().endswith(name), (where, sk.name())
    assert async_many(sk) == [n] * 3, (where, "ahead of any verdict")
    every_count_call(sk, n, sum(int(b.size) for b in blocks), where, name)
    return n


@pytest.mark.parametrize("grid", (None, 1), ids=("default_grid", "grid1"))
@pytest.mark.parametrize("plen", (4, 8, 28, 32, 40))
def test_window_starts_at_every_span_border(sk, oracle, text, plen, grid):
    blocks, pat, flags = BINDINGS[f"borders{plen}"](text)
    if grid is not None:
        os.environ["XSG_GATE_GRID"] = str(grid)
    n = run_binding(sk, oracle, blocks, pat, flags, ("borders", plen, grid))
    assert n >= 4 * 4


def test_one_span_each_all_four_and_two_in_one(sk, oracle, model, text):
    blocks, pat, flags = span_patterns(text)
    sp = spm.build(model, blocks[0])
    masks = [spm.mask(model, sp, t, pat) for t in (2, 5, 8, 11, 20, 26, 30)]
    # what the locator says of those tiles (a superset of): one span each, all four, span 2, span 1 (the window's start)
    assert [m & w for m, w in zip(masks, (1, 2, 4, 8, 15, 4, 2))] == [1, 2, 4, 8, 15, 4, 2]
    assert masks[:4] == [1, 2, 4, 8] and masks[5] == 4  # on this text the locator is exact there: three waves read nothing
    assert run_binding(sk, oracle, blocks, pat, flags, "span patterns") == 11


@pytest.mark.parametrize("plen", (4, 8, 32))
def test_chunks_that_end_inside_every_span(sk, oracle, text, plen):
    """a zone's occurrence is counted once, by the walk, whether or not its span passes; the zone look does not depend on
    any span of the tile"""
    blocks, pat, flags = chunk_ends(text, plen)
    n = run_binding(sk, oracle, blocks, pat, flags, ("chunk ends", plen))
    assert n >= len(blocks)
    os.environ["XSG_GATE_GRID"] = "1"
    sk.ctx.set_pattern(pat)
    every_count_call(sk, n, sum(int(b.size) for b in blocks), ("chunk ends", plen, "grid 1"), SPANS_FIN)


@pytest.mark.parametrize("grid", (1, 3))
def test_many_tiny_chunks_under_small_grids(sk, oracle, text, grid):
    blocks, pat, flags = tiny_chunks(text)
    os.environ["XSG_GATE_GRID"] = str(grid)
    assert run_binding(sk, oracle, blocks, pat, flags, ("tiny chunks", grid)) >= 40


def test_a_decoy_span_is_read_and_counts_nothing(sk, oracle, model, text):
    blocks, pat, flags = decoy(text)
    sp = spm.build(model, blocks[0])
    for t, s in ((3, 0), (9, 2), (14, 3)):
        assert spm.mask(model, sp, t, pat) == 1 << s  # the locator lets exactly the decoy's span through
    assert run_binding(sk, oracle, blocks, pat, flags, "decoy") == 0


def test_the_switch_keeps_whole_tile_reads_in_the_same_build(sk, oracle, text):
    """XSG_GATE_SPANS=0 (re-read at every use under the test hooks) takes the locator out of the name and of the pass"""
    blocks, pat, flags = span_patterns(text)
    n = run_binding(sk, oracle, blocks, pat, flags, "spans on")
    os.environ["XSG_GATE_SPANS"] = "0"
    assert sk.name().endswith(FIN) and "spans" not in sk.name()
    every_count_call(sk, n, sum(int(b.size) for b in blocks), "spans off", FIN)
    os.environ.pop("XSG_GATE_SPANS")
    every_count_call(sk, n, sum(int(b.size) for b in blocks), "spans on again", SPANS_FIN)
    # the storing form (a count with newline totals, a list) never names the locator
    assert "spans" not in sk.name(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES) and "spans" not in sk.name(xsg.MATCH_BYTE_OFFSETS)


# ---- the same bindings with whole-tile reads, in a fresh process ----------------------------------------------------------
def child_main():
    """every binding under the environment it was started with: {name: [kernel name, count, async counts, status counters]}"""
    text = make_text()
    os.environ["XSG_SKETCH"] = "1"
    out = {}
    for key, make in BINDINGS.items():
        blocks, pat, flags = make(text)
        s = Sketched()
        s.status = s.torch.zeros(1, dtype=s.torch.int64, device="cuda:0")
        s.bind(blocks)
        s.ctx.set_pattern(pat, flags)
        first = s.count()  # builds the sketch (XSG_SKETCH=1) and reaches the verdict
        out[key] = [s.name(), first, async_many(s), count_with_status(s)[0], s.count_begin_end()]
        s.close()
    print("CHILD " + json.dumps(out))


def test_whole_tile_reads_in_a_fresh_process_give_the_same_numbers(oracle, text):
    env = {k: v for k, v in os.environ.items() if k not in ("XSG_TEST_HOOKS", "XSG_GATE_GRID", "XSG_SKETCH")}
    env.update(XSG_GATE_SPANS="0", XSG_SKETCH_MIN_BYTES="0", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_gate_spans as t; t.child_main()"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
    assert sorted(got) == sorted(BINDINGS)
    for key, make in BINDINGS.items():
        blocks, pat, flags = make(text)
        n, _ = oracle_wanted(oracle, blocks, pat, flags)
        nbytes = sum(int(b.size) for b in blocks)
        name, first, many, status, begin_end = got[key]
        assert name.endswith(FIN) and "spans" not in name, (key, name)
        assert (first, many, status, begin_end) == (n, [n] * 3, [n, 0, 0, nbytes], n), key
