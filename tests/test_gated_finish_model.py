"""CPU model of the finishing form of the gated count pass (x-search_amd/csrc/xsg_kernels.hip: gated_pass<..., FIN>),
built from the product's own headers (tests/cpu_model/gated_finish_model.cpp), against the oracle.  No GPU needed.

(a) The end-of-chunk walk reports nothing unless the needle occurs in full inside the zone, whatever its entry; where the
    zone holds an occurrence the entry matters.
(b) The entry found by walking a chunk's tiles backwards and searching only the tiles whose sketch passes, fed to
    tail_walk in the one tile that owns the zone, gives the oracle's count of the chunk -- also for long needles counted
    at a filter window (koff > 0) whose start and window lie in different tiles.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "cpu_model" / "gated_finish_model.cpp"
LIB = HERE / "cpu_model" / "build" / "libgated_finish_model.so"
CSRC = HERE.parent / "x-search_amd" / "csrc"
TILE = 16384


@pytest.fixture(scope="module")
def gf():
    LIB.parent.mkdir(exist_ok=True)
    deps = [SRC, CSRC / "xsg_tail.h", CSRC / "xsg_sketch.h"]
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", str(LIB), str(SRC)])
    lib = C.CDLL(str(LIB))
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    u64p = C.POINTER(u64)
    lib.gf_check_zero_walk.argtypes = [u64, u64, u32, u64p, u64p]
    lib.gf_check_zero_walk.restype = u64
    lib.gf_count.argtypes = [vp, u64, C.c_char_p, u32, u32, u64p, u64p, u64p]
    lib.gf_count.restype = u64
    lib.gf_tail_walk.argtypes = [vp, u64, C.c_char_p, u32, u64]
    lib.gf_tail_walk.restype = u32
    lib.gf_zone_begin.argtypes = [u64, u32]
    lib.gf_zone_begin.restype = u64
    return lib


def bordered(p: bytes) -> bool:
    return any(p[:k] == p[-k:] for k in range(1, len(p)))


def model_count(gf, data, pat, koff):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    entry, searched, walks = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    n = gf.gf_count(data.ctypes.data, data.size, pat, len(pat), koff, C.byref(entry), C.byref(searched), C.byref(walks))
    assert walks.value <= 1  # a zone is walked once, however many tiles look at it
    return int(n), (None if entry.value == 2**64 - 1 else int(entry.value)), int(searched.value)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", (0, 1), ids=("abc_nl_space", "ab_nl"))
def test_a_zone_without_an_occurrence_counts_nothing_from_any_entry(gf, alphabet):
    dep, cases = C.c_uint64(0), C.c_uint64(0)
    assert gf.gf_check_zero_walk(7 + alphabet, 60000, alphabet, C.byref(dep), C.byref(cases)) == 0
    assert cases.value > 2_000_000
    assert dep.value > 100  # the entry cannot be dropped: with an occurrence in the zone the count depends on it


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def _text(rng, n):
    words = [b"that", b"with", b"have", b"this", b"from", b"they", b"which", b"would", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


def _plant(b, pat, offs):
    for o in offs:
        b[o:o + len(pat)] = np.frombuffer(pat, dtype=np.uint8)


LENGTHS = (1, 7, 8, 38, 39, 40, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 2 * TILE + 7, 2 * TILE + 8, 2 * TILE + 23, 2 * TILE + 39,
           5 * TILE + 20)


@pytest.mark.parametrize("pat,koff", ((b"SHER", 0), (b"SHERL", 0), (b"SHERLOCK", 0), (b"SHERLOCKX", 0), (b"SHERLOCKX", 1),
                                      (b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456", 25), (b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456", 0)))
def test_the_pass_on_one_chunk_gives_the_oracles_count(gf, oracle, pat, koff):
    assert not bordered(pat)
    plen = len(pat)
    rng = np.random.default_rng(4100 + plen + koff)
    seen_walk = seen_lookback = 0
    for L in LENGTHS:
        for trial in range(6):
            b = _text(rng, L)
            if L >= plen:
                spots = {int(rng.integers(0, L - plen + 1)) for _ in range(int(rng.integers(0, 4)))}
                if trial & 1:
                    spots.add(L - plen - int(rng.integers(0, min(L - plen, plen + 30) + 1)))  # in the zone
                if trial & 2 and L > TILE:
                    spots.add(TILE - koff - 1)       # starts in tile 0, its window in tile 0's last byte ...
                    spots.add(2 * TILE - koff if 2 * TILE - koff + plen <= L else 0)  # ... / in the first byte of tile 2
                spots = {s for s in spots if 0 <= s <= L - plen}
                _plant(b, pat, sorted(s for s in spots if not any(abs(s - o) < plen and s != o for o in spots)))
            want = oracle.count(b, pat, False)
            got, entry, searched = model_count(gf, b, pat, koff)
            assert got == want, (L, trial, pat, koff, entry, searched)
            seen_walk += entry is not None
            seen_lookback += bool(entry)
    assert seen_walk >= 10 and seen_lookback >= 5


def test_entry_dependence_through_the_look_back(gf, oracle):
    """`SSHERLOCK`-shaped zones: the lossy scalar part skips the needle behind a partial prefix for some entries only.  The
    last occurrence before Z sits at each of 32 consecutive positions, in the zone's own tile, one tile back, several
    tiles back with passing-but-empty tiles in between, or nowhere."""
    pat = b"SHERLOCK"
    plen = len(pat)
    rng = np.random.default_rng(4200)
    tails = set()
    for L in (3 * TILE + 17, 3 * TILE + plen + 15, 6 * TILE + 5):
        Z = int(gf.gf_zone_begin(L, plen))
        for where in ("zone_tile", "previous_tile", "far", "nowhere"):
            for shift in range(32):
                b = _text(rng, L)
                _plant(b, b"S" + pat, (L - plen - 1 - 3,))          # needle behind a partial prefix, in the zone
                _plant(b, b"SHERL", (TILE + 100,))                  # grams of the needle, apart: tile 1 passes, holds nothing
                _plant(b, b"ERLOCK", (TILE + 300,))
                if where == "zone_tile" and (Z - 1) // TILE * TILE + plen + 40 < Z:
                    _plant(b, pat, (Z - plen - shift,))
                elif where == "previous_tile":
                    _plant(b, pat, ((Z - 1) // TILE * TILE - 2 * plen - shift,))
                elif where == "far":
                    _plant(b, pat, (500 + shift,))
                want = oracle.count(b, pat, False)
                got, entry, searched = model_count(gf, b, pat, 0)
                assert got == want, (L, where, shift)
                assert entry is not None
                tails.add(gf.gf_tail_walk(b.ctypes.data, b.size, pat, plen, entry))
                if where == "far":
                    assert searched >= 2  # the passing-but-empty tile was searched on the way back
    assert len(tails) >= 2  # the cases do produce different tail counts for different entries
