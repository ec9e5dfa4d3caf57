"""The run arithmetic of k_count_chunks (x-search_amd/csrc/xsg_chunkcount.h), driven on the CPU through a model built from
the product's own header (tests/cpu_model/chunk_runs_model.cpp).  No GPU needed.

A wave holds 64 consecutive tiles; from the mask of lanes whose chunk id differs from their left neighbour's the header
derives the run heads and the lane range each head owns.  Every mask below is checked against a naive loop over the lanes,
for a full wave and for last waves that hold fewer than 64 tiles: same heads, same ends, and the owned ranges cover every
active lane exactly once and no other lane.
"""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "cpu_model" / "chunk_runs_model.cpp"
LIB = HERE / "cpu_model" / "build" / "libchunk_runs_model.so"
HDR = HERE.parent / "x-search_amd" / "csrc" / "xsg_chunkcount.h"
FULL = (1 << 64) - 1
LANE_COUNTS = (64, 63, 62, 33, 32, 2, 1)  # a full wave, and last waves with fewer valid tiles


@pytest.fixture(scope="module")
def cr():
    LIB.parent.mkdir(exist_ok=True)
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", str(LIB), str(SRC)])
    lib = C.CDLL(str(LIB))
    u64, u32 = C.c_uint64, C.c_uint32
    lib.cr_check.argtypes = [u64, u32]
    lib.cr_check.restype = C.c_int
    lib.cr_check_many.argtypes = [C.c_void_p, u64, C.c_void_p, u32, C.POINTER(u64), C.POINTER(u32), C.POINTER(C.c_int)]
    lib.cr_check_many.restype = u64
    lib.cr_check_sums.argtypes = [C.c_void_p, C.c_void_p, u32, u32]
    lib.cr_check_sums.restype = C.c_int
    return lib


def check_masks(cr, masks, lane_counts=LANE_COUNTS):
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    ns = np.ascontiguousarray(lane_counts, dtype=np.uint32)
    bad_mask, bad_n, bad_code = C.c_uint64(0), C.c_uint32(0), C.c_int(0)
    bad = cr.cr_check_many(m.ctypes.data, m.size, ns.ctypes.data, ns.size, C.byref(bad_mask), C.byref(bad_n), C.byref(bad_code))
    assert bad == 0, (hex(bad_mask.value), bad_n.value, bad_code.value)


def test_the_empty_and_the_full_mask(cr):
    check_masks(cr, [0, FULL], lane_counts=range(1, 65))


def test_all_single_bit_masks(cr):
    check_masks(cr, [1 << i for i in range(64)], lane_counts=range(1, 65))


def test_all_two_bit_masks(cr):
    check_masks(cr, [(1 << a) | (1 << b) for a, b in itertools.combinations(range(64), 2)], lane_counts=range(1, 65))


def test_masks_with_bits_at_the_edge_lanes(cr):
    edge = (0, 1, 62, 63)
    masks = []
    for k in range(1, 5):
        for lanes in itertools.combinations(edge, k):
            e = sum(1 << i for i in lanes)
            masks += [e, e | (1 << 31), e | (1 << 32), e | (FULL & ~((1 << 0) | (1 << 1) | (1 << 62) | (1 << 63)))]
    check_masks(cr, masks, lane_counts=range(1, 65))


def test_random_masks(cr):
    rng = np.random.default_rng(5300)
    dense = rng.integers(0, 1 << 63, size=50_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=50_000, dtype=np.uint64)
    sparse = dense[:25_000] & dense[25_000:] & rng.integers(0, 1 << 63, size=25_000, dtype=np.uint64)  # few boundaries
    check_masks(cr, np.concatenate([dense, sparse, sparse | np.uint64(1 << 63), ~sparse]))


def test_lane_0_and_lanes_without_a_tile(cr):
    # lane 0 is a head whether or not its change bit is set; bits of lanes without a tile do not count
    assert cr.cr_check(0, 64) == 0
    assert cr.cr_check(1, 64) == 0
    assert cr.cr_check(FULL, 1) == 0
    assert cr.cr_check(1 << 63, 63) == 0


def test_run_sums_by_prefix_differences(cr):
    """the kernel's sum per run -- inclusive prefix at the run's last lane minus the prefix in front of its head -- equals
    a plain sum per chunk, for the cuts of the GPU test (chunks of [1, 62, 1, 1, 63, 64, 2] tiles) and random ones"""
    rng = np.random.default_rng(5301)
    sizes = [1, 62, 1, 1, 63, 64, 2]
    tile_chunk = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    for start in range(0, tile_chunk.size, 64):
        ids = np.ascontiguousarray(tile_chunk[start:start + 64])
        vals = rng.integers(0, 16385, size=ids.size, dtype=np.uint32)  # a tile holds at most 16384 matches
        assert cr.cr_check_sums(ids.ctypes.data, vals.ctypes.data, ids.size, len(sizes)) == 0, start
    for _ in range(2000):
        n = int(rng.integers(1, 65))
        ids = np.cumsum(rng.integers(0, 3, size=n) * (rng.random(n) < 0.2)).astype(np.uint32)  # ascending, gaps allowed
        vals = (rng.integers(0, 16385, size=n) * (rng.random(n) < 0.5)).astype(np.uint32)
        assert cr.cr_check_sums(ids.ctypes.data, vals.ctypes.data, n, int(ids[-1]) + 1) == 0
