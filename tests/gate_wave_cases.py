"""The dealing of the wave form of the finishing gated count (x-search_amd/csrc/xsg_kernels.hip: gated_pass_waves), restated
in Python, and the bindings that tests/test_gpu_gate_waves.py runs on it.

A sketch group is 64 consecutive tiles of the binding (lane l <-> tile g * 64 + l).  Wave w of workgroup b takes the groups
b * 4 + w, then adds grid * 4 each round; the grid is min(ceil(ntiles / 256), XSG_GATE_GRID or 8192).  tests/
test_gate_wave_cases.py proves without a GPU that every binding below reaches the edge it is named after.

Every binding is a function of one text (make_text) alone: name -> (blocks, pattern, flags).
"""
import numpy as np

import test_gpu_sketch as base
import xsg
from test_gpu_gate_spans import SPAN, chunk_ends, flags_of, needle, quiet, span_patterns
from test_gpu_sketch import TILE
from test_gpu_sketch_select import plant

GROUP = 64
WAVES = 4
UNIT = GROUP * WAVES
DEFAULT_GRID = 8192
TEXT_TILES = 700
WAVE_TAG = " a wave per group"


def make_text():
    rng = np.random.Generator(np.random.PCG64(6400))
    t = base._text(rng, TEXT_TILES * TILE)
    t.setflags(write=False)
    return t


# ---- the dealing -----------------------------------------------------------------------------------------------------------
def grid_of(ntiles, grid=None):
    return min(max((ntiles + UNIT - 1) // UNIT, 1), grid or DEFAULT_GRID)


def ngroups(ntiles):
    return (ntiles + GROUP - 1) // GROUP


def deal(ntiles, grid=None):
    """-> [(workgroup, wave, round)] of every group of a binding of `ntiles` tiles"""
    stride = grid_of(ntiles, grid) * WAVES
    return [(g % stride // WAVES, g % stride % WAVES, g // stride) for g in range(ngroups(ntiles))]


def owner(ntiles, tile, grid=None):
    """-> (workgroup, wave, round) of the wave that tests and scans `tile`"""
    return deal(ntiles, grid)[tile // GROUP]


def tiles_of(blocks):
    return [(int(b.size) + TILE - 1) // TILE for b in blocks]


def tile0_of(blocks):
    """the binding's first tile of every chunk (tiles never span chunks)"""
    out = [0]
    for n in tiles_of(blocks):
        out.append(out[-1] + n)
    return out


# ---- the bindings ----------------------------------------------------------------------------------------------------------
GROUP_EDGE_TILES = (63, 64, 65, 127, 128, 129, 255, 256, 257)


def edge_spots(ntiles):
    """the first and the last tile of every group, and the last tile of the binding"""
    t = {g * GROUP for g in range(ngroups(ntiles))} | {min(g * GROUP + GROUP - 1, ntiles - 1) for g in range(ngroups(ntiles))}
    return sorted(t | {ntiles - 1})


def group_edges(text, ntiles, chunked):
    """`ntiles` tiles with the needle in the first and the last tile of every group; one chunk, or chunks of 1, 2, 3, ...
    tiles so that tile_chunk is in play.  The quiet filler is a binding of its own kind: the tile count IS the case, so
    the needle sits in few enough tiles (at most 2 per 64 + 1) for the verdict."""
    pat = needle(8)
    whole = text[:ntiles * TILE - 5].copy()
    plant(whole, pat, [t * TILE + (t % 4) * SPAN + 100 + t for t in edge_spots(ntiles)])
    if not chunked:
        return [whole], pat, 0
    blocks, t, k = [], 0, 1
    while t < ntiles:
        n = min(k, ntiles - t)
        blocks.append(whole[t * TILE:(t + n) * TILE - (3 if t + n < ntiles else 0)].copy())
        t, k = t + n, k % 7 + 1
    return blocks, pat, 0


MANY_GROUPS_CHUNKS = (600, 600, 430)  # tiles: 26 groups -- 6 or 7 a wave under grid 1 (4 waves), 2 or 3 under grid 3 (12 waves)
MANY_GROUPS_TILES = sum(MANY_GROUPS_CHUNKS)


def many_groups(text):
    """26 groups in three chunks, a needle in two tiles of each group: every wave of a small grid takes several groups,
    and in the last round some waves have none while others scan"""
    pat = needle(8)
    big = np.concatenate([text[20 * i * TILE:][:n * TILE] for i, n in enumerate(MANY_GROUPS_CHUNKS)])
    spots = []
    for g in range(ngroups(MANY_GROUPS_TILES)):
        for l in (g % 20, 25 + g % 4):
            t = g * GROUP + l
            if t < MANY_GROUPS_TILES:
                spots.append(t * TILE + (g % 4) * SPAN + 17 * g + l)
    plant(big, pat, spots)
    blocks, t = [], 0
    for n in MANY_GROUPS_CHUNKS:
        blocks.append(big[t * TILE:(t + n) * TILE - 9].copy())
        t += n
    return blocks, pat, 0


def busy_waves(text, busy):
    """under XSG_GATE_GRID=1: groups 0 .. 3 are the first round of waves 0 .. 3.  The groups of the `busy` waves hold the
    needle in all four spans of all 64 tiles (256 pairs for one wave); the other waves' groups hold none.  Quiet filler
    behind them keeps the share of passing tiles under the verdict's quarter."""
    pat = needle(8)
    a = text[:UNIT * TILE].copy()
    spots = [(w * GROUP + l) * TILE + s * SPAN + 200 + 3 * l + s for w in busy for l in range(GROUP) for s in range(4)]
    plant(a, pat, spots)
    fill = 5 * GROUP * len(busy)
    blocks = [a]
    while fill > 0:  # (the text is 700 tiles long: the filler comes in pieces)
        n = min(fill, TEXT_TILES - 60)
        blocks.append(quiet(text, n, len(blocks)))
        fill -= n
    return blocks, pat, 0


def long_staged(text, plen):
    """kLong under XSG_GATE_GRID=1: occurrences only in groups owned by waves 1, 2 and 3, and beside each a decoy -- the
    needle with every byte outside one 8-byte window altered, for every window the filter can sit on: a wave that
    verifies against an unstaged s_pat counts wrong"""
    pat = needle(plen)
    a = text[:(UNIT + 6 * GROUP) * TILE + 77].copy()
    spots, k = [], 0
    for g in (1, 2, 3, 5, 6, 7):  # waves 1, 2, 3 in rounds 0 and 1
        for l in (0, 31, 63):
            at = (g * GROUP + l) * TILE + (k % 4) * SPAN + 300 + 7 * k
            spots.append(at)
            for j, koff in enumerate(range(0, plen - 7)):
                d = bytearray(b"~" * plen)
                d[koff:koff + 8] = pat[koff:koff + 8]
                plant(a, bytes(d), [at + 600 + 64 * j])
            k += 1
    plant(a, pat, spots)
    return [a], pat, flags_of(plen)


def zone_pairs(text, plen):
    """chunks that end in tiles owned by waves 1, 2 and 3 of XSG_GATE_GRID=1, in pairs whose last tiles lie 64 tiles apart
    -- two waves of one workgroup look at their zones in the same round, each in its own row of s_zone -- with the needle
    in the zone only, ahead of the zone only, and in both (the chunk_ends recipe)"""
    pat = needle(plen)
    blocks, salt = [], 0

    def chunk(ntiles, r, spots_of):
        nonlocal salt
        L = (ntiles - 1) * TILE + r
        b = text[(salt * 13 % 40) * TILE + 7 * salt:][:L].copy()
        salt += 1
        plant(b, pat, spots_of(L, L - plen - 31))
        blocks.append(b)

    recipes = (lambda L, Z: [L - plen], lambda L, Z: [Z - 2 * plen - 3], lambda L, Z: [Z - 2 * plen - 3, L - plen])
    # last tiles at 64 + 9, 128 + 9 | 128 + 40, 192 + 40 | 256 + 64 + 20, 256 + 128 + 20: waves (1, 2), (2, 3), (1, 2) round 1
    for i, (ends, r) in enumerate((((73, 137), SPAN + 1), ((168, 232), 2 * SPAN + plen + 31), ((340, 404), TILE - 1))):
        t = tile0_of(blocks)[-1]
        for e in ends:
            chunk(e + 1 - t, r, recipes[i])
            t = e + 1
    blocks.append(quiet(text, 4 * 64, plen))
    return blocks, pat, 0


BINDINGS = {f"edges{n}{'c' if c else ''}": (lambda t, n=n, c=c: group_edges(t, n, c)) for n in GROUP_EDGE_TILES for c in (False, True)}
BINDINGS.update({
    "many_groups": many_groups,
    "one_busy_wave": lambda t: busy_waves(t, (2,)), "three_busy_waves": lambda t: busy_waves(t, (0, 1, 3)),
    "long28": lambda t: long_staged(t, 28), "long32": lambda t: long_staged(t, 32), "long40": lambda t: long_staged(t, 40),
    "zones4": lambda t: zone_pairs(t, 4), "zones8": lambda t: zone_pairs(t, 8), "zones32": lambda t: zone_pairs(t, 32),
    "span_patterns": span_patterns,
})
assert chunk_ends and xsg  # (the recipes this module restates and the flags it returns)
