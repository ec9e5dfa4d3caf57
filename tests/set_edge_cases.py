"""Cases of the literal-list route at five edges that tests/set_cases.py does not reach (plain Python, no GPU):
tests/test_set_edge_cases.py proves without a GPU that every case meets the condition it was built for,
tests/test_gpu_set_edges.py searches them on the device.

  A  grid_case        more than 2 * grid tiles from tiny chunks: every workgroup of k_set_scan's bounded grid loops
  B  walk_periodic,   more than 524 288 + 2048 candidates in one chunk: k_rx_block_max_scan's second iteration, and covers
     walk_long_cover  across the item, wave, block and scan-iteration boundaries of k_rx_heads
  C  fold_case        every byte value at every gram position, at every byte of a lane's w[0..4], under ignore-case
  D  collision_case,  grams that share a filter bit with a literal's gram without being it; the list's limits
     limit_*
  E  nul_*            literals of NUL bytes against the zeros the scan substitutes behind a chunk's end

Expected values are set_cases.expected's (the oracle's regex reader on E(S), tests/set_model.py where it refuses)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import set_cases as SC
import xsg
from set_cases import TILE, u8

# ---- A. the bounded grid of k_set_scan -----------------------------------------------------------------------------------------
GRID_PER_CU = 8  # kSetGridPerCu of x-search_amd/csrc/xsg_set_kernels.hip; set_grid launches min(ntiles, 8 * CUs) workgroups
GRID_LITS = SC.END_LITS[4]  # (b"kqzw", b"needle"): g = 4
_FILLER = SC._LINE * 3  # (holds no byte of `kqzw` and no `need`)

GridCase = namedtuple("GridCase", "blocks lack")  # lack[c]: what chunk c's last bytes need to become an occurrence, or b""


def grid_hit(tile: int, grid: int) -> bool:
    """whether tile `tile` holds an occurrence: workgroup b of a grid of `grid` sees hit, no hit, hit on the tiles b,
    b + grid, b + 2 * grid when b is even and no hit, hit, no hit when b is odd"""
    return (tile // grid + tile % grid) % 2 == 0


def _paint(buf: bytearray, lo: int, room: int, tile: int, hit: bool):
    """the bytes [lo, lo + room) of a chunk are tile number `tile`"""
    if hit:
        assert room >= 4
        if room >= 12:
            at = (tile * 7919) % (room - 5)
            buf[lo + at:lo + at + 6] = b"needle"
            if room >= 30:  # one more that only ignore-case finds
                up = at + 10 if at + 16 <= room else at - 10
                buf[lo + up:lo + up + 6] = b"NEEdle" if tile & 1 else b"KqZW k"
        else:
            at = tile % (room - 3)
            buf[lo + at:lo + at + 4] = b"kqzw"
    elif room >= 8 and tile % 3 == 0:  # a candidate that is no occurrence: the gram of `needle` without its rest
        at = tile % (room - 4)
        buf[lo + at:lo + at + 5] = b"needs"
    elif room >= 8 and tile % 3 == 1:  # `need` as the last bytes: `le` is what the chunk lacks (grid_fill puts it there)
        buf[lo + room - 4:lo + room] = b"need"


@lru_cache(maxsize=None)
def grid_case(grid: int) -> GridCase:
    """2 * grid + grid // 2 + 40 tiles and more: chunks of 1..40 bytes, one tile each, and every grid // 3 + 7 tiles a
    chunk of 16 KiB + 1..17 bytes, two tiles; the first of those tiles ends inside an occurrence"""
    rng = np.random.Generator(np.random.PCG64(4242 + grid))
    want_tiles = 2 * grid + grid // 2 + 40
    blocks, lack, tile, big = [], [], 0, 0
    next_big = grid // 3 + 7
    while tile < want_tiles:
        k = big % 17 + 1
        if tile >= next_big and (k >= 4 or not grid_hit(tile + 1, grid)):
            buf = bytearray((_FILLER * (TILE // len(_FILLER) + 2))[tile % 31:][:TILE + k])
            _paint(buf, 0, TILE, tile, grid_hit(tile, grid))
            cut = b""
            if grid_hit(tile, grid) and not grid_hit(tile + 1, grid):
                buf[TILE - 3:TILE + k] = (b"needle" + b" " * 17)[:3 + k]  # starts in the first tile, goes on (or is cut) in the second
                cut = b"needle"[3 + k:]
            if grid_hit(tile + 1, grid):
                _paint(buf, TILE, k, tile + 1, True)
            blocks.append(u8(buf))
            lack.append(cut)
            tile += 2
            big += 1
            next_big = tile + grid // 3 + 7
            continue
        hit = grid_hit(tile, grid)
        n = int(rng.integers(1, 41))
        if hit and n < 8:
            n += 8
        buf = bytearray(_FILLER[tile % 29:][:n])
        _paint(buf, 0, n, tile, hit)
        blocks.append(u8(buf))
        lack.append(b"le" if bytes(buf).endswith(b"need") else b"")
        tile += 1
    return GridCase(tuple(blocks), tuple(lack))


def grid_fill(case: GridCase):
    """set_cases.end_fill(4)'s stale matches in every pad and guard, behind what the chunk in front lacks"""
    stale = SC.end_fill(4)

    def fill(i, n):
        head = case.lack[i - 1] if i > 0 else b""
        return u8((head + stale(0, n).tobytes())[:n])
    return fill


def grid_conditions(case: GridCase, grid: int, hit):
    """what the case was built for, given hit[t] = tile t holds a match (from the expected result): more than 2 * grid
    tiles; a match in a tile is a function of the tile number; for a quarter of the workgroups b and more the tiles b,
    b + grid, b + 2 * grid alternate, in both orders; consecutive tiles of a workgroup lie in different chunks"""
    tiles = tiles_of(case.blocks)
    assert len(tiles) == len(hit) == sum(-(-int(b.size) // TILE) for b in case.blocks) >= 2 * grid + grid // 2 > 2 * grid
    assert list(hit) == [grid_hit(t, grid) for t in range(len(tiles))]
    three = [(hit[b], hit[b + grid], hit[b + 2 * grid]) for b in range(grid) if b + 2 * grid < len(tiles)]
    assert three.count((True, False, True)) >= grid // 8 and three.count((False, True, False)) >= grid // 8
    assert three.count((True, False, True)) + three.count((False, True, False)) >= grid // 4
    assert all(tiles[b][0] != tiles[b + grid][0] for b in range(len(tiles) - grid))


def tiles_of(blocks):
    """-> [(chunk, offset of the tile in the chunk)] in tile order, as xsg_shard lays them out (ceil(len / 16 KiB) per chunk)"""
    return [(c, o) for c, b in enumerate(blocks) for o in range(0, int(b.size), TILE)]


# ---- B. the walk over more than 2^19 candidates ---------------------------------------------------------------------------------
WALK_ITEMS, WALK_WAVE, WALK_BLOCK = 8, 512, 2048  # x-search_amd/csrc/xsg_rx_kernels.hip: kRxScanItems, 64 lanes of them, kRxScanBlock
WALK_SCAN = 256 * WALK_BLOCK  # k_rx_block_max_scan takes 256 blocks per iteration: 524 288 candidates
PERIODIC_LITS = (b"abc", b"bcd", b"de")
PERIODIC_PREFIX = b"de "  # one candidate: number 524 288 then is a `bcd`
COVER_X = b"a" + b"ab" * 127
COVER_LITS = (COVER_X, b"a")
COVER_AT = (8 * 1000 + 7, 512 * 40 + 511, 2048 * 30 + 2047, WALK_SCAN - 1)  # the candidate numbers at which X starts


@lru_cache(maxsize=None)
def walk_periodic():
    """units of `abcde `: `abc` a head, `bcd` covered by it, `de` no head (the running maximum is `bcd`'s end) but kept by
    the chain walk; the second chunk's candidates lie at offsets below the first chunk's last end"""
    units = 180_000
    body = bytearray(b"abcde " * units)
    body[6 * 300 - 1::6 * 300] = b"\n" * len(body[6 * 300 - 1::6 * 300])
    return (u8(PERIODIC_PREFIX + bytes(body)), u8(b"abcde abcde\nbcde abc"))


@lru_cache(maxsize=None)
def walk_long_cover():
    """runs of `a` with a newline every 200 bytes; X = `a` + 127 x `ab` (128 candidates, 255 bytes) starts at the
    candidate numbers COVER_AT, the last candidate of a thread's items, of a wave, of a block and of the first scan
    iteration: what it covers begins in the next one"""
    out, cands, line = bytearray(), 0, 0
    targets = list(COVER_AT)
    while len(out) < 1_150_000:
        if targets and cands == targets[0]:
            out += COVER_X
            cands += 128
            line += 255
            targets.pop(0)
        elif line >= 200:
            out += b"\n"
            line = 0
        else:
            out += b"a"
            cands += 1
            line += 1
    assert not targets
    return (u8(out), u8(b"aaa\n" + COVER_X + b"a\naa"))


def candidates(block, literals, flags=0):
    """the positions of one chunk that k_set_scan reports, from the product's filter image (xsg_literals_info): the
    gram at p has its bit and p + g <= L"""
    d, filt = xsg.literals_info(xsg.literal_list(literals), flags, with_filter=True)
    g = d["gram"]
    t = np.asarray(block, dtype=np.uint8)
    if flags & xsg.FLAG_IGNORE_CASE:
        t = np.where((t >= 65) & (t <= 90), t + 32, t).astype(np.uint8)
    if t.size < g:
        return np.zeros(0, dtype=np.int64)
    n = t.size - g + 1
    v = np.zeros(n, dtype=np.uint64)
    for k in range(g):
        v |= t[k:k + n].astype(np.uint64) << np.uint64(8 * k)
    h = gram_hash(v, g)
    bits = (filt[(h >> np.uint64(5)).astype(np.int64)] >> (h & np.uint64(31)).astype(np.uint32)) & 1
    return np.flatnonzero(bits)


def gram_hash(v, g: int):
    """xsg_set.h: set_gram_hash on an array of grams (uint64 holding 32-bit values)"""
    v = np.asarray(v, dtype=np.uint64)
    return v if g <= 2 else ((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)


# ---- C. the packed fold of the scan against the per-byte fold of the compiler and the verifier -----------------------------------
# byte groups: no group holds a byte together with its false partner (0x40 / 0x60, 0x5B / 0x7B, 0xC1..0xDA / 0xE1..0xFA), and
# the filler bytes of a group's literals and of its text come from outside the group and are no letters
FoldGroup = namedtuple("FoldGroup", "name values filler pad")
FOLD_GROUPS = (
    FoldGroup("00-5f", tuple(b for b in range(0x00, 0x60) if b != 10), b"~|}\x7f", b"\x7f"),
    FoldGroup("60-7f", tuple(range(0x60, 0x80)), b"#$%&", b"!"),
    FoldGroup("80-df", tuple(range(0x80, 0xE0)), b"#$%&", b"!"),
    FoldGroup("e0-ff", tuple(range(0xE0, 0x100)), b"#$%&", b"!"),
)


def false_partner(b: int):
    """the byte a wrong fold would confuse b with: the neighbours of the letters 0x20 apart, and a byte >= 0x80 whose
    low seven bits are a capital letter with the byte 0x20 above it"""
    if b in (0x40, 0x5B) or 0xC1 <= b <= 0xDA:
        return b + 0x20
    if b in (0x60, 0x7B) or 0xE1 <= b <= 0xFA:
        return b - 0x20
    return None


FoldCase = namedtuple("FoldCase", "name g group lits blocks partners")  # partners: the false-partner strings in the text


def fold_literals(g: int, group: FoldGroup):
    """for every byte b of the group: b at gram position 0 .. g - 1 (g bytes: the filler with b in it), and b behind the gram"""
    f = group.filler[:g]
    out = []
    for b in group.values:
        for j in range(g):
            out.append((f[:j] + bytes([b]) + f[j + 1:], j))
        out.append((f + bytes([b]), g))
    return out


@lru_cache(maxsize=None)
def fold_case(g: int, gi: int) -> FoldCase:
    """the text holds every literal verbatim, with its ASCII letters' case swapped, and with b replaced by its false
    partner, each starting at every offset 0..15 of a lane's unit (so b visits bytes 0..18 of w[0..4] and the strings
    cross the unit's edge)"""
    group = FOLD_GROUPS[gi]
    lits = fold_literals(g, group)
    strings, partners = [], []
    for lit, j in lits:
        strings.append(lit)
        if lit.swapcase() != lit:
            strings.append(lit.swapcase())
        p = false_partner(lit[j])
        if p is not None:
            partners.append(lit[:j] + bytes([p]) + lit[j + 1:])
    out, since_nl = bytearray(), 0
    for s in strings + partners:
        for off in range(16):
            gap = (off - len(out)) % 16 or 16
            if since_nl > 120:
                out += b"\n" + group.pad * (gap - 1)
                since_nl = 0
            else:
                out += group.pad * gap
            assert len(out) % 16 == off
            out += s
            since_nl += gap + len(s)
    out += group.pad + b"\n"
    cut = (len(out) // 2) & ~15 | 7  # two chunks, the cut at an odd place
    return FoldCase("g%d-%s" % (g, group.name), g, group, tuple(l for l, _ in lits), (u8(out[:cut]), u8(out[cut:])), tuple(partners))


FOLD_CASES = [(g, gi) for g in (1, 2, 3, 4) for gi in range(len(FOLD_GROUPS))]
FOLD_PLAIN = [(4, 0), (1, 1), (2, 2), (3, 3)]  # also searched without the flag, where nothing may fold


# ---- D. grams that collide in the hashed filter, and the list's limits -----------------------------------------------------------
PRINTABLE = np.arange(0x21, 0x7F, dtype=np.uint64)


@lru_cache(maxsize=None)
def colliding_grams(g: int):
    """-> {literal gram: [other printable g-grams with the same set_gram_hash]} for SC.END_LITS[g], g = 3 or 4"""
    assert g in (3, 4)
    a = PRINTABLE
    v3 = (a[:, None, None] | (a[None, :, None] << np.uint64(8)) | (a[None, None, :] << np.uint64(16))).ravel()
    grams = {lit[:g]: int(gram_hash(np.array([int.from_bytes(lit[:g], "little")]), g)[0]) for lit in SC.END_LITS[g]}
    out = {k: [] for k in grams}
    for top in ([0] if g == 3 else [int(x) for x in a]):
        v = v3 | np.uint64(top << 24)
        h = gram_hash(v, g)
        for gram, hh in grams.items():
            for x in v[h == np.uint64(hh)]:
                c = int(x).to_bytes(4, "little")[:g]
                if c != gram:
                    out[gram].append(c)
    return out


# the first eight of colliding_grams per literal gram: tests/cpp/set_selftest.cpp verifies the same strings on the host
COLLIDING_PINNED = {
    b"kqz": (b'":P', b"&h%", b"-@T", b"N$M", b"Uer", b"Ye4", b"`kv", b"dk8"),
    b"nee": (b"%\\N", b"0bR", b";:C", b";hV", b"F@G", b"QFK", b"c$~", b"g$@"),
    b"kqzw": (b"/_h!", b":el!", b">e.!", b"Ekp!", b"Ik2!", b"PCa!", b"TC#!", b"[Ie!"),
    b"need": (b"!vp!", b"%v2!", b",|t!", b"0|6!", b"7Te!", b";T'!", b"BZi!", b"FZ+!"),
}


@lru_cache(maxsize=None)
def collision_case(g: int):
    """-> (literals, blocks, the colliding strings in the text).  For every colliding gram c (at most 24 per literal) and
    every literal l of the list: c + l[g:], the string a verifier that trusted the filter would accept whichever
    gram its lookup lands on; they and real occurrences lie at lane and tile edges"""
    lits = SC.END_LITS[g]
    coll = colliding_grams(g)
    fakes = []
    for gram, cs in coll.items():
        for c in cs[:24]:
            fakes += [c + l[g:] for l in lits]
    buf = bytearray((_FILLER * ((2 * TILE + 4096) // len(_FILLER) + 2))[:2 * TILE + 4096])
    edges = [16, 32, 1024, 4096, TILE, TILE + 4096, 2 * TILE]
    for e, s in zip(edges, (fakes[0], lits[0], fakes[1], lits[1], lits[1], fakes[2], fakes[3])):  # across an edge: one byte in front of it
        buf[e - 1:e - 1 + len(s)] = s
    at = 200
    for i, s in enumerate(fakes + list(lits) * 4):
        buf[at + i % 16:at + i % 16 + len(s)] = s
        at += 48
        while any(e - 32 < at < e + 32 for e in edges):
            at += 48
    assert at < len(buf) - 64
    tail = bytearray(_FILLER[:64])
    tail[-len(fakes[0]):] = fakes[0]  # a colliding string as a chunk's last bytes
    return lits, (u8(buf), u8(tail), u8(fakes[1] + b" and " + lits[1])), tuple(fakes)


# the limits: 4096 literals, 32 767 bytes with the separators (XSG_MAX_PATTERN is 32 768)
_A16, _A8 = b"abcdefghijklmnop", b"abcdefgh"
ROOM_SHORT = b"abcdb"  # the room case: the only literal under 7 bytes of LIMIT_SHARED


@lru_cache(maxsize=None)
def limit_shared():
    """4096 literals that all begin with `abcd`: 4096 entries under one key.  4095 of 7 bytes (every tail of three of 16
    letters but one) and `abcdb` (5 bytes) listed late: where only 5 bytes are left of a chunk, the 256 seven-byte
    literals `abcdb??` listed in front of it do not fit and it must be reported"""
    tails = [bytes((_A16[i >> 8], _A16[(i >> 4) & 15], _A16[i & 15])) for i in range(4096)]
    lits = [b"abcd" + t for t in tails]
    lits[3000] = ROOM_SHORT
    assert len(xsg.literal_list(lits)) == 32765 <= xsg.MAX_PATTERN and lits.index(ROOM_SHORT + b"aa") == 256
    return tuple(lits)


@lru_cache(maxsize=None)
def limit_distinct():
    """4096 seven-byte literals with 4096 distinct grams (every 4-gram of 8 letters): the binary search at full depth"""
    rng = np.random.Generator(np.random.PCG64(77))
    lits = []
    for i in range(4096):
        gram = bytes(_A8[(i >> s) & 7] for s in (9, 6, 3, 0))
        lits.append(gram + bytes(_A8[int(x)] for x in rng.integers(0, 8, size=3)))
    assert len(xsg.literal_list(lits)) == 32767 <= xsg.MAX_PATTERN
    return tuple(lits)


LIMIT_LONG = (bytes(_A8[int(x)] for x in np.random.Generator(np.random.PCG64(79)).integers(0, 8, size=255)), b"hhgh")
LIMIT_SMALL = (b"needle", b"abcd")


LimitCase = namedtuple("LimitCase", "blocks lack")


@lru_cache(maxsize=None)
def limit_blocks() -> LimitCase:
    """two chunks of about 64 KiB and one of 24 KB -- letters a..q, letters a..h, letters a..h -- with the first-listed,
    a middle and the last-listed literal of each list planted, some across tile edges; then the room case: a chunk that
    ends in `abcdb` and lacks `aa` (behind its end: `abcdbaa` is listed first of its gram)"""
    rng = np.random.Generator(np.random.PCG64(78))

    def text(alphabet, n):
        t = bytearray(bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n)))
        t[97::131] = b"\n" * len(t[97::131])
        return t

    def plant(t, lits, at):
        for l in lits:
            t[at:at + len(l)] = l
            at += len(l) + 301
    sh, di = limit_shared(), limit_distinct()
    a = text(_A16 + b"q", 65_531)
    plant(a, (sh[0], sh[2047], sh[4095], ROOM_SHORT + b"q", sh[16], b"abcdqaa", LIMIT_SMALL[0]), 1000)
    plant(a, (sh[4095], sh[0], sh[1234]), TILE - 3)
    for i in range(60):  # the shared gram with any three letters behind it
        at = 20_000 + 613 * i
        a[at:at + 4] = b"abcd"
    b = text(_A8, 65_536)
    plant(b, (di[0], di[2047], di[4095], LIMIT_LONG[0], LIMIT_LONG[1]), 777)
    plant(b, (di[4095], LIMIT_LONG[0]), 3 * TILE - 2)
    c = text(_A8, 24_000 + 14)
    plant(c, (LIMIT_LONG[0][:254], LIMIT_LONG[0], di[1], sh[0]), 5000)
    c[-14:] = b"\ngg " + b"needle " + b"abc"  # (cut: the `d` lies behind the end)
    room = text(_A16, 16 * 9) + ROOM_SHORT
    return LimitCase((u8(a), u8(b), u8(c), u8(room), u8(b"aab\nabcdaaa\n")), (b"", b"", b"d", b"aa", b""))


def limit_fill(case):
    def fill(i, n):
        head = case.lack[i - 1] if i > 0 else b""
        return u8((head + b"bcdaaa abcdbaa hhgh\n" * (n // 20 + 1))[:n])
    return fill


LIMIT_LISTS = (("small", lambda: LIMIT_SMALL), ("shared", limit_shared), ("long", lambda: LIMIT_LONG), ("distinct", limit_distinct))


# ---- E. NUL bytes ----------------------------------------------------------------------------------------------------------------
NUL_LISTS = ((b"\0",), (b"\0\0", b"\0"), (b"a\0b", b"\0\0\0\0"))
NUL_RUNS = (1, 2, 15, 16, 17, 16383, 16384, 16385)


@lru_cache(maxsize=None)
def nul_plan():
    """-> ((chunk, ends in text + NULs), ...): chunks of NUL bytes alone; text that ends in one, two and three NULs at
    lengths = 13, 14, 15, 0 (mod 16), a chunk of NULs behind each that has no pad; text with NULs inside it"""
    plan = [(np.zeros(n, dtype=np.uint8), False) for n in NUL_RUNS[:5]]
    for k in (1, 2, 3):
        for r in (13, 14, 15, 16):
            plan.append((SC._ending_in(b"a" + b"\0" * k, 48 + r), True))
        plan.append((np.zeros(NUL_RUNS[4 + k], dtype=np.uint8), False))
    plan.append((u8(b"a\0b a\0\0b\n\0\0\0\0\0 a\0B\n" + b"x" * 30 + b"\0\0\0\0a\0b\0"), False))
    return tuple(plan)


def nul_blocks():
    return [b for b, _ in nul_plan()]


def nul_cut_chunks():
    """the chunks of nul_blocks() that end in text and one to three NULs: zeros lie behind their end, in the pad, in
    the chunk of NULs that follows, or wherever the scan substitutes them"""
    return [c for c, (_, cut) in enumerate(nul_plan()) if cut]
