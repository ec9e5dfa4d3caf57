"""Bindings whose chunks lie at buffer offsets beyond 2^31 and 2^32: the layouts, their decoys and the patterns of
tests/test_high_offsets_layout.py (CPU) and tests/test_gpu_high_offsets.py.  numpy only: nothing here touches a GPU.

A LAYOUT is a list of Chunk records (offset, block, global_offset, line_base) in binding order plus `writes`, the ordered
list of (address, bytes) that fills the buffer: guards first, decoys next, the chunks last, so a bound chunk always holds
its own bytes.  The buffer is about 6 GiB; only what `writes` names is ever defined, and no search may depend on the rest.

  abutting    control chunk at 4096 | a chunk across 2^31 | a chunk whose padded end is 2^32 | a chunk that begins at 2^32 |
              an empty chunk at 2^32 + 2^20 | 257 small chunks packed at 16-byte steps from 2^32 + 2^21 |
              a chunk at 2^32 + 2^31 + 4096 (the top bit of the offset's low word is set)
  straddling  the same, the two chunks around 2^32 replaced by one that starts at 2^32 - 3 * TILE - 16 and holds a match
              and a line across 2^32

The two straddling chunks keep the start offsets they were specified with (5 and 3 tiles and 16 bytes below the boundary)
and are therefore 7 and 5 tiles and a few bytes long, not 33 to 40 KiB: a chunk of 40 KiB that starts 80 KiB below 2^31
does not reach it.

DECOYS.  A kernel that loses the high bits of an address reads `address mod 2^31` or `address mod 2^32`.  Every bound
chunk is cut at the multiples of 2^31; for every piece at or above 2^31 a decoy -- seeded text of the piece's length that
is not the piece's -- is written at both images where they differ from the piece's address.  Where an image meets a bound
chunk the chunk wins (it is written last): a truncated read sees that chunk's text there, which is other text as well.
Layout.image(chunk, modulus) is what such a read of the whole chunk returns; the CPU test demands that the oracle tells
it from the chunk for every pattern.  So no small chunk can be told from its decoy by chance, the small chunks that hold a
byte are RICH (every pattern matches) or POOR (none does) and their decoys are of the other family; a chunk shorter than
a pattern's shortest match could never differ from a decoy of its length, so these chunks are 61 to 64 bytes long (one,
where every line matches every pattern, has 120), and the chunks without a byte are the short ones.

GUARDS.  The 256 bytes before and the 4096 bytes behind every chunk and decoy hold 0xA5."""
from collections import namedtuple

import numpy as np

TILE = 16384
B31, B32 = 1 << 31, 1 << 32
GUARD_BEFORE, GUARD_AFTER, GUARD_BYTE = 256, 4096, 0xA5
CAPACITY = B32 + B31 + 4096 + (64 << 10)
N_SMALL = 257
SMALL_BASE = B32 + (1 << 21)

Chunk = namedtuple("Chunk", "name offset block global_offset line_base")

AB32 = b"ab" * 16
# every pattern of PATTERNS matches in each of these; RICH_TAIL ends in a match, RICH_HEAD begins with `x that`
RICH_HEAD = b"x that ing going\nx colour aa " + AB32                     # 61 bytes, the last line lacks its newline
RICH_B = b"x colour going\nx aa that ing " + AB32                        # 61 bytes
RICH_TAIL = b"x colour going\nx aa " + AB32 + b" ing that"                # 61 bytes; ends in `that`
EVERY_LINE = (b"x that colour aa " + AB32 + b" ing going\n") * 2         # every line holds a match of every pattern but g\nx, which lies between them
LAST_LINE = EVERY_LINE[:59]                                               # one such line without its newline: `(?m)\\w+ing$` holds at the chunk's end
WORDS = [b"that", b"That", b"colour", b"color", b"COLOUR", b"running", b"going", b"x", b"xy", b"aa", b"aaa", b"aaaaa", b"AA",
         b"plain", b"words", b"zebra", b"the", b"bat", b"thet", b"g", b"sing", b"THAT", b"ing", b"abbab", b"ab" * 20, b"babbaab" * 3, b"thatch", b"recolour"]
POOR_WORDS = [b"plain", b"words", b"the", b"bat", b"lamp", b"Quiet", b"7", b"--", b"row", b"hut"]

X, IC, RX, INV = 0x1, 0x2, 0x4, 0x8  # xsg.FLAG_EXACT_TAIL, _IGNORE_CASE, _REGEX, _INVERT (asserted in the tests that import xsg)

# (id, kind, pattern or literals, pattern flags); the kinds of tests/per_chunk_model.py, "anyof_w" / "allof_w": whole words
PATTERNS = [
    ("literal", "lit", b"that", 0),
    ("aa_overlapping", "lit", b"aa", 0),
    ("literal_with_newline", "nl", b"g\nx", 0),
    ("class_sequence", "rx", b"th[ae]t", RX),
    ("class_sequence_9", "rx", b"[ab]{9}", RX),       # tests/class_paths.py: DIRECTED, "dense, overlaps itself"
    ("class_sequence_32", "rx", b"[ab]{31}b", RX),    # tests/class_paths.py: DENSE_OVERLAP, 32 positions
    ("prefilter", "rx", b"colou?r", RX),
    ("line_walk", "rx", b"\\w+ing", RX),
    ("anchored_begin", "anchor", b"(?m)^x", RX),
    ("anchored_end", "anchor", b"(?m)\\w+ing$", RX),  # tests/test_gpu_anchors.py: AUTOMATON
    ("any_of", "anyof", (b"that", b"colour", b"zebra"), 0),
    ("any_of_words", "anyof_w", (b"that", b"colour", b"zebra"), 0),
    ("all_of", "allof", (b"that", b"ing"), 0),
    ("all_of_words", "allof_w", (b"that", b"ing"), 0),
]
# the list of the per-literal counters: duplicates, a literal that covers another, one that is absent
LITERALS = (b"that", b"hat", b"colour", b"our", b"aa", b"that", b"ing", b"going", b"zebra", b"absent-literal", b"x", b"ab")


def u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


def words_text(rng, nbytes: int, terminated: bool, words=WORDS):
    out, size = [], 0
    while size < nbytes:
        w = words[int(rng.integers(0, len(words)))] + (b"\n" if rng.random() < 0.3 else b" ")
        out.append(w)
        size += len(w)
    b = u8(b"".join(out)[:nbytes])
    if terminated:
        b[-1] = 10
    return b


def big_block(rng, nbytes: int, head=b"", tail=b"", terminated=True):
    """word salad of nbytes with EVERY_LINE in it (every pattern matches in every large chunk), `head` / `tail` at its ends"""
    b = words_text(rng, nbytes, terminated and not tail)
    at = nbytes // 3
    nl = at + int(np.flatnonzero(b[at:] == 10)[0]) + 1  # (EVERY_LINE begins a line)
    b[nl:nl + len(EVERY_LINE)] = u8(EVERY_LINE)
    if head:
        b[:len(head)] = u8(head)
    if tail:
        b[nbytes - len(tail) - 1] = 10
        b[nbytes - len(tail):] = u8(tail)
    return b


def rich_small(rng):
    t = (RICH_HEAD, RICH_B)[int(rng.integers(0, 2))]
    run = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 31).tolist()) + b"b"
    t = t[:-32] + run
    return u8(t + (b"", b"\n", b"\n ", b" \n")[int(rng.integers(0, 4))])


def poor_small(rng, n: int):
    return words_text(rng, n, bool(rng.random() < 0.5), POOR_WORDS)


def opposite(rng, block):
    """a decoy of a small chunk: of its length and of the other family"""
    n = int(block.size)
    if is_rich(block):
        return poor_small(rng, n)
    assert n >= len(RICH_HEAD), n
    return u8(RICH_HEAD + b"\n" * (n - len(RICH_HEAD)))


def is_rich(block) -> bool:
    return b"that" in block.tobytes()


def small_blocks(rng):
    """257 chunks: without a byte first, last and in runs; one where every line matches, one without a match, a matching
    last line without its newline"""
    n = N_SMALL
    blocks = [rich_small(rng) if rng.random() < 0.5 else poor_small(rng, int(rng.integers(61, 65))) for _ in range(n)]
    for i in (0, 1, 100, 101, 102, 103, 104, n - 1):
        blocks[i] = u8(b"")
    blocks[2] = u8(EVERY_LINE)
    blocks[3] = poor_small(rng, 64)
    blocks[4] = u8(RICH_HEAD)            # the matching last line lacks its newline
    blocks[n - 2] = u8(RICH_TAIL)        # ... in the last chunk that holds a byte
    return blocks


def offsets_and_bases(n: int):
    """disjoint global ranges and line bases in an order that is not the chunks' (7919 and 31 are coprime to n = 263)"""
    go = [((i * 7919) % n) * 1_000_000 + 13 for i in range(n)]
    lb = [((i * 31) % n) * 1_000 + 7 for i in range(n)]
    return go, lb


class Layout:
    def __init__(self, name, chunks, seed):
        self.name = name
        self.chunks = chunks
        self.capacity = CAPACITY
        rng = np.random.default_rng(seed)
        self.decoys = []  # (chunk index, modulus, address, bytes)
        for i, c in enumerate(chunks):
            lo, hi = c.offset, c.offset + int(c.block.size)
            cut = lo
            while cut < hi:  # the pieces between multiples of 2^31
                end = min(hi, (cut // B31 + 1) * B31)
                if cut >= B31:
                    piece = c.block[cut - lo:end - lo]
                    for m in (B31, B32):
                        if cut % m != cut:
                            text = opposite(rng, piece) if c.name.startswith("small") else words_text(rng, end - cut, True)
                            self.decoys.append((i, m, cut % m, text))
                cut = end
        guard = lambda a, n: [(max(a - GUARD_BEFORE, 0), np.full(a - max(a - GUARD_BEFORE, 0), GUARD_BYTE, dtype=np.uint8)),
                              (a + n, np.full(GUARD_AFTER, GUARD_BYTE, dtype=np.uint8))]
        spans = [(c.offset, int(c.block.size)) for c in chunks] + [(a, int(t.size)) for _, _, a, t in self.decoys]
        self.writes = [w for a, n in spans for w in guard(a, n) if w[1].size]
        self.writes += [(a, t) for _, _, a, t in self.decoys]
        self.writes += [(c.offset, c.block) for c in chunks if c.block.size]
        assert all(0 <= a and a + t.size <= self.capacity for a, t in self.writes)
        self._lo = np.array([a for a, _ in self.writes], dtype=np.int64)
        self._hi = np.array([a + t.size for a, t in self.writes], dtype=np.int64)

    def read(self, addr: int, n: int):
        """the n bytes at addr of the filled buffer; asserts that every one of them was written"""
        out = np.zeros(n, dtype=np.uint8)
        known = np.zeros(n, dtype=bool)
        for k in np.flatnonzero((self._lo < addr + n) & (self._hi > addr)):
            a, t = self.writes[int(k)]
            lo, hi = max(a, addr), min(a + t.size, addr + n)
            out[lo - addr:hi - addr] = t[lo - a:hi - a]
            known[lo - addr:hi - addr] = True
        assert known.all(), (self.name, addr, n, "a truncated read meets bytes that nothing wrote")
        return out

    def image(self, i: int, modulus: int):
        """what a read of chunk i returns whose addresses lost the bits from `modulus` on; None if that is the chunk itself"""
        c = self.chunks[i]
        lo, hi = c.offset, c.offset + int(c.block.size)
        if hi <= modulus:
            return None
        parts, cut = [], lo
        while cut < hi:
            end = min(hi, (cut // modulus + 1) * modulus)
            parts.append(self.read(cut % modulus, end - cut))
            cut = end
        return np.concatenate(parts)

    def blocks(self):
        return [c.block for c in self.chunks]

    def global_offsets(self):
        return [c.global_offset for c in self.chunks]

    def line_bases(self):
        return [c.line_base for c in self.chunks]


def _layouts():
    rng = np.random.default_rng(20250)
    go, lb = offsets_and_bases(N_SMALL + 6)
    control = big_block(rng, 35_011, terminated=False)
    across31 = big_block(rng, 7 * TILE + 1_234)
    # a line and a match across 2^31: byte 5 * TILE + 16 of the chunk is address 2^31
    at = 5 * TILE + 16
    across31[at - 23] = 10
    across31[at - 22:at + 39] = u8(RICH_B)  # `x colour going\nx aa th|at ing ab...`: `that` and its line lie across the boundary
    across31[at + 39] = 10
    to32 = big_block(rng, 34_000, tail=RICH_TAIL)                     # its padded end is 2^32
    assert to32.size % 16 == 0
    from32 = big_block(rng, 3_000, head=RICH_HEAD[:17])               # begins at 2^32 with `x that` at byte 0
    empty = u8(b"")
    smalls = small_blocks(rng)
    last = big_block(rng, 36_502, terminated=False, tail=LAST_LINE)   # an unterminated matching last line above 2^32
    across32 = big_block(rng, 5 * TILE + 2_345)
    at = 3 * TILE + 16
    across32[at - 23] = 10
    across32[at - 22:at + 39] = u8(RICH_B)
    across32[at + 39] = 10
    for b in [control, across31, to32, from32, last, across32] + smalls:
        b.setflags(write=False)

    small_offsets, o = [], SMALL_BASE
    for b in smalls:
        small_offsets.append(o)
        o += (int(b.size) + 15) // 16 * 16
    head = [("control", 4096, control), ("across_2_31", B31 - 5 * TILE - 16, across31)]
    around = [("ends_at_2_32", B32 - to32.size, to32), ("begins_at_2_32", B32, from32)]
    rest = [("empty", B32 + (1 << 20), empty)] + [("small%d" % k, small_offsets[k], smalls[k]) for k in range(N_SMALL)]
    rest.append(("top_bit_of_low_word", B32 + B31 + 4096, last))
    abut = head + around + rest
    index = {name: k for k, (name, _, _) in enumerate(abut)}
    strad = head + [("across_2_32", B32 - 3 * TILE - 16, across32)] + rest
    index["across_2_32"] = index["ends_at_2_32"]
    mk = lambda spec: [Chunk(name, off, blk, go[index[name]], lb[index[name]]) for name, off, blk in spec]
    return {"abutting": Layout("abutting", mk(abut), 31), "straddling": Layout("straddling", mk(strad), 32)}


_CACHE = {}


def layouts():
    if not _CACHE:
        _CACHE.update(_layouts())
    return _CACHE


# ---- the oracle per chunk: tests/per_chunk_model.py, and the whole-word lists through tests/words_model.py ---------------------
def chunk_plain(oracle, kind, pat, pflags, flags, b, g, lb):
    """per_chunk_model.chunk_plain with the kinds "anyof_w" / "allof_w" (XSG_LIST_WHOLE_WORDS) next to its own"""
    import all_of_model
    import invert_model
    import per_chunk_model
    import words_model
    if kind == "anyof_w":
        want = words_model.all_modes([b], list(pat), bool(flags & IC), global_offsets=[g], line_bases=[lb])
        return invert_model.invert_all_modes(want, [b], [g], [lb]) if flags & INV else want
    if kind == "allof_w":
        return all_of_model.all_modes([b], list(pat), bool(flags & IC), True, bool(flags & INV), global_offsets=[g], line_bases=[lb])
    return per_chunk_model.chunk_plain(oracle, kind, pat, pflags, flags, b, g, lb)


def chunk_matches(oracle, kind, pat, pflags, flags, b, g):
    import per_chunk_model
    import words_model
    if kind == "anyof_w":
        s, o, _ = words_model.matches([b], list(pat), bool(flags & IC), [g])
        return s, o
    return per_chunk_model.chunk_matches(oracle, kind, pat, pflags, flags, b, g)


def signature(oracle, kind, pat, pflags, b):
    """what the decoy condition compares: (count_matches, line_byte_offsets) of the chunk alone at global offset 0"""
    w = chunk_plain(oracle, kind, pat, pflags, 0, b, 0, 0)
    return w.get("count_matches"), [int(x) for x in w["line_byte_offsets"]]
