"""The cases of the literal-list tests (plain Python, no GPU): tests/test_gpu_set.py searches them on the device,
tests/test_set_host.py pins tests/set_model.py to the oracle on every one the oracle's regex reader accepts.

Geometry of k_set_scan (x-search_amd/csrc/xsg_set_kernels.hip): a tile is 16 KiB, a wave-load 1 KiB, a lane's unit 16 B."""
from functools import lru_cache

import numpy as np

import corpus
import set_model
from gpu_util import oracle_rx_all_modes
from xs_oracle import RegexProgram, UnsupportedRegex

TILE, WAVE_LOAD, UNIT = 16384, 1024, 16


def u8(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def expected(oracle, blocks, literals, icase=False, global_offsets=None, line_bases=None) -> dict:
    """every tag's result: the oracle's regex reader on E(S); a list it refuses (bytes >= 0x80 that are no UTF-8) is
    the brute-force model's, which test_set_host.py pins to the oracle wherever both answer"""
    try:
        prog = RegexProgram(set_model.expression(literals), icase)
    except UnsupportedRegex:
        return set_model.all_modes(blocks, literals, icase, global_offsets, line_bases)
    return oracle_rx_all_modes(oracle, blocks, prog, global_offsets, line_bases)


# ---- all seven tags: about 1 MiB in 5 chunks of unequal length, lists of 1, 2, 9 and 300 literals of 1..40 bytes -----------
TEXT_LENGTHS = (300_001, 150_017, 400_003, 65_537, 133_000)
LIST_SIZES = (1, 2, 9, 300)


@lru_cache(maxsize=None)
def text_blocks():
    return tuple(corpus.text_block(7, i, n, needle_rate=3e-4) for i, n in enumerate(TEXT_LENGTHS))


@lru_cache(maxsize=None)
def word_list(k: int):
    """k literals of mixed lengths 1..40 cut from the text (so they occur), some with their case swapped (so that
    XSG_FLAG_IGNORE_CASE finds more than the plain search); one-byte literals are capitals, which are rare."""
    if k == 1:
        return (b"Sherlock",)
    if k == 2:
        return (b"Holmes", b"Sherlock")
    text = text_blocks()[0].tobytes()
    rng = np.random.Generator(np.random.PCG64(1000 + k))
    lengths = [1, 2, 3, 4, 5, 7, 9, 13, 40, 22, 6, 8, 31, 17, 11]
    out = []
    while len(out) < k:
        n = lengths[len(out) % len(lengths)]
        at = int(rng.integers(0, len(text) - n))
        lit = text[at:at + n]
        if b"\n" in lit or (n == 1 and not lit.isupper()):
            continue
        if len(out) % 4 == 3:
            lit = lit.swapcase()
        out.append(lit)
    return tuple(out)


# ---- order and overlap ------------------------------------------------------------------------------------------------
def _abcd(n):
    return u8((b"abcd ab abc bcd xabcdx\nab\nbcd abcd\n" * (n // 34 + 1))[:n])


ORDER_CASES = [
    ("ab-abc", (b"ab", b"abc"), [_abcd(5000), _abcd(333)]),
    ("abc-ab", (b"abc", b"ab"), [_abcd(5000), _abcd(333)]),
    ("b-abc", (b"b", b"abc"), [_abcd(5000), _abcd(333)]),
    ("ab-bcd", (b"ab", b"bcd"), [_abcd(5000), _abcd(333)]),
    ("a_a", (b"a a",), [u8(b"ba a a"), u8(b"ba a a\na a a a a\n")]),
    # one chain across four tiles: every position is a candidate and each overlaps the next (heads and chains)
    ("aa-a-run", (b"aa", b"a"), [u8(b"a" * 65536)]),
]


# ---- every alignment: chunks of 32 KiB + 16 B, one occurrence of a 5-byte and of a 255-byte literal each ---------------------
LIT5 = b"Qx#Zj"
LIT255 = bytes((37 * i + 11) % 94 + 33 for i in range(255)).replace(b"Q", b"q")  # printable, no blank, no 'Q': never inside LIT5's
ALIGN_CHUNK = 2 * TILE + UNIT
ALIGN_OFFSETS = list(range(TILE - 260, TILE + 5)) + list(range(WAVE_LOAD - 8, WAVE_LOAD + 9))
# a second shortest literal sets the gram length: g = 1, 2, 3, 4 (none of them occurs in the filler or the two literals)
ALIGN_SHORTEST = {1: b"\x7f", 2: b"\x7f~", 3: b"\x7f~\x7f", 4: None}


@lru_cache(maxsize=None)
def align_blocks():
    """one chunk per offset: filler lines, the 255-byte literal at the offset, the 5-byte one 300 bytes behind its end --
    and once more the other way round in the second half of the list, so both literals start at every offset"""
    filler = (b"the quick brown fox jumps over the lazy dog\n" * (ALIGN_CHUNK // 44 + 1))[:ALIGN_CHUNK]
    blocks = []
    for first, second in ((LIT255, LIT5), (LIT5, LIT255)):
        for off in ALIGN_OFFSETS:
            b = bytearray(filler)
            b[off:off + len(first)] = first
            at = off + len(first) + 300
            b[at:at + len(second)] = second
            blocks.append(u8(b))
    return tuple(blocks)


def align_list(g: int):
    short = ALIGN_SHORTEST[g]
    return (LIT255, LIT5) + ((short,) if short else ())


# ---- chunk ends: tightly packed chunks, hostile bytes behind every end ---------------------------------------------------------
END_LITS = {1: (b"k", b"needle"), 2: (b"kq", b"needle"), 3: (b"kqz", b"needle"), 4: (b"kqzw", b"needle")}  # (shortest: g bytes, long)


_LINE = b"some text in front\nmore of it "  # (holds no byte of a shortest literal and no `needle`)


def _ending_in(tail: bytes, n: int):
    """n bytes of filler lines whose last bytes are `tail`"""
    return u8((_LINE * (n // len(_LINE) + 2))[:n - len(tail)] + tail)


@lru_cache(maxsize=None)
def end_plan(g: int):
    """-> ((chunk, lack), ...) for the list END_LITS[g] (shortest literal g bytes).  `lack` is what the chunk's last
    bytes need to become an occurrence, or b"" where they need nothing; end_fill puts it right behind the chunk's end.
      whole occurrences ending exactly at the end (lack nothing);
      `needle` cut short by 1 byte, by all but 1 byte, and after 3 bytes at the end of a tile; the shortest literal cut
        short by 1 byte (g > 1: a gram that straddles the end), in a small chunk and at the end of a tile.  Each comes
        twice: in a chunk whose pad is exactly `lack` long, so the pad completes it, and in a chunk whose length is a
        multiple of 16 (no pad at all) followed by a chunk that begins with `lack`;
      chunks of 1, g - 1, g, 15, 16, 17 bytes made of the shortest literal's bytes, the cut ones lacking its rest"""
    short, long_ = END_LITS[g]
    plan = [(_ending_in(long_, 37), b""), (_ending_in(short, 41), b"")]
    cuts = [(long_[:-1], 64), (long_[:1], 64), (long_[:3], TILE)]
    if g > 1:
        cuts += [(short[:-1], 64), (short[:-1], TILE)]
    for tail, n in cuts:
        whole = long_ if long_.startswith(tail) and tail != short[:-1] else short
        lack = whole[len(tail):]
        plan.append((_ending_in(tail, n - len(lack)), lack))  # the pad is `lack`
        plan.append((_ending_in(tail, n), lack))  # no pad: the next chunk follows at once
        plan.append((u8(lack + b" goes on\n"), b""))
    rep = short * 17
    for n in (1, g - 1, g, 15, 16, 17):
        if n > 0:
            rest = short[n % g:] if n % g else b""
            plan.append((u8(rep[:n]), rest if len(rest) <= -n % 16 else b""))  # (16 bytes have no pad to hold it)
    return tuple(plan)


def end_blocks(g: int):
    return [b for b, _ in end_plan(g)]


def end_cut_chunks(g: int):
    """the chunks of end_plan(g) that end inside an occurrence the bytes behind them complete"""
    return [c for c, (_, lack) in enumerate(end_plan(g)) if lack]


def end_fill(g: int):
    """what lies behind every chunk's end (the pad up to the next 16-byte boundary, the guards), in the form
    packing.pack_tight takes: fill(i, n) is the gap in FRONT of chunk i, so it follows chunk i - 1 and begins with
    what that chunk lacks; stale matches follow"""
    short, long_ = END_LITS[g]
    plan = end_plan(g)

    def fill(i, n):
        head = plan[i - 1][1] if i > 0 else b""
        body = head + (b" " + long_ + b"\n" + short) * (n // 4 + 2)
        return u8(body[:n])
    return fill


def end_naive_spans(g: int, icase: bool, packed, c: int):
    """a model of a kernel that reads past the end: the match walk over chunk c and the 255 bytes behind it (the
    longest literal the header allows) -> the (start, len) that begin inside the chunk"""
    short_long = END_LITS[g]
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    seen = packed.host[o:o + n + 255]
    return [s for s in set_model.Occurrences(seen, short_long, icase).spans() if s[0] < n]


# ---- a candidate-dense list -------------------------------------------------------------------------------------------------------
DENSE_LIST = (b"e", b"th")


@lru_cache(maxsize=None)
def dense_blocks():
    return (corpus.text_block(11, 0, 200_000), corpus.text_block(11, 1, 62_144))


# ---- bytes that are no UTF-8: the oracle's reader refuses them, the model serves them --------------------------------------------
RAW_LIST = (b"\xff\xfe", b"caf\xe9", b"\x80")


def raw_blocks():
    t = bytearray(corpus.text_block(13, 0, 40_000).tobytes())
    for at, lit in ((100, b"caf\xe9"), (5000, b"\xff\xfe\xff\xfe"), (TILE - 1, b"\xff\xfe"), (20_000, b"\x80\x80caf\xe9"), (39_990, b"CAF\xe9")):
        t[at:at + len(lit)] = lit
    return [u8(t), u8(b"\x80caf\xe9\n\xff")]
