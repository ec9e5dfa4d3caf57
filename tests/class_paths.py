"""Class-sequence expressions of 9 to 32 positions, and the five ways k_scan decides a candidate (plain Python, no GPU).

x-search_amd/csrc/xsg_pattern.cpp: class_fields picks the filter window of an expression (koff) and the verification
its candidates get; x-search_amd/csrc/xsg_kernels.hip (scan_load, match_mask16_from, cls_verify_positions) acts on it:

  exact               the window compare is the decision (cls_exact)
  inreg               the cls_chk positions looked up in registers (cls_inreg)
  view                the lane's 32-byte view in LDS: up to 12 positions, the match starts inside the unit
  memory:long         more than 12 positions: a byte at a time from memory, one `alive` bit per alternative
  memory:before-unit  koff > 0 and the window lies in the first koff bytes of its 16-byte unit: the match starts in the
                      previous unit (wave-load, span, tile) -- the same walk

  class_fields(expr, flags)   what the compiler chose (xsg_test_class_fields: host only, XSG_TEST_HOOKS=1)
  info_of(expr, flags)        that, and the sets of every alternative as [alternative, position, byte] booleans
  path_of(f, window_byte)     the path model
  DIRECTED                    expressions that are each there for a path, with the path
  rand_long_expr(rng)         9..32 positions, 1..8 alternatives, the pinned 8-byte stretch at a random offset
  build_text(info, rng, ..)   chunks in which the expression really occurs, with decoys, planted at the geometry edges:
                              a packing.Case, so tests/packing.py packs it and fills the bytes around it
  events(info, block)         a byte-wise model of acceptance and of the window filter: true positions, filter-passing
                              positions that are no match, positions only the union of the alternatives accepts
  reader_koff_before          the model reader of the new direction: it looks koff bytes in front of a chunk"""
import ctypes as C
from collections import namedtuple

import numpy as np

import corpus
import packing as P
import xsg

IC, RX = xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX
UNIT, REG_VERIFY = 16, 12  # xsg_devutil.h: kUnit; xsg_kernels.hip: kRegVerify
PATHS = ("exact", "inreg", "view", "memory:long", "memory:before-unit")
FIELDS = ("plen", "nalt", "koff", "cls_fast", "cls_inreg", "cls_exact", "cls_chk", "ascii_only", "has_newline", "m0", "m1", "p0", "p1")
Fields = namedtuple("Fields", FIELDS)
Info = namedtuple("Info", "expr flags f table union agree value")
MAX_CHUNK = 3 * P.TILE + UNIT  # 49 168
EDGES = (P.TILE, P.WAVE_SPAN, P.WAVE_LOAD, P.UNIT)


def class_fields(expr: bytes, flags: int = 0) -> Fields:
    """xsg_test_class_fields; raises xsg.XsgError (ENOTSUP) for what goes to the automaton route or is a plain literal"""
    lib = xsg.load()
    fn = lib.xsg_test_class_fields
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t]
    out = (C.c_uint32 * len(FIELDS))()
    rc = fn(expr, len(expr), flags & IC, out, len(FIELDS))
    if rc != xsg.OK:
        raise xsg.XsgError(rc, lib.xsg_last_error().decode("utf-8", "replace"))
    return Fields(*[int(x) for x in out])


def info_of(expr: bytes, flags: int = 0) -> Info:
    f = class_fields(expr, flags)
    n, na, ao, sets = xsg.regex_info(expr, flags & IC)
    assert (n, na, int(ao)) == (f.plen, f.nalt, f.ascii_only), (expr, n, na, ao, f)
    table = ((sets[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(na, n, 256)
    union = table.any(axis=0)
    m, p = f.m0 | f.m1 << 32, f.p0 | f.p1 << 32
    agree = [(m >> 8 * i) & 0xff for i in range(8)]
    value = [(p >> 8 * i) & 0xff for i in range(8)]
    return Info(bytes(expr), flags & IC, f, table, union, agree, value)


def info_or_none(expr: bytes, flags: int = 0):
    """info_of, or None where the expression is a plain literal under these flags (`[Ss]herlock` without case): it is
    then searched as an ordinary pattern and class_fields has no say"""
    n, na, _, sets = xsg.regex_info(expr, flags & IC)
    if na == 1 and all(int(sum(bin(int(x)).count("1") for x in sets[0, k])) == 1 for k in range(n)):
        return None
    return info_of(expr, flags)


def path_of(f: Fields, window_byte: int) -> str:
    """the path k_scan takes for a candidate whose filter window begins at byte `window_byte` of its 16-byte unit"""
    if f.cls_exact:
        return "exact"
    if f.cls_inreg:
        return "inreg"
    if window_byte - f.koff < 0:
        return "memory:before-unit"
    return "view" if f.plen <= REG_VERIFY else "memory:long"


def paths_of(f: Fields) -> set:
    return {path_of(f, b) for b in range(UNIT)}


def window_len(f: Fields) -> int:
    return min(8, f.plen - f.koff)


# ---- the directed expressions: (expression, the paths it is there for, text alphabet or None, note)
Directed = namedtuple("Directed", "expr paths alphabet note")
ALT8x8 = b"|".join(bytes([97 + i]) * 4 + bytes([110 + i]) * 4 for i in range(8))       # aaaannnn|bbbboooo|...: nothing merges
ALT7x9 = b"|".join(bytes([97 + i]) * 5 + bytes([110 + i]) * 4 for i in range(7))
DENSE = b"ab" * 20 + b"\n"  # the `ab\n` alphabet with a newline every ~40 bytes: runs long enough for 32 positions
FACTOR_EXPR, FACTOR_OF = b"\\w+ing of the [a-z]{4}", b"\\wing of the [a-z]{4}"  # the automaton route, and its 16-position factor as an expression

DIRECTED = [
    Directed(b"[a-z]{3}Sherlock", {"view", "memory:before-unit"}, None, "koff 3"),
    Directed(b"[a-z]{5} Sherlock Holmes", {"memory:long", "memory:before-unit"}, None, "21 positions, koff > 0"),
    Directed(b"Sherlock [A-Z][a-z]{5}", {"memory:long"}, None, "15 positions, koff 0"),
    Directed(b"[0-9]{4}-[0-9]{2}-[0-9]{2}T[0-9]{2}:[0-9]{2}", {"memory:long", "memory:before-unit"}, None, "16 positions, no fully pinned window"),
    Directed(b"\\w{8}ing \\w{4}", {"memory:long", "memory:before-unit"}, None, "16 positions"),
    Directed(b"(Sherlock|detectiv) (Holmes|street)", {"memory:long", "memory:before-unit"}, None, "4 alternatives x 15"),
    Directed(b"a{32}|b{32}", {"memory:long"}, DENSE, "64 sets exactly"),
    Directed(ALT8x8, {"view"}, None, "8 alternatives of 8 positions"),
    Directed(ALT7x9, {"view"}, None, "7 alternatives of 9 positions: 63 sets"),
    Directed(b"Sherlock [a-z]{3}", {"view"}, None, "12 positions: the last the view takes"),
    Directed(b"Sherlock [a-z]{4}", {"memory:long"}, None, "13 positions: the first the memory walk takes"),
    Directed(b"[a-z]{4}Sherlock", {"view", "memory:before-unit"}, None, "12 positions, koff 4"),
    Directed(b"[a-z]{5}Sherlock", {"memory:long", "memory:before-unit"}, None, "13 positions, koff 5"),
    Directed(b"x.{11}y", {"memory:long"}, None, "ASCII-only, 13 positions"),
    Directed(b"x.{10}y", {"view"}, None, "ASCII-only, 12 positions"),
    Directed(b"x.{12}y", {"memory:long"}, None, "ASCII-only, 14 positions"),
    Directed(b"[^a]{13}", {"memory:long"}, None, "ASCII-only, a negated class, accepts '\\n'"),
    Directed(b"[ab]{9}", {"view"}, DENSE, "dense, overlaps itself"),
    Directed(b"a[ab]{15}", {"memory:long"}, DENSE, "dense, overlaps itself"),
    Directed(b"[ab]{31}b", {"memory:before-unit"}, DENSE, "dense, overlaps itself, koff 24: every window lies in the first koff bytes of its unit"),
    Directed(b"(Sherlock|detectiv)[a-z]", {"view"}, None, "2 alternatives x 9, koff 0"),
    Directed(b"[a-z](Sherlock|detectiv)", {"view", "memory:before-unit"}, None, "2 alternatives x 9, koff 1"),
    Directed(b"[a-z]{2}(Holmes s|street S)[a-z]", {"view", "memory:before-unit"}, None, "2 alternatives x 11, koff > 0"),
    Directed(b"[a-z](Sherlock|detectiv) (Holmes|street)", {"memory:long", "memory:before-unit"}, None, "4 alternatives x 16: 64 sets, koff > 0"),
    Directed(b"Sherlock (Holmes|Watson)", {"memory:long"}, None, "2 alternatives x 15, koff 0"),
    Directed(b"Sherlock[a-z]{3}(ab|cd)", {"memory:long"}, None, "2 alternatives x 13, koff 0"),
    Directed(b"detectiv(e street|es walks)", {"memory:long"}, None, "2 alternatives x 16, koff 0"),
    # up to 8 positions, one alternative: decided in registers
    Directed(b"[Ss]herlock", {"exact"}, None, ""), Directed(b"[Hh]olmes", {"exact"}, None, ""),
    Directed(b"[Ss]he", {"exact"}, None, ""), Directed(b"stree[tu]", {"exact"}, None, ""),
    Directed(b"w[ai]tson", {"exact"}, None, ""), Directed(b"[01]234", {"exact"}, None, ""),
    Directed(b"She[r ]lock", {"inreg"}, None, ""), Directed(b"Sh[a-z]rlock", {"inreg"}, None, ""),
    Directed(b"[a-z]olmes", {"inreg"}, None, ""), Directed(b"t[a-z]e", {"inreg"}, None, ""),
    Directed(b"[0-9]{4}", {"inreg"}, None, ""), Directed(b"stre[a-z]t", {"inreg"}, None, ""),
]
KOFF_POSITIVE, MULTI_ALT, DENSE_OVERLAP = b"[a-z]{5} Sherlock Holmes", b"(Sherlock|detectiv) (Holmes|street)", b"[ab]{31}b"
AT_LIMIT = [(b"a{32}|b{32}", 32, 2), (ALT8x8, 8, 8), (ALT7x9, 9, 7)]
OVER_LIMIT = [b"a{32}|b{32}|c{32}", b"|".join(bytes([97 + i]) * 5 + bytes([110 + i]) * 4 for i in range(8)), b"(a{16}|b{16})(c{16}|d{16})"]


# ---- random expressions
WINDOWS = [b"Sherlock", b"detectiv", b" Holmes ", b"street S", b"Watson s", b"e street", b"k Holmes"]
SEEDS_DEFAULT, SEEDS_HOT1 = (9101, 9102, 9103), (9201, 9202)
SEEDS = SEEDS_DEFAULT + SEEDS_HOT1


def _token(rng, dotty: bool) -> bytes:
    k = int(rng.integers(0, 12 if dotty else 10))
    if k <= 2:
        return bytes([b"abcxyz019_ "[int(rng.integers(0, 11))]])
    if k == 3:
        return b"[xy]"
    if k == 4:
        return [b"[a-z]", b"[a-f]", b"[A-Z]"][int(rng.integers(0, 3))]
    if k == 5:
        return b"[0-9]"
    if k == 6:
        return b"\\d"
    if k <= 9:
        return b"\\w"
    return [b".", b"[^a-c]", b"[^0-9 ]"][int(rng.integers(0, 3))]


def _join(tokens) -> bytes:
    """the tokens in order; a run of equal ones becomes tok{n} half of the time (by the run's length, no more draws)"""
    out, i = b"", 0
    while i < len(tokens):
        j = i
        while j < len(tokens) and tokens[j] == tokens[i]:
            j += 1
        n = j - i
        out += tokens[i] + (b"{%d}" % n if n > 1 and (n + len(out)) & 1 else tokens[i] * (n - 1))
        i = j
    return out


def rand_long_expr(rng) -> bytes:
    """9..32 positions, 1..8 alternatives, at most 64 sets.  Every alternative holds the same eight literal bytes at the
    same random offset (the window the compiler should pick: koff varies); the other positions are literals, [xy],
    ranges, \\d, \\w and -- a third of the expressions -- '.' or a negated class.  Alternatives differ from one another
    in two positions that hold a letter of their own each, so no two merge into one class sequence."""
    plen = int(rng.integers(9, 13)) if rng.random() < 0.4 else int(rng.integers(13, 33))  # (both sides of kRegVerify)
    nalt = int(rng.integers(2, min(8, 64 // plen) + 1)) if rng.random() < 0.5 else 1
    dotty = rng.random() < 1 / 3
    at = int(rng.integers(0, plen - 8 + 1))
    if rng.random() < 0.25:
        at = 0 if rng.random() < 0.5 else plen - 8
    window = WINDOWS[int(rng.integers(0, len(WINDOWS)))]
    # runs of one token, as expressions are written ([a-z]{5}, \w{8}); a literal stands alone
    common = []
    while len(common) < plen:
        t = _token(rng, dotty)
        common += [t] * (1 if len(t) == 1 and t != b"." else int(rng.integers(1, 5)))
    common = common[:plen]
    for i in range(8):
        common[at + i] = bytes([window[i]])
    free = [k for k in range(plen) if not at <= k < at + 8]
    if all(len(common[k]) == 1 and common[k] != b"." for k in free):  # (all literals would be no class sequence at all)
        common[free[int(rng.integers(0, len(free)))]] = b"\\w"
    differ = sorted(int(x) for x in rng.choice(free, size=2, replace=False)) if nalt > 1 and len(free) >= 2 else []
    if len(differ) < 2:
        nalt = 1
    alts = []
    for a in range(nalt):
        seq = list(common)
        if nalt > 1:
            seq[differ[0]], seq[differ[1]] = bytes([ord("a") + a]), bytes([ord("k") + a])
        alts.append(_join(seq))
    return b"|".join(alts)


# ---- members, decoys
PRINTABLE = np.zeros(256, dtype=bool)
PRINTABLE[0x20:0x7f] = True
LETTERS = np.zeros(256, dtype=bool)
LETTERS[0x61:0x7b] = True


def _pick(rng, allowed: np.ndarray):
    """a byte of `allowed` [256 bool]: a lower-case letter if there is one, else printable, else ASCII, else any; None if empty"""
    for pool in (allowed & LETTERS, allowed & PRINTABLE, allowed & (np.arange(256) < 0x80), allowed):
        c = np.flatnonzero(pool)
        if c.size:
            return int(c[int(rng.integers(0, c.size))])
    return None


def member(info: Info, rng, alt=None) -> bytes:
    a = int(rng.integers(0, info.f.nalt)) if alt is None else alt
    return bytes(_pick(rng, info.table[a, k]) for k in range(info.f.plen))


def fold(data: np.ndarray) -> np.ndarray:
    d = np.asarray(data, dtype=np.uint8)
    return np.where((d >= 0x41) & (d <= 0x5a), d + 32, d).astype(np.uint8)


def accepts(info: Info, s: bytes) -> bool:
    d = fold(P.u8(s)) if info.flags & IC else P.u8(s)
    return len(s) == info.f.plen and bool(info.table[:, np.arange(info.f.plen), d].all(axis=1).any())


def decoy_outside(info: Info, rng, m: bytes):
    """one byte outside the filter window changed to a byte no alternative takes there: passes the filter, fails verification"""
    f = info.f
    ks = [k for k in range(f.plen) if not f.koff <= k < f.koff + 8]
    for k in [ks[int(i)] for i in rng.permutation(len(ks))] if ks else []:
        x = _pick(rng, ~info.union[k] & PRINTABLE)
        if x is not None and not accepts(info, m[:k] + bytes([x]) + m[k + 1:]):
            return m[:k] + bytes([x]) + m[k + 1:]
    return None


def decoy_inside(info: Info, rng, m: bytes):
    """one byte inside the window changed to a value that agrees on the window's `agree` bits and is in no set there
    ('{' or '`' for [a-z]): the compare passes it, the sets do not"""
    f = info.f
    idx = np.arange(256)
    for i in [int(i) for i in rng.permutation(window_len(f))]:
        k = f.koff + i
        x = _pick(rng, ((idx & info.agree[i]) == info.value[i]) & ~info.union[k] & (idx != 10) & (idx < 0x80))
        if x is not None and not accepts(info, m[:k] + bytes([x]) + m[k + 1:]):
            return m[:k] + bytes([x]) + m[k + 1:]
    return None


def crossover(info: Info, rng):
    """a string spliced from two alternatives that the position-wise union takes and no single alternative does"""
    f = info.f
    if f.nalt < 2:
        return None
    for _ in range(8):
        a, b = (int(x) for x in rng.choice(f.nalt, size=2, replace=False))
        ma, mb = member(info, rng, a), member(info, rng, b)
        for k in [int(i) for i in rng.permutation(np.arange(1, f.plen))]:
            s = ma[:k] + mb[k:]
            if not accepts(info, s):
                return s
    return None


# ---- the byte-wise model of a chunk
Events = namedtuple("Events", "accept filt union")  # bool per start 0..L - plen: a match begins; the window filter passes; the union accepts


def events(info: Info, block) -> Events:
    f = info.f
    d = fold(block) if info.flags & IC else np.asarray(block, dtype=np.uint8)
    n = d.size - f.plen + 1
    if n <= 0:
        z = np.zeros(0, dtype=bool)
        return Events(z, z, z)
    acc = np.zeros(n, dtype=bool)
    for a in range(f.nalt):
        ok = np.ones(n, dtype=bool)
        for k in range(f.plen):
            ok &= info.table[a, k][d[k:k + n]]
        acc |= ok
    uni = np.ones(n, dtype=bool)
    for k in range(f.plen):
        uni &= info.union[k][d[k:k + n]]
    filt = np.ones(n, dtype=bool)
    for i in range(window_len(f)):
        filt &= (d[f.koff + i:f.koff + i + n] & info.agree[i]) == info.value[i]
    return Events(acc, filt, uni)


def greedy(accept: np.ndarray, plen: int) -> list:
    """leftmost, non-overlapping: the walk of the reference (and of re.finditer)"""
    out, nxt = [], 0
    for s in np.flatnonzero(accept).tolist():
        if s >= nxt:
            out.append(s)
            nxt = s + plen
    return out


def census(info: Info, blocks, true_starts) -> dict:
    """path -> {"true": matches of the oracle on it, "decoy": filter-passing positions that are no match, "cross": positions
    the union accepts and no alternative does}.  true_starts[c]: the oracle's chunk-relative match offsets of chunk c.
    Every start counts, up to the last one at L - plen: a class sequence is searched with exact_tail (class_fields), so
    k_scan's position limit is L - plen + 1 and no start is left to the end-of-chunk walk."""
    f = info.f
    out = {p: {"true": 0, "decoy": 0, "cross": 0} for p in PATHS}
    for b, true in zip(blocks, true_starts):
        ev = events(info, b)
        assert list(true) == greedy(ev.accept, f.plen), (info.expr, "the model's accept map and the oracle's walk differ")
        assert not (ev.accept & ~ev.filt).any() and not (ev.accept & ~ev.union).any(), info.expr
        for key, starts in (("true", np.asarray(true, dtype=np.int64)), ("decoy", np.flatnonzero(ev.filt & ~ev.accept)),
                            ("cross", np.flatnonzero(ev.union & ~ev.accept))):
            for wb in ((starts + f.koff) % UNIT).tolist():
                out[path_of(f, wb)][key] += 1
    return out


# ---- texts
WORDS = [w for w in corpus.LEXICON_NOSH if w.islower()] + [b"Sherlock", b"Holmes", b"detective", b"street", b"Sher", b"She", b"2024-01-", b"x", b"y"]
Text = namedtuple("Text", "info case plants missed")  # case: a packing.Case; plants: (chunk, offset, what); missed: (edge, rel) wishes without room


def _background(rng, n: int, alphabet, extra) -> np.ndarray:
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    if alphabet is not None:
        a = np.frombuffer(alphabet, dtype=np.uint8)
        return a[rng.integers(0, len(a), size=n)].copy()
    words = WORDS + list(extra)
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + (b"\n" if rng.random() < 0.12 else b" ")
    return P.u8(bytes(out[:n]))


def edge_rels(plen: int, koff: int) -> list:
    """where a match starts relative to a geometry edge B: the match at B - plen, B - 1, B; the window (start + koff) at
    B - 8, B - 1, B, and at B + j for every j < koff -- there the match begins in front of the edge"""
    rels = []
    for r in [-plen, -1, 0, -8 - koff, -1 - koff, -koff] + [j - koff for j in range(koff)]:
        if r not in rels:
            rels.append(r)
    return rels


def rel_groups(plen: int, koff: int) -> list:
    """edge_rels in groups whose members do not overlap one another around the same edge: one chunk carries a group"""
    groups = []
    for r in edge_rels(plen, koff):
        for g in groups:
            if all(abs(r - q) >= plen for q in g):
                g.append(r)
                break
        else:
            groups.append([r])
    return groups


BASE_LENGTHS = [MAX_CHUNK, 16384, 32769, 4096, 20479, 1024, 1025, 16385]


def lengths_directed(plen: int, koff: int) -> list:
    """the geometry and tail-zone lengths, then one chunk of three tiles per group of edge plants"""
    return BASE_LENGTHS + [plen - 1, plen, plen + 31, plen + 32] + [MAX_CHUNK] * len(rel_groups(plen, koff))


def lengths_random(plen: int, rng) -> list:
    pool = [n for n in P.GEOMETRY if n <= MAX_CHUNK] + [MAX_CHUNK, plen - 1, plen, plen + 31, plen + 32]
    n = int(rng.integers(1, 6))
    return [[MAX_CHUNK, 32769, 32768][int(rng.integers(0, 3))]] + [pool[int(i)] for i in rng.integers(0, len(pool), size=n - 1)]


def build_text(info: Info, rng, lengths, alphabet=None, edge_chunks: int = 0) -> Text:
    """Chunks of the given lengths in which the expression occurs.  One witness member w (an all-lower-case one where the
    sets allow) makes the chunk heads and tails, as packing.build_case does: a chunk ends in w[:plen - 1] (its last byte
    would be at L) and the next one begins with w[j:], 0 < j <= koff -- a window inside the first koff bytes of the chunk
    that nothing completes; behind a chunk without a pad the next one carries on (w[:koff] | w[koff:]).  Every third
    chunk, and every one without a pad that nothing carries on from, ends with a whole match instead; of the chunks
    long enough for both, every other one begins with a whole match (the only one, if there is one only).
    Members at the geometry edges B = 16384, 4096, 1024, 16, starting at every r of edge_rels(plen, koff) from the edge:
      edge_chunks > 0 (the directed texts): the last edge_chunks chunks, of three tiles each, carry one group of
        rel_groups each: every r at B and at 2 B for the three large B, nothing left out (`missed` stays empty).  The
        unit edge has two multiples of 16 per r further inside the chunk: 16 and 32 themselves lie inside what begins
        the chunk, and 16 - plen in front of it.
      edge_chunks == 0 (the random texts: 1..5 chunks cannot hold plants that overlap one another around one edge):
        every (B, r) once, at the first multiple of B in any chunk with room; what finds none is listed in `missed`.
    Then at each of the 16 byte alignments a member, a member with its case changed, and the three decoys."""
    f = info.f
    plen, koff = f.plen, f.koff
    w = member(info, rng)
    extra = [w[:plen // 2], w[plen // 2:], w[koff:koff + 8]]
    blocks = [_background(rng, n, alphabet, extra) for n in lengths]
    used = [np.zeros(b.size, dtype=bool) for b in blocks]
    plants, missed = [], []

    def put(c, pos, s, what, margin=1):
        if pos < 0 or pos + len(s) > blocks[c].size or used[c][max(0, pos - margin):pos + len(s) + margin].any():
            return False
        blocks[c][pos:pos + len(s)] = P.u8(s)
        used[c][pos:pos + len(s)] = True
        plants.append((c, pos, what))
        return True

    # heads and tails (the plan of packing.Case: chunk c begins with w[j:] and ends with w[:k])
    plan = [(0, 0)] * len(lengths)
    room = 2 * plen + 4
    crafted = (plen - 1, plen, plen + 31, plen + 32)
    rank = {c: i for i, c in enumerate(c for c, n in enumerate(lengths) if n >= room and n not in crafted)}

    def head_wanted(c):  # every other chunk that has room begins with a head; the others (the only one) with a whole match
        return koff > 0 and c in rank and rank[c] % 2 == 0 and len(rank) > 1
    free, carry = P.GUARD, 0
    for c, n in enumerate(lengths):
        pad = P.round_up16(n) - n
        j = k = 0
        if n == plen - 1:
            put(c, 0, w[:plen - 1], "tail", 0)
            k = plen - 1
        elif n == plen:
            put(c, 0, w, "whole", 0)
        elif n == plen + 31:
            put(c, 31, w, "end", 0)
        elif n == plen + 32:
            put(c, 0, w, "start", 0)
        elif n >= room:
            j = carry if carry else min(koff, free) if head_wanted(c) else 0
            if j:
                put(c, 0, w[j:], "head", 0)
            else:
                put(c, 0, member(info, rng), "start", 0)
            carries = pad == 0 and head_wanted(c + 1)
            if c % 3 == 2 or (pad == 0 and not carries):
                put(c, n - plen, member(info, rng), "end", 0)
            else:
                k = koff if carries else plen - 1
                put(c, n - k, w[:k], "tail", 0)
        plan[c] = (j, k)
        rest = plen - k if k else 0
        carry = k + pad if k and rest > pad else 0
        free = pad - rest if rest <= pad else 0
    big = sorted(range(len(lengths)), key=lambda c: -lengths[c])

    def at_edge(B, rel, s, what):
        for mult in range(1, MAX_CHUNK // B + 1):
            for c in big:
                if put(c, mult * B + rel, s, what):
                    return True
        return False

    if edge_chunks:
        groups = rel_groups(plen, koff)
        assert len(groups) == edge_chunks and all(n == MAX_CHUNK for n in lengths[-edge_chunks:])
        for c, group in zip(range(len(lengths) - edge_chunks, len(lengths)), groups):
            for B in EDGES[:3]:
                for mult in (1, 2):
                    for r in group:
                        if not put(c, mult * B + r, member(info, rng), f"edge {B} {r} x{mult}", 0):
                            missed.append((B, mult, r))
            for r in group:
                units = (u for u in range(4, MAX_CHUNK // UNIT) if u % (P.WAVE_LOAD // UNIT) > 3)
                done = sum(1 for x in (1, 2) if any(put(c, u * UNIT + r, member(info, rng), f"edge {UNIT} {r} x{x}", 0) for u in units))
                if done < 2:
                    missed.append((UNIT, done + 1, r))
    else:
        for B in EDGES:
            for r in edge_rels(plen, koff):
                if not at_edge(B, r, member(info, rng), f"edge {B} {r} x1"):
                    missed.append((B, 1, r))
    order = [int(c) for c in rng.permutation(len(lengths))]
    for r in range(UNIT):
        m = member(info, rng)
        flipped = bytes(x - 32 if 0x61 <= x <= 0x7a and rng.random() < 0.4 else x for x in m)
        for what, s in (("member", m), ("case", flipped), ("decoy outside", decoy_outside(info, rng, m)),
                        ("decoy inside", decoy_inside(info, rng, m)), ("crossover", crossover(info, rng))):
            if s is None:
                continue
            for c in order:
                n = blocks[c].size
                if n < 3 * plen + 64:
                    continue
                first = int(rng.integers(1, max(2, n // UNIT - 3)))
                if any(put(c, ((first + t) % (n // UNIT)) * UNIT + r - koff, s, what) for t in range(0, n // UNIT, 7)):
                    break
        order = order[1:] + order[:1]
    flags = RX | info.flags
    lines = not f.has_newline
    kind = P.Kind(info.expr[:24].decode("latin-1") + f"/{flags:x}", info.expr, flags, w, "cls", lines, lines, bool(f.ascii_only), w)
    stale = corpus.text_block(plen * 131 + koff, 99, 3 * P.GUARD, needle=w, needle_rate=min(0.2, 2.0 / plen), words_per_line=2.0)
    return Text(info, P.Case(kind, blocks, plan, stale), plants, missed)


def directed_text(d: Directed, flags: int = 0) -> Text:
    """the text of a directed expression: a function of the expression alone"""
    expr = FACTOR_OF if d.expr == FACTOR_EXPR else d.expr
    info = info_of(expr, flags)
    rng = np.random.default_rng([len(expr), expr[0], expr[-1], sum(expr)])
    f = info.f
    return build_text(info, rng, lengths_directed(f.plen, f.koff), d.alphabet, edge_chunks=len(rel_groups(f.plen, f.koff)))


def random_texts(seed: int) -> list:
    """the 12..15 expressions of a seed, each with its text (1..5 chunks)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(int(rng.integers(12, 16))):
        info = info_of(rand_long_expr(rng))
        out.append(build_text(info, rng, lengths_random(info.f.plen, rng)))
    return out


# ---- the reader of the new direction
def reader_koff_before(oracle, text: Text, packed, c: int):
    """A model reader that starts koff bytes in front of chunk c (where the match of a window at the chunk's first
    bytes would begin).  -> what it gets wrong: the matches that begin in those bytes and reach into the chunk (None:
    it would refuse: a byte >= 0x80 there and an ASCII-only expression), and how many newlines too many it counts."""
    koff = text.info.f.koff
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    seen = packed.host[o - koff:o + n]
    extra_nl = int((seen[:koff] == 10).sum())
    sp = P.spans(oracle, text.case.kind, seen)
    return (None if sp is None else [s for s in sp if s[0] < koff < s[0] + s[1]]), extra_nl


# ---- everything the two test files run, built once per process
_TEXTS = {}


def all_texts() -> dict:
    """label -> Text: the directed list, then the expressions of the committed seeds (case-sensitive fields)"""
    if not _TEXTS:
        for d in DIRECTED:
            _TEXTS[f"directed {d.expr[:40].decode('latin-1')}"] = directed_text(d)
        for seed in SEEDS:
            for i, t in enumerate(random_texts(seed)):
                _TEXTS[f"seed {seed} #{i}"] = t
    return _TEXTS


def true_starts(oracle, info: Info, blocks) -> list:
    """the oracle's chunk-relative match offsets, chunk by chunk (under ignore_case: of the lowered data)"""
    from xs_oracle import compile_class_sequence
    cs = compile_class_sequence(info.expr, bool(info.flags & IC))
    return [oracle.regex_byte_offsets_match(oracle.lower(b) if info.flags & IC else b, cs).tolist() for b in blocks]


def reached(info: Info, cen: dict) -> list:
    """the paths an expression reaches in its text as the census asks: a true match, a filter-passing decoy that is
    rejected (none exists where the compare is the decision) and, with several alternatives, a rejected crossover"""
    return [p for p in PATHS if cen[p]["true"] and (p == "exact" or cen[p]["decoy"]) and (info.f.nalt == 1 or cen[p]["cross"])]


def kernel_fields(name: str):
    """xsg_scan_kernel_name of a k_scan launch -> (kind, ICASE, ALIGNED)"""
    args = name[name.index("<") + 1:name.index(">")].split(", ")
    return int(args[0]), args[5] == "true", args[6] == "true"
