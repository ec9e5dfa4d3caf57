"""Tightly packed bindings with chosen bytes around every chunk (plain Python, no GPU).

include/xsg.h asks of a binding: offset % 16 == 0, offset + round_up(length, 16) <= capacity, chunks in increasing order.
A caller may therefore lay chunks back to back, and the 0..15 pad bytes of a chunk, like everything around the binding,
may hold anything.  tests/gpu_util.py: upload puts every chunk on a 256-byte boundary into zeroed memory; here the
layout is the tightest the header allows and the surroundings are picked to hurt:

  pack_tight(blocks, fill)   the host buffer (guard band, chunks 16-byte packed, guard band), where d_base lies in it,
                             the exact capacity and the chunk table
  FILLS                      zero (the control), nl, hi, stale, complete: what the guards and the pads hold
  KINDS                      the pattern kinds, each with a witness string it matches
  build_case(kind)           the chunks of a kind (a function of the kind alone, never of the fill) and the plan of
                             witness pieces at their heads and tails that the `complete` fill finishes from outside
  reader_*                   models of kernels that read past a chunk's ends; tests/test_packing.py uses them to prove
                             that a layout really is hostile before a GPU sees it
  pipeline_chunks, reused_buffer, host_sequence
                             the alternating long/short chunks of the file and host-searcher tests, and the device
                             buffer the product reuses from chunk to chunk, simulated
  truth_of                   everything the GPU file compares, from the blocks alone: the existing sources
                             (gpu_util.oracle_*_all_modes, anchor_oracle, match_model, invert_model, context_model);
                             plain_model only picks the source of a kind, as test_gpu_context.plain_model does, and
                             also serves the kinds that have no line tags"""
from collections import namedtuple

import numpy as np

import corpus
import match_model
import xsg
from xs_oracle import UnsupportedRegex

UNIT, WAVE_LOAD, WAVE_SPAN, TILE = 16, 1024, 4096, 16384  # the kernels' geometry (x-search_amd/csrc/xsg_devutil.h)
GUARD = 4096
X, IC, RX = xsg.FLAG_EXACT_TAIL, xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX

GEOMETRY = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 20479, 32768, 32769]
SINGLES = [15, 4097, 16384, 32769]  # also bound alone: a one-chunk shard takes the tile_chunk == nullptr branches
FILLS = ("zero", "nl", "hi", "stale", "complete")
HOSTILE = FILLS[1:]
CONTEXT_PAIRS = ((1, 0), (0, 1), (2, 3))


def round_up16(n: int) -> int:
    return (int(n) + 15) & ~15


def u8(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def _words(n: int, start: int) -> bytes:
    """n bytes of lexicon words separated by blanks, no newline (the long literals)"""
    out, i = b"", start
    while len(out) < n + 1:
        out += corpus.LEXICON[(i * 7 + 3) % len(corpus.LEXICON)] + b" "
        i += 1
    return out[:n - 1] + b"x"  # (never ends in a blank: the last byte is part of a word)


LIT110, LIT1500 = _words(110, 1), _words(1500, 5)

# family: which route toggles apply (lit: the literal kernels; cls: class sequences, same kernels; rx: the automaton)
# lines: the line tags apply; invctx: XSG_FLAG_INVERT / XSG_FLAG_CONTEXT apply (refused when the pattern can match '\n')
# needle: what corpus.text_block plants (default: the witness); ascii_only: '.' or a negated class (non-ASCII data refused)
Kind = namedtuple("Kind", "name pat flags witness family lines invctx ascii_only needle")


def _kind(pat, flags, witness, family, lines=True, invctx=True, ascii_only=False, needle=None):
    name = pat[:12].decode("latin-1").replace("\n", "\\n") + (f"..{len(pat)}" if len(pat) > 12 else "") + f"/{flags:x}"
    return Kind(name, pat, flags, witness, family, lines, invctx, ascii_only, needle or witness)


def _kinds():
    out = []
    lits = [(b"e", {}), (b"he", {}), (b"lock", {}), (b"Sherlock", {}), (b"detective street", {}), (LIT110, {}),
            (LIT1500, {}), (b"that", {"needle": b"thathat"}), (b"aa", {"needle": b"aaaa"}),
            (b"street\nthe", {"invctx": False})]
    for pat, kw in lits:  # each literal with the reference's lossy tail walk and with every occurrence reported
        out += [_kind(pat, 0, pat, "lit", **kw), _kind(pat, X, pat, "lit", **kw)]
    out += [_kind(b"sHERLOCK", IC, b"SHerlock", "lit"), _kind(b"THAT", IC | X, b"That", "lit", needle=b"tHaThat")]
    out += [_kind(b"She[r ]lock", RX, b"She lock", "cls"), _kind(b"t.e", RX, b"the", "cls", ascii_only=True),
            _kind(b"[^a-z]he", RX, b" he", "cls", lines=False, invctx=False, ascii_only=True)]
    out += [_kind(b"colou?r", RX, b"colour", "rx"), _kind(b"\\w+ing", RX, b"walking", "rx"),
            _kind(b"Sher.*mes", RX, b"Sherlock Holmes", "rx", ascii_only=True),
            _kind(b"(?m)^She", RX, b"\nShe", "rx"), _kind(b"(?m)locked$", RX, b"locked\n", "rx"),
            _kind(b"She\\s+lock", RX, b"She\nlock", "rx", lines=False, invctx=False)]
    return out


KINDS = _kinds()
assert len({k.name for k in KINDS}) == len(KINDS)


def plen_of(kind) -> int:
    """the length the tail zone is measured with: the literal's, the witness's for an expression"""
    return len(kind.pat) if not kind.flags & RX else len(kind.witness)


def lengths_of(kind) -> list[int]:
    """every geometry edge and the kind's four tail-zone edges, large and small chunks next to each other"""
    p = plen_of(kind)
    geo = sorted(GEOMETRY)
    mixed = []
    while geo:  # largest, smallest, second largest, ...
        mixed.append(geo.pop())
        if geo:
            mixed.append(geo.pop(0))
    return mixed + [p - 1, p, p + 31, p + 32]


Case = namedtuple("Case", "kind blocks plan stale")  # plan[c] = (j, k): chunk c begins with witness[j:] and ends with witness[:k]


def _text(kind, seed, index, n, terminated):
    rate = 2e-2 if len(kind.needle) <= 16 else 6e-3 if len(kind.needle) <= 110 else 1.5e-3
    if n < 2:
        return u8(kind.witness[:n])
    if terminated:
        return corpus.text_block(seed, index, n, needle=kind.needle, needle_rate=rate, words_per_line=5.0)
    b = corpus.text_block(seed, index, n + 1, needle=kind.needle, needle_rate=rate, words_per_line=5.0)[:n].copy()
    if b[-1] == 10:
        b[-1] = ord("w")
    return b


def build_case(kind) -> Case:
    """The chunks of a kind.  Chunk c holds text with the kind's needle; odd chunks lack the final '\\n'.  The last four
    are the tail-zone edges: witness[:-1], the witness alone, the witness as the last bytes of plen + 31, and as the first
    of plen + 32.  Every other chunk that is long enough ends in witness[:k], k cycling, and begins with the witness
    suffix that the bytes in front of it (a pad, the front guard, or the previous chunk's tail plus its pad) lack: its
    own content either way, so the truth accounts for it, and what the `complete` fill writes around it finishes
    the witness from outside."""
    w, p = kind.witness, plen_of(kind)
    lengths = lengths_of(kind)
    seed = 7000 + KINDS.index(kind)
    blocks = [_text(kind, seed, c, n, terminated=not c & 1) for c, n in enumerate(lengths)]
    crafted = set(range(len(lengths) - 4, len(lengths)))
    c0 = len(lengths) - 4
    full = kind.pat if not kind.flags & RX else w
    blocks[c0] = u8(full[:p - 1])
    blocks[c0 + 1] = u8(full)
    blocks[c0 + 2][31:] = u8(full)
    blocks[c0 + 3][:p] = u8(full)
    plan = [(0, 0)] * len(lengths)
    if full == w and len(w) > 1:
        plan[c0] = (0, len(w) - 1)
    room = 2 * len(w) + 2  # a chunk this long takes a head and a tail without the two meeting
    rests = min(len(w) - 1, 24)  # long witnesses: the rest that follows the tail stays short enough to matter
    t, free, carry = 0, GUARD, 0  # free: bytes in front of the chunk that the fill may use for a witness prefix
    for c, n in enumerate(lengths):
        pad = round_up16(n) - n
        if c in crafted or len(w) < 2:
            free, carry = pad, 0
            continue
        j = k = 0
        keeps_newline = c % 4 == 0  # (a tail would take the final '\\n' of every chunk: these keep theirs)
        if n >= room:
            j = carry if carry else 1 + t % min(free, len(w) - 1) if free else 0
            if j:
                blocks[c][:len(w) - j] = u8(w[j:])
            k = 0 if keeps_newline else len(w) - 1 - t % rests
        elif n > len(w) - 1 - t % rests and len(w) <= 24 and not keeps_newline:
            k = len(w) - 1 - t % rests
        if k:
            blocks[c][n - k:] = u8(w[:k])
        plan[c] = (j, k)
        rest = len(w) - k if k else 0
        carry = k + pad if rest > pad else 0  # the witness does not end inside the pad: the next chunk's head goes on
        free = pad - rest if rest <= pad else 0
        t += 1
    stale = corpus.text_block(seed, 99, 3 * GUARD, needle=kind.needle, needle_rate=min(0.2, 2.0 / len(kind.needle)), words_per_line=2.0)
    return Case(kind, blocks, plan, stale)


def single_case(case: Case, length: int) -> Case:
    """one chunk of the case, bound alone (same bytes, same plan entry)"""
    c = lengths_of(case.kind).index(length)
    return Case(case.kind, [case.blocks[c]], [case.plan[c]], case.stale)


# ---- fills: gap(i, n) -> the n bytes between chunk i - 1 and chunk i (i == 0: the front guard, i == nchunks: the rear)
def make_fill(name: str, case: Case):
    w = case.kind.witness
    if name == "zero":
        return lambda i, n: np.zeros(n, dtype=np.uint8)
    if name == "nl":
        return lambda i, n: np.full(n, 10, dtype=np.uint8)
    if name == "hi":
        return lambda i, n: np.full(n, 0xFF, dtype=np.uint8)
    if name == "stale":
        text = case.stale[:case.stale.size - GUARD].tobytes()
        needles = [m for m in range(len(text)) if text.startswith(case.kind.needle, m)] or [0]
        newlines = [m - 1 for m in range(1, len(text)) if text[m] == 10]

        def stale(i, n):  # what an earlier, longer chunk left in a reused buffer: text with needles and newlines
            # (behind the chunk either a needle at once, or one byte and then a '\n': a pad of two bytes shows it)
            starts = newlines if i & 1 else needles
            at = starts[(i * 7) % len(starts)]
            return case.stale[at:at + n].copy()
        return stale
    assert name == "complete"

    def complete(i, n):
        unit = w if len(w) == 1 else w + b" "
        out = u8((unit * (n // len(unit) + 1))[:n])
        k = case.plan[i - 1][1] if i > 0 else 0
        j = case.plan[i][0] if i < len(case.plan) else 0
        if k:
            cont = u8(w[k:])[:n]
            out[:cont.size] = cont
        if j and not (k and k + n == j):  # (k + n == j: the pad is the middle of a witness that the next chunk's head ends)
            assert j <= n - (len(w) - k if k else 0), (i, n, j, k)
            out[n - j:] = u8(w[:j])
        return out
    return complete


Packed = namedtuple("Packed", "host base capacity offsets lengths")


def pack_tight(blocks, fill, guard=GUARD) -> Packed:
    """-> (host buffer, byte offset of d_base in it, capacity, chunk offsets, chunk lengths).  Chunk k starts at
    sum(round_up16(len_j), j < k); capacity is exactly sum(round_up16(len_j)); `guard` bytes lie in front of d_base and
    behind d_base + capacity, inside the same buffer, so a kernel that reads a little too far reads chosen bytes of
    this allocation.  fill(i, n) paints the guards and the pad [len, round_up16(len)) of every chunk."""
    assert guard % UNIT == 0 and guard > 0
    lengths = np.array([int(b.size) for b in blocks], dtype=np.uint64)
    padded = np.array([round_up16(n) for n in lengths], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.uint64) if len(blocks) else np.zeros(0, dtype=np.uint64)
    cap = int(padded.sum())
    host = np.empty(guard + cap + guard, dtype=np.uint8)
    host[:guard] = fill(0, guard)
    for c, b in enumerate(blocks):
        o, n, pad = guard + int(offsets[c]), int(lengths[c]), int(padded[c] - lengths[c])
        host[o:o + n] = b
        if c + 1 < len(blocks):
            host[o + n:o + n + pad] = fill(c + 1, pad)
    if blocks:  # the last pad and the rear guard are one run of bytes behind the last chunk
        end = guard + int(offsets[-1]) + int(lengths[-1])
        host[end:] = fill(len(blocks), host.size - end)
    else:
        host[guard:] = fill(0, guard)
    return Packed(host, guard, cap, offsets, lengths)


def pack_case(case: Case, fill_name: str) -> Packed:
    return pack_tight(case.blocks, make_fill(fill_name, case))


# ---- naive readers: models of the failure modes, used to prove hostility only
def spans(oracle, kind, data):
    """(start, len) of every match in `data`, or None where the product refuses (an ASCII-only expression on other bytes)"""
    try:
        return match_model.chunk_spans(oracle, data, kind.pat, kind.flags)
    except UnsupportedRegex:
        return None


def reader_past_end(oracle, kind, packed: Packed, c: int):
    """(a) a match runs past the end: the search sees the chunk and the plen + 31 bytes behind it.
    -> (the matches it reports that start inside the chunk, those that start in the chunk's pad)"""
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    seen = packed.host[o:o + n + plen_of(kind) + 31]
    sp = spans(oracle, kind, seen)
    if sp is None:
        return None, None
    return [s for s in sp if s[0] < n], [s for s in sp if n <= s[0] < round_up16(n)]


def reader_before_start(oracle, kind, packed: Packed, c: int):
    """(d) a match begins before the start: the search sees plen + 31 bytes in front of the chunk as well.
    -> the matches that begin there and end inside the chunk (None: refused), and whether the byte in front of the chunk
    denies its first byte the line start that it is"""
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    front = plen_of(kind) + 31
    sp = spans(oracle, kind, packed.host[o - front:o + n])
    straddle = None if sp is None else [s for s in sp if s[0] < front < s[0] + s[1]]
    return straddle, bool(n) and packed.host[o - 1] != 10


def reader_newlines(packed: Packed, c: int):
    """(b) newlines counted and the last line's termination decided over round_up16(len) bytes instead of len
    -> (newline count, last line terminated) as that reader has them, and as they are"""
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    r = round_up16(n)
    naive = (int((packed.host[o:o + r] == 10).sum()), bool(n) and bool((packed.host[o + n - 1:o + r] == 10).any()))
    true = (int((packed.host[o:o + n] == 10).sum()), bool(n) and packed.host[o + n - 1] == 10)
    return naive, true


def reader_non_ascii(packed: Packed, c: int) -> bool:
    """(c) a byte >= 0x80 within 16 bytes behind the end of an all-ASCII chunk"""
    o, n = packed.base + int(packed.offsets[c]), int(packed.lengths[c])
    return bool((packed.host[o:o + n] < 0x80).all()) and bool((packed.host[o + n:o + n + UNIT] >= 0x80).any())


def hostility(oracle, kind, packed: Packed, blocks, max_len=5000) -> dict:
    """-> reader name -> the chunks on which it disagrees with the chunk searched alone.  The searching readers skip
    chunks above max_len (the proof needs one chunk, not all)."""
    out = {"a": [], "pad": [], "b": [], "c": [], "d": [], "d_line": []}
    for c, b in enumerate(blocks):
        nb, tb = reader_newlines(packed, c)
        if nb != tb:
            out["b"].append(c)
        if reader_non_ascii(packed, c):
            out["c"].append(c)
        if b.size > max_len:
            continue
        alone = spans(oracle, kind, b)
        inside, in_pad = reader_past_end(oracle, kind, packed, c)
        if inside != alone:
            out["a"].append(c)
        if in_pad:
            out["pad"].append(c)
        straddle, denied = reader_before_start(oracle, kind, packed, c)
        if straddle is None or straddle:
            out["d"].append(c)
        if denied:
            out["d_line"].append(c)
    return out


# ---- the pipeline: one device buffer reused from chunk to chunk (x-search_amd/csrc/xsg_job.cpp: the device workers,
# and xsg_stage.h: stage, copy exactly `length` bytes and bind capacity = round_up16(length) + 256)
PIPELINE_PATTERNS = [(b"street\nthe", 0, False), (b"that", 0, True), (b"colou?r", RX, True), (b"t.e", RX, True)]  # (.., line tags)
PIPELINE_CHUNK = 4096
PIPELINE_LONG = [12013, 12010, 12007, 12004]  # each ends inside the pad of the next: its '\n' stays behind the next one's end
PIPELINE_SHORT = [4099, 4115, 4131, 4147]
BEHIND = b"the that colour the that colour"  # what a long chunk holds right behind the end of the short one that follows


def _row(i: int, n: int) -> bytes:
    """a '\\n'-terminated line of n bytes"""
    words = [b"that", b"colour", b"color", b"the street", b"tie", b"she said", b"Holmes", b"it was time"]
    body = b" ".join(words[(i + k) % len(words)] for k in range(n // 4 + 2))
    return body[:n - 1] + b"\n"


def _rows_then(i: int, upto: int, total: int, end: bytes) -> bytearray:
    """short rows up to about `upto` bytes, then one row that makes the chunk `total` bytes long and ends in `end`"""
    rows, size = [], 0
    while size < upto:
        rows.append(_row(i * 50 + len(rows), 38 + (len(rows) * 7) % 23))
        size += len(rows[-1])
    for r in range(0, len(rows) - 1, 3):  # `street\\nthe` inside the chunk as well
        rows[r], rows[r + 1] = rows[r][:-8] + b" street\n", b"the " + rows[r + 1][4:]
    assert size < PIPELINE_CHUNK - 1 and total - size > len(end) + 8
    last = _row(i + 3, total - size)
    return bytearray(b"".join(rows) + last[:len(last) - len(end)] + end)


def pipeline_chunks() -> list[bytes]:
    """The chunks of the pipeline file as xsg.plan_chunks cuts it at chunk_bytes = 4096 (a chunk ends behind the first
    '\\n' at or after its 4096th byte, so a chunk holds no '\\n' from there on but its last byte): long ones of ~12 KB
    -- short rows, then one row of 8 KB across the mark -- and short ones of ~4.1 KB, alternating.
    What the reused buffer then holds behind a chunk's end:
      behind a short chunk, which ends in `ththat street\\n`, the long one's BEHIND: `the` finishes `street\\nthe`, the
        words start matches inside the 13 pad bytes, and the text moves the reference's lossy tail zone off `ththat`;
      behind the last chunk, which has no final newline and ends in `colo`, the long one's `ur`;
      behind a long chunk, the final '\\n' of the long chunk before it, three bytes on: a newline in the pad."""
    chunks = []
    for i, (ln, sn) in enumerate(zip(PIPELINE_LONG, PIPELINE_SHORT)):
        last = i + 1 == len(PIPELINE_SHORT)
        short = _rows_then(i, 4030, sn, b"colo" if last else b" ththat street\n")
        long_chunk = _rows_then(10 + i, 4000, ln, b"\n")
        behind = b"ur " + BEHIND if last else BEHIND
        long_chunk[sn:sn + len(behind)] = behind
        assert long_chunk.find(b"\n", PIPELINE_CHUNK - 1) + 1 == len(long_chunk) == ln
        assert len(short) == sn and (last or short.find(b"\n", PIPELINE_CHUNK - 1) + 1 == sn)
        chunks += [bytes(long_chunk), bytes(short)]
    return chunks


def reused_buffer(chunks) -> list[np.ndarray]:
    """the device buffer when chunk k is searched: buf[:len_k] = chunk_k, in chunk order -> one snapshot per chunk"""
    buf = np.zeros(max(len(c) for c in chunks) + 256 + UNIT, dtype=np.uint8)
    out = []
    for c in chunks:
        buf[:len(c)] = u8(c)
        out.append(buf.copy())
    return out


def as_packed(snapshot: np.ndarray, length: int, guard: int = 64) -> Packed:
    """a snapshot of the reused buffer as a one-chunk Packed (zeros in front of it), for the readers"""
    host = np.concatenate([np.zeros(guard, dtype=np.uint8), snapshot])
    return Packed(host, guard, round_up16(length), np.zeros(1, dtype=np.uint64), np.array([length], dtype=np.uint64))


def host_sequence(kind, pairs: int = 4) -> list[np.ndarray]:
    """Chunks for one host searcher with a single slot, long and short alternating.  Short chunk i ends in witness[:k]
    (k cycling); the long chunk before it holds at that very offset the witness's rest -- or, every other time, a '\\n'
    and then the witness -- so that it lies behind the short chunk's last byte when that is searched.  For an ASCII-only
    expression the long chunk holds a non-ASCII byte there instead: the long chunk is refused, the short one is not."""
    w, out = kind.witness, []
    seed = 9000 + KINDS.index(kind)
    for i in range(pairs):
        n = 3000 + 37 * i + (5 if i & 1 else 0)
        short = _text(kind, seed, 2 * i, n, terminated=False)
        k = 1 + i % (len(w) - 1) if len(w) > 1 else 0
        if k:
            short[n - k:] = u8(w[:k])
        long_chunk = _text(kind, seed, 2 * i + 1, 9000 + 1111 * i, terminated=True)
        behind = (b"\n" + w if i & 1 else w[k:] + b" " + w) + b"\n" + w
        if kind.ascii_only:
            behind = b"\xc3\xa9" + behind
        long_chunk[n:n + len(behind)] = u8(behind)
        out += [long_chunk, short]
    return out


def plain_model(oracle, kind, blocks, go=None, lb=None) -> dict:
    """the oracle's dict of a kind (tests/gpu_util.py, tests/anchor_oracle.py); a kind without line tags has no line keys"""
    from gpu_util import oracle_all_modes, oracle_regex_all_modes
    import anchor_oracle
    icase = bool(kind.flags & IC)
    if not kind.flags & RX:
        return oracle_all_modes(oracle, blocks, kind.pat, exact=bool(kind.flags & X), global_offsets=go, line_bases=lb, ignore_case=icase)
    if kind.pat.startswith(b"(?m)"):
        return anchor_oracle.all_modes(blocks, kind.pat, icase, global_offsets=go, line_bases=lb)
    want, with_lines = oracle_regex_all_modes(oracle, blocks, kind.pat, icase, global_offsets=go, line_bases=lb)
    assert with_lines == kind.lines, kind.name
    return want


Truth = namedtuple("Truth", "plain matches invert context edges")


def truth_of(oracle, kind, blocks, go=None, lb=None) -> Truth:
    """everything tests/test_gpu_packed.py compares, from the blocks alone: the oracle's dict, XSG_MATCHES (strings,
    offsets, lengths), and where the kind takes them the XSG_FLAG_INVERT dict and, per (B, A) of CONTEXT_PAIRS, the
    XSG_FLAG_CONTEXT dict and the edges"""
    import context_model
    import invert_model
    plain = plain_model(oracle, kind, blocks, go, lb)
    matches = match_model.matches(oracle, blocks, kind.pat, kind.flags, go)
    assert matches[1] == plain["match_byte_offsets"]
    if not kind.invctx:
        return Truth(plain, matches, None, {}, {})
    invert = invert_model.invert_all_modes(plain, blocks, go, lb)
    context = {p: context_model.context_all_modes(plain, blocks, p[0], p[1], go, lb) for p in CONTEXT_PAIRS}
    edges = {p: context_model.edges(plain, blocks, p[0], p[1], go) for p in CONTEXT_PAIRS}
    return Truth(plain, matches, invert, context, edges)


def offsets_and_bases(blocks):
    """-> (global offsets, line bases as the models take them, line bases as the binding takes them): every odd chunk
    lies far away in the file and names its line base; every even one keeps the running offset and XSG_LINE_BASE_AUTO,
    which stands for the newlines of all chunks in front of it"""
    n = len(blocks)
    go, lb, lb_bind = [], [], []
    at = nl = 0
    for i, b in enumerate(blocks):
        odd = bool(i & 1)
        go.append((1 << 33) + 10_000_000 * (n - i) + 13 if odd else at)
        lb.append(1000 * i + 7 if odd else nl)
        lb_bind.append(1000 * i + 7 if odd else xsg.LINE_BASE_AUTO)
        at += int(b.size)
        nl += int((b == 10).sum())
    return go, lb, lb_bind
