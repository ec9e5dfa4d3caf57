"""Inputs for k_rx_count (x-search_amd/csrc/xsg_rx_kernels.hip) at its span, look-ahead and chunk-end edges, and a
model of WHICH PATH a span takes there.

`cases(family)` builds one chunk per case, from fixed seeds; the GPU tests (test_gpu_rx_spans.py) bind a family's
chunks as one shard and compare every result with the oracle.  `span_paths(chunk, triggers)` restates the kernel's
branch conditions -- not its matching -- and labels every 4 KiB span of a chunk; it is used ONLY to prove that the
cases reach every branch (test_rx_span_cases.py) and to name the branch in a failure message, never as an expected
value.

The constants and `span_paths` restate the kernel as of the commit that added this file: kRxSpan (4 KiB, one wave),
the 256 bytes of look-ahead (one dword per lane), the 64 raw look-ahead bytes copied to LDS for the staged path, the
64-byte segments, the 16 KiB tile.  Nothing here can notice a change of that geometry: whoever changes kRxSpan, the
look-ahead width or the LDS look-ahead copy updates S, A, LDS_LA and `span_paths` by hand.
"""
import numpy as np

S = 4096      # kRxSpan: the bytes of one wave
A = 256       # the look-ahead behind a span, lane l holds dword l
LDS_LA = 64   # the raw look-ahead bytes the staged path keeps in LDS
SEG = 64      # kRxSeg: a lane's segment of a staged span
T = 16384     # kRxTile: four spans
UNIT = 16     # one lane's load
SPANS = (0, 1, 3, 4)  # the span under test: 0 opens the chunk, 3 -> 4 is a span border that is a tile border too

FAMILIES = ("look-ahead", "chunk-end", "segments", "newlines")

# no trigger of any expression of the sweep with 1..4 trigger values (S s H h W M), none of A-F, no '\n'
FILL = np.frombuffer(b"ijklnopqrtuvxyz ,.-01", dtype=np.uint8)
# what is planted: a line of all expressions (four of seven), its lower-case form (ignore-case only), a third trigger
# value, and a decoy that holds trigger bytes and no match
NEEDLES = (b"Sherlock Holmes", b"Sherlock Holmes", b"sherlock holmes", b"Sherlock Holmes", b"Watsonn Holmes",
           b"Sherlock Holmes", b"Sherlocc Holmez")

E_LIST = tuple(range(0, 10)) + (15, 16, 17) + tuple(range(62, 67)) + tuple(range(251, 258)) + (300, S - 1, S, S + 300)
R_LIST = tuple(range(-17, 18)) + tuple(range(239, 274)) + (1 - S,)

NL = 10

# (expression, ignore_case, trigger class): the number of trigger byte values k_rx_count tests a span for (1..4),
# "many" (5 or more: trigger jumps, but every span is staged), "no-skip" (>= 9 common lower-case starts: no jumps
# either), "anchored" ((?m) forms: xsg_regex_dfa_info has no forward table for them, results only)
EXPRESSIONS = (
    (b"Sher.*mes", False, 1), (b"Sherlocks?", False, 1), (b"S[a-z]{3,9}k", False, 1),
    (b"Sherlock|Holmes", False, 2), (b"Sher.*?k|Holmes", False, 2),
    (b"S[a-z]|Holmes", False, 2),  # a match of two bytes: the only kind that fit below a '\n' in its own dword
    (b"Sherlock|Holmes|Watson+", False, 3),
    (b"sherlock|holmes", True, 4), (b"[SHWM]\\w+ock", False, 4),
    (b"[A-F]\\w+ock|Holmes", False, "many"),
    (b"\\w+ock", False, "no-skip"),
    (b"(?m)Holmes$", False, "anchored"), (b"(?m)Sher.*mes$", False, "anchored"), (b"(?m)^Sher.*mes", False, "anchored"),
)


def _fill(rng, n):
    return FILL[rng.integers(0, len(FILL), size=n)].copy()


def _put(c, pos, w):
    """w at pos, cut at the chunk's end; False (nothing written) if it would start in front of the chunk"""
    if pos < 0:
        return False
    w = np.frombuffer(w, dtype=np.uint8)[:max(0, c.size - pos)]
    c[pos:pos + w.size] = w
    return True


def _earlier_spans(c, rng, k, idx):
    """spans in front of the one under test: every other one holds a '\\n' (not as its last byte)"""
    for j in range(k):
        if (idx + j) % 2:
            c[j * S + int(rng.integers(1, S - 2))] = NL


PLACEMENTS = ("none", "inside", "ends-at-nl", "next-line", "dword-below", "dword-above", "straddle-span",
              "straddle-lds", "straddle-lds-staged", "beyond")
STARTS = ("first", "mid", "last")


def _look_ahead():
    """a line starts in span k and ends at (k+1)S + e; a needle somewhere around that look-ahead"""
    rng = np.random.default_rng(1001)
    out, idx = [], 0
    for k in SPANS:
        send = (k + 1) * S
        for e in E_LIST:
            for place in PLACEMENTS:
                idx += 1
                nl = send + e
                w = NEEDLES[idx % len(NEEDLES)]
                n = len(w)
                start = STARTS[(idx + idx // len(PLACEMENTS)) % 3]
                c = _fill(rng, nl + 1 + 300 + idx % 7)
                c[-1] = NL
                c[nl] = NL
                _earlier_spans(c, rng, k, idx)
                if start == "first" and k:
                    c[k * S - 1] = NL
                elif start == "mid":
                    c[k * S + 1000 + idx % 2000] = NL
                elif start == "last":
                    c[send - 2] = NL
                if place == "inside":
                    if e < n + 2:
                        continue
                    _put(c, send + 1 + (idx % (e - n - 1)), w)
                elif place == "ends-at-nl":
                    _put(c, nl - n, w)  # (e < n: it straddles the span's end, and the span is staged)
                elif place == "next-line":
                    _put(c, nl + 1, w)
                elif place == "dword-below":  # the needle's head, 1..3 bytes, below the '\n' in its aligned dword
                    if nl % 4 == 0:
                        continue
                    _put(c, nl - nl % 4, w[:nl % 4])
                elif place == "dword-above":  # the next line's needle begins in the dword of the '\n'
                    if nl % 4 == 3:
                        continue
                    _put(c, nl + 1, w)
                elif place == "straddle-span":  # byte i of the needle is the first byte behind the span
                    i = max(1 + idx % (n - 1), n - e)
                    if i > n - 1:
                        continue
                    _put(c, send - i, w)
                elif place in ("straddle-lds", "straddle-lds-staged"):  # ... behind the LDS copy of the look-ahead
                    i = 1 + idx % (n - 1)
                    if send + LDS_LA - i + n > nl:
                        continue
                    _put(c, send + LDS_LA - i, w)
                    if place == "straddle-lds-staged":  # a lone trigger in the span's last byte: the span is staged, and
                        c[send - 1] = ord("S")          # its line is followed through the LDS copy, then global memory
                elif place == "beyond":  # behind the look-ahead, in a line with no earlier '\n'
                    if send + A + 4 + n > nl:
                        continue
                    _put(c, send + A + 4 + idx % (nl - n - send - A - 3), w)
                out.append((f"la k={k} e={e} start={start} needle={place}/{w.decode()}", c))
    return out


SHAPES = ("mid", "mid", "last-is-nl", "no-start")
ENDS = ("at-L", "at-L-1", "cut", "none")


def _chunk_end():
    """the chunk ends at (k+1)S + r; the last line has no '\\n' (or the '\\n' is the last byte); a needle at the end"""
    rng = np.random.default_rng(1002)
    out, idx = [], 0
    for k in SPANS:
        for r in R_LIST:
            L = (k + 1) * S + r
            for v in range(5):
                idx += 1
                final_nl = v == 4
                end = ENDS[idx % 4] if final_nl else ENDS[v]
                shape = SHAPES[idx % 4]
                w = NEEDLES[(idx // 5 + v) % len(NEEDLES)]
                n = len(w)
                c = _fill(rng, L)
                _earlier_spans(c, rng, k, idx)
                body = L - 1 if final_nl else L  # the bytes in front of a final '\n'
                if L > k * S + 600:  # the span under test, where it is long enough to be shaped
                    if shape == "mid":
                        c[k * S + 100 + idx % 400] = NL
                    elif shape == "last-is-nl" and r > 0:
                        c[(k + 1) * S - 1] = NL
                if final_nl:
                    c[L - 1] = NL
                if end == "at-L":
                    _put(c, body - n, w)
                elif end == "at-L-1":
                    _put(c, body - 1 - n, w)
                elif end == "cut":  # head present, tail missing
                    cut = 1 + idx % (n - 1)
                    _put(c, body - cut, w[:cut])
                out.append((f"ce k={k} r={r} L={L} span={shape} needle={end}/{w.decode()}" + (" final-nl" if final_nl else ""), c))
    return out


def _segments():
    """dense text: a trigger in every span, so every span is staged; line starts around segment and span borders"""
    rng = np.random.default_rng(1003)
    out, idx = [], 0
    for k in SPANS:
        for border, bname in ((k * S + 17 * SEG, "segment"), (k * S, "span")):
            for d in range(-4, 5):
                for variant in ("at-start", "crossing", "empty-line"):
                    idx += 1
                    p = border + d  # the line's first byte
                    if p < 0 or (variant == "empty-line" and p < 2):
                        continue
                    w = NEEDLES[idx % len(NEEDLES)]
                    n = len(w)
                    c = _fill(rng, (k + 1) * S + 600 + idx % 50)
                    for j in range(0, c.size - 200, 190):  # decoy triggers, at least one in every span
                        c[j + int(rng.integers(0, 190))] = (ord("S"), ord("H"))[j // 190 % 2]
                    for j in range(0, c.size - 1500, 1400):
                        c[j + int(rng.integers(0, 1400))] = NL
                    c[-1] = NL
                    if p:
                        c[p - 1] = NL
                    if variant == "empty-line":
                        c[p - 2] = NL  # "\n\n" in front of p: an empty line
                    nxt = (p // SEG + 1) * SEG  # the next segment border
                    at = max(p, nxt - 1 - idx % (n - 1)) if variant == "crossing" else p
                    _put(c, at, w)
                    c[at + n if idx % 2 else nxt + 40] = NL  # (every other needle ends its line)
                    out.append((f"seg k={k} {bname}-border{d:+d} {variant}/{w.decode()}", c))
    return out


def _newlines():
    """what WITH_NEWLINES counts: only '\\n', no '\\n', '\\n' at the end and at every byte of the last 16-byte unit"""
    rng = np.random.default_rng(1004)
    kinds = ["only-nl", "no-nl", "nl-at-L-1", "nl-at-L-2"] + [f"nl-in-last-unit+{i}" for i in range(UNIT)]
    out, idx = [], 0
    for k in SPANS:
        for r in R_LIST:
            L = (k + 1) * S + r
            for rep in range(3):
                idx += 1
                kind = kinds[(idx * 7 + rep) % len(kinds)]
                w = NEEDLES[idx % len(NEEDLES)]
                if kind == "only-nl":
                    c = np.full(L, NL, dtype=np.uint8)
                else:
                    c = _fill(rng, L)
                    if idx % 2 and L > 3 * len(w):
                        _put(c, int(rng.integers(0, L - 2 * len(w))), w)
                    if kind == "nl-at-L-1":
                        c[L - 1] = NL
                    elif kind == "nl-at-L-2" and L >= 2:
                        c[L - 2] = NL
                    elif kind.startswith("nl-in-last-unit"):
                        q = (L - 1) // UNIT * UNIT + int(kind.split("+")[1])
                        if q < L:
                            c[q] = NL
                out.append((f"nl k={k} r={r} L={L} {kind}/{w.decode()}", c))
    return out


_BUILD = {"look-ahead": _look_ahead, "chunk-end": _chunk_end, "segments": _segments, "newlines": _newlines}
_cache = {}


def cases(family):
    """-> list of (name, np.uint8 chunk); the same list on every call"""
    if family not in _cache:
        _cache[family] = _BUILD[family]()
    return _cache[family]


def triggers(info, fwd):
    """the trigger byte values of an expression from xsg.regex_dfa's (info, fwd): a byte that moves the forward
    automaton out of its start state (set_dfa_pattern's lambda, xsg_pattern.cpp), '\\n' left out as the kernel's
    rx_trig4 leaves it out"""
    start = int(info.fwd_start)
    row = start * int(info.ncls)
    return bytes(b for b in range(256) if b != NL and int(fwd[start][info.class_of[b]]) != row)


def span_paths(chunk, trig):
    """one label per 4 KiB span of the chunk, '<inner|clamped> <path>': the branches of k_rx_count in the order it
    takes them.  `trig`: the expression's trigger bytes; none or more than four and every span is staged."""
    c = np.asarray(chunk, dtype=np.uint8)
    L = int(c.size)
    quick = 1 <= len(trig) <= 4
    is_trig = np.zeros(256, dtype=bool)
    is_trig[list(trig)] = True
    tmask = is_trig[c]
    nlmask = c == NL
    out = []
    for soff in range(0, L, S):
        send = soff + S
        geo = "inner" if send + A <= L else "clamped"
        if not quick or tmask[soff:send].any():
            path = "staged"
        elif send >= L:
            path = "quiet-ends-chunk"
        elif nlmask[send - 1]:
            path = "quiet-last-is-nl"
        elif not (nlmask[soff:send].any() or soff == 0 or nlmask[soff - 1]):
            path = "quiet-no-start"
        else:
            la_nl = nlmask[send:send + A]
            la_tg = tmask[send:send + A]
            # bytes at or beyond L read as '\n'
            first_nl = int(np.argmax(la_nl)) if la_nl.any() else (la_nl.size if la_nl.size < A else -1)
            if first_nl < 0:
                path = "quiet-walk-long"
            elif la_tg[:first_nl].any():
                path = "quiet-walk-trigger"
            else:
                path = "quiet-settled"
        out.append(f"{geo} {path}")
    return out


def walked_line(chunk, soff):
    """[begin, end) of what a quiet span's walk covers: from the span's end to the line's '\\n' or the chunk's end"""
    c = np.asarray(chunk, dtype=np.uint8)
    send = soff + S
    nl = np.flatnonzero(c[send:] == NL)
    return send, (send + int(nl[0])) if nl.size else int(c.size)
