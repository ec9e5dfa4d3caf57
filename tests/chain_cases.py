"""Inputs for the occurrence-chain walks at their budget, link and chunk edges, and a model of WHICH BRANCH a case takes.

The device code under test decides which raw occurrences the reference's sequential walk (shift = match + plen; line
modes: shift = the byte behind the next '\\n') reports:
  k_greedy_keep, k_greedy_links, k_greedy_jump, k_nlpat_links   x-search_amd/csrc/xsg_list_kernels.hip
  close_chains, decide_keep                                      x-search_amd/csrc/xsg_list.cpp
  k_rx_verify                                                    x-search_amd/csrc/xsg_rx_kernels.hip
  ensure_overlap_check, set_pattern_plain                        x-search_amd/csrc/xsg_count.cpp, xsg_pattern.cpp

`bindings(family)` builds, from fixed seeds, the shards of a family: a Binding is one pattern with its flags and a list
of named chunks (one named case per chunk) that test_gpu_chains.py binds together and compares with the oracle; the
cases listed in `solo` are bound alone as well, because what they are about -- the end of the whole occurrence list inside
an 8-entry fetch, the number of rounds of the closure, a link window clamped at the list's end -- is a property of the
whole binding.

The models below (`greedy_labels`, `closure_rounds`, `nlpat_labels`, `verify_labels`, `overlap_words`) restate the BRANCH
CONDITIONS of that code, not its matching.  They are used only to prove that the cases reach every branch
(test_chain_cases.py) and to name the branch in a failure message; never as an expected value -- every expected value is
the oracle's.

The constants restate the library as of the commit that added this file: kChainBudget and kRxVerifyBudget (4096), the 8
entries k_greedy_keep fetches at a time, the 40 rounds close_chains allows, the three words of the overlap probe,
XSG_MAX_PATTERN (32768), the one candidate per 128 bytes above which prefilter_candidates gives up.  Nothing here can
notice a change of them: whoever changes one updates this file by hand.

What the models say about the code, for the reader of a label:
  * k_greedy_keep tests its budget only between fetches, where j - i is 1, 9, 17, ...: a head decides its first 4096
    followers and gives up at j - i == 4097 -- if the list goes on there (j < M).  So a chain of exactly 4096 followers
    with entries behind it raises the flag with nothing left to close, and one at the very end of the list does not.
  * k_greedy_jump reads marks that other lanes set in the same launch, so the device may need FEWER rounds than
    `closure_rounds` (which squares the links synchronously) says, never more.
"""
import re
from collections import namedtuple

import numpy as np

BUDGET = 4096         # kChainBudget: followers a chain head decides before it hands the chain to the parallel passes
FETCH = 8             # entries k_greedy_keep fetches at a time
ROUND_CAP = 40        # rounds close_chains allows
MAX_WORDS = 3         # words of the overlap probe (one per border); a fourth border clears the list
MAX_PATTERN = 32768   # XSG_MAX_PATTERN: a probe word longer than this clears the list
VERIFY_BUDGET = 4096  # kRxVerifyBudget: bytes k_rx_verify follows one candidate
DENSE_PER = 128       # prefilter_candidates: more than one candidate per 128 bytes and no candidate is verified at all
NOLINK = -1           # kNoLink
EXACT, ICASE, REGEX = 0x1, 0x2, 0x4  # XSG_FLAG_EXACT_TAIL, XSG_FLAG_IGNORE_CASE, XSG_FLAG_REGEX (test_chain_cases.py compares)
NL = 10

FAMILIES = ("budget", "seams", "rounds", "links", "newline", "verify", "probe")

Binding = namedtuple("Binding", "name pattern flags chunks solo")

FILL = np.frombuffer(b"cdefghij", dtype=np.uint8)  # in no pattern of this file


def _fill(rng, n, newlines=True):
    c = FILL[rng.integers(0, len(FILL), size=n)].copy()
    if newlines and n > 8:
        c[rng.integers(0, n, size=max(1, n // 23))] = NL
    return c.tobytes()


def _chunk(*parts):
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------------
# the raw occurrence list
# ---------------------------------------------------------------------------------------------------------------------
def pattern_length(pattern, flags):
    if flags & REGEX:
        m = re.fullmatch(rb"\[ab\]\{(\d+)\}", pattern)
        assert m, "the only class sequence of this file"
        return int(m.group(1))
    return len(pattern)


def tail_zone_begin(length, plen, flags):
    """the bulk scan lists the occurrences that start below this offset; the rest is the end-of-chunk walk's (xsg_tail.h).
    A class sequence and XSG_FLAG_EXACT_TAIL have no such zone."""
    if flags & (REGEX | EXACT) or plen <= 1:
        return length
    return max(0, length - (plen + 31))


def all_occurrences(chunk, pattern, flags):
    """every start of an occurrence, overlapping ones included: bytes.find from each start + 1 (a look-ahead for the class sequence)"""
    d = np.asarray(chunk, dtype=np.uint8).tobytes()
    if flags & REGEX:
        return np.array([m.start() for m in re.finditer(b"(?=" + pattern + b")", d)], dtype=np.int64)
    if flags & ICASE:
        d, pattern = d.lower(), pattern.lower()
    out, p = [], d.find(pattern)
    while p >= 0:
        out.append(p)
        p = d.find(pattern, p + 1)
    return np.array(out, dtype=np.int64)


def raw_occurrences(chunk, pattern, flags):
    occ = all_occurrences(chunk, pattern, flags)
    return occ[occ < tail_zone_begin(len(chunk), pattern_length(pattern, flags), flags)]


def flatten(per_chunk):
    """per-chunk position arrays -> (pos, chunk index) of the whole list, as the emit pass orders it"""
    pos = np.concatenate([np.asarray(p, dtype=np.int64) for p in per_chunk] + [np.zeros(0, dtype=np.int64)])
    chunk = np.concatenate([np.full(len(p), c, dtype=np.int64) for c, p in enumerate(per_chunk)] + [np.zeros(0, dtype=np.int64)])
    return pos, chunk


# ---------------------------------------------------------------------------------------------------------------------
# k_greedy_keep / k_greedy_links / k_greedy_jump
# ---------------------------------------------------------------------------------------------------------------------
def chain_heads(pos, chunk, plen):
    """-> (index of every chain head, its number of followers F)"""
    M = len(pos)
    if M == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    head = np.ones(M, dtype=bool)
    head[1:] = (chunk[1:] != chunk[:-1]) | (pos[1:] - pos[:-1] >= plen)
    h = np.flatnonzero(head)
    return h, np.diff(np.append(h, M)) - 1


def sequential_marks(pos, chunk, plen, budgeted=True):
    """what k_greedy_keep leaves: -> (keep, flag raised, number of chains it left unfinished)"""
    M = len(pos)
    keep = np.zeros(M, dtype=bool)
    heads, F = chain_heads(pos, chunk, plen)
    flag, unfinished = False, 0
    for i, f in zip(heads.tolist(), F.tolist()):
        n = min(f, BUDGET) if budgeted else f
        if budgeted and f >= BUDGET and i + BUDGET + 1 < M:
            flag = True
            unfinished += f > BUDGET
        q = pos[i:i + n + 1]
        k = 0
        while k <= n:
            keep[i + k] = True
            k = int(np.searchsorted(q, q[k] + plen, side="left"))
    return keep, flag, unfinished


def greedy_links(pos, chunk, plen):
    """k_greedy_links: nxt(i) = the first entry of i's chunk at or behind the end of occurrence i -> (J, the window was clamped at M)"""
    M = len(pos)
    key = chunk * (1 << 40) + pos
    lo = np.searchsorted(key, key + plen, side="left")
    ok = lo < M
    ok[ok] = chunk[lo[ok]] == chunk[ok]
    return np.where(ok, lo, NOLINK), np.arange(M) + 1 + plen > M


def closure_rounds(keep, J):
    """close_chains on synchronous rounds: -> (keep closed, rounds that marked something); the device runs one more, which
    marks nothing, and may need fewer (see the module docstring)"""
    keep, J = keep.copy(), J.copy()
    marking = 0
    for _ in range(ROUND_CAP):
        src = np.flatnonzero(keep & (J != NOLINK))
        new = J[src][~keep[J[src]]]
        if new.size == 0:
            break
        keep[new] = True
        marking += 1
        J = np.where(J != NOLINK, J[np.maximum(J, 0)], NOLINK)
    return keep, marking


def greedy_labels(per_chunk, plen):
    """the branches of k_greedy_keep, k_greedy_links and close_chains that a binding with these raw occurrences reaches"""
    pos, chunk = flatten(per_chunk)
    M = len(pos)
    heads, F = chain_heads(pos, chunk, plen)
    out = set()
    over = 0
    for i, f in zip(heads.tolist(), F.tolist()):
        e = i + f + 1  # the first entry behind the chain
        out.add(f"chain ends in fetch slot {f % FETCH}")
        if f == 0:
            out.add("F=0")
        if e == M:
            out.add("ends with the list, " + ("inside a fetch" if f % FETCH else "on a fetch border"))
        elif chunk[e] != chunk[i]:
            out.add("ends with its chunk" + (": only the chunk test says so" if 0 <= pos[e] - pos[e - 1] < plen else ""))
        else:
            out.add("next head exactly plen behind" if pos[e] - pos[e - 1] == plen else "next head more than plen behind")
        if i and chunk[i - 1] != chunk[i] and 0 <= pos[i] - pos[i - 1] < plen:
            out.add("head by the chunk test alone")
        if f and int(np.max(np.diff(pos[i:e]))) == plen - 1:
            out.add("follower at plen - 1")
        if f < BUDGET:
            out.add("under budget" if f < BUDGET - 1 else "F=4095: the last fetch within budget is full")
        elif f == BUDGET:
            out.add("F=4096 with entries behind: flag, nothing left to close" if e < M else "F=4096 at the list's end: no flag")
        elif i + BUDGET + 1 < M:
            over += 1
            out.add("over budget: flag")
            out.add(f"over budget by {f - BUDGET}" if f - BUDGET <= FETCH + 1 else "over budget by more than a fetch")
            if e < M:
                out.add("over budget with entries behind")
    if over > 1:
        out.add("several chains over budget")
    keep0, flag, _ = sequential_marks(pos, chunk, plen)
    if flag:
        J, clamped = greedy_links(pos, chunk, plen)
        live = np.flatnonzero(J != NOLINK)
        for d in np.unique(J[live] - live).tolist():
            out.add(f"link to i+{d}" if d <= 3 else "link inside the window")
            if d == plen:
                out.add("link to i+plen")
        dead = J == NOLINK
        nxt_other = np.zeros(M, dtype=bool)
        key = chunk * (1 << 40) + pos
        lo = np.searchsorted(key, key + plen, side="left")
        nxt_other[lo < M] = True
        if (dead & nxt_other).any():
            out.add("no link: the target lies in the next chunk")
        if (dead & ~nxt_other).any():
            out.add("no link: the search ends at M")
        if (clamped & keep_closed(keep0, J)).any():
            out.add("link window clamped at M")
        out.add(f"closure: {closure_rounds(keep0, J)[1]} marking rounds")
    else:
        out.add("no flag: no closure")
    return out


def keep_closed(keep0, J):
    return closure_rounds(keep0, J)[0]


def greedy_rounds(per_chunk, plen):
    pos, chunk = flatten(per_chunk)
    keep0, flag, _ = sequential_marks(pos, chunk, plen)
    return closure_rounds(keep0, greedy_links(pos, chunk, plen)[0])[1] if flag else None


# ---------------------------------------------------------------------------------------------------------------------
# k_nlpat_links
# ---------------------------------------------------------------------------------------------------------------------
def nlpat_links(chunks, per_chunk, plen):
    """-> (heads, J, per-entry facts) of the line walk of a literal that contains a newline"""
    pos, chunk = flatten(per_chunk)
    M = len(pos)
    J = np.full(M, NOLINK, dtype=np.int64)
    behind_all = np.full(M, -1, dtype=np.int64)
    base = 0
    for c, p in enumerate(per_chunk):
        p = np.asarray(p, dtype=np.int64)
        nlp = np.flatnonzero(np.asarray(chunks[c]) == NL)
        k = np.searchsorted(nlp, p + plen, side="left")
        has = k < len(nlp)
        behind = np.where(has, nlp[np.minimum(k, max(len(nlp) - 1, 0))] if len(nlp) else -1, -1)
        nxt = np.searchsorted(p, behind, side="right")
        link = has & (nxt < len(p))
        J[base:base + len(p)] = np.where(link, base + nxt, NOLINK)
        behind_all[base:base + len(p)] = behind
        base += len(p)
    heads = np.ones(M, dtype=bool)
    heads[1:] = chunk[1:] != chunk[:-1]
    return heads, J, behind_all


def nlpat_labels(chunks, per_chunk, pattern):
    plen = len(pattern)
    pos, chunk = flatten(per_chunk)
    M = len(pos)
    heads, J, behind = nlpat_links(chunks, per_chunk, plen)
    out = {"line start one byte behind the match start" if pattern[0] == NL else "line start behind the last newline before the match"}
    lengths = np.array([len(c) for c in chunks], dtype=np.int64)
    r1 = np.cumsum([len(p) for p in per_chunk])
    if M:
        L = lengths[chunk]
        none, link = behind < 0, J != NOLINK
        rest = ~none & ~link
        for mask, label in ((none, "no newline behind the match"), (link, "link found"),
                            (rest & (r1[chunk] == M), "no occurrence left in the chunk, r1 == M"),
                            (rest & (r1[chunk] < M), "no occurrence left in the chunk, r1 < M"),
                            (~none & (behind == L - 1), "the only newline behind the match is the chunk's last byte"),
                            (pos + plen == L, "occurrence ends with the chunk")):
            if mask.any():
                out.add(label)
    with_raw = [c for c, p in enumerate(per_chunk) if len(p)]
    for a, b in zip(with_raw, with_raw[1:]):
        if b > a + 1 and all(lengths[k] == 0 for k in range(a + 1, b)):
            out.add("empty chunks between two chunks with occurrences")
    if any(len(c) and not (np.asarray(c) == NL).any() for c in chunks):
        out.add("a chunk without any newline")
    out.add(f"closure: {closure_rounds(heads, J)[1]} marking rounds")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# k_rx_verify
# ---------------------------------------------------------------------------------------------------------------------
# expression -> (its three-byte start: a candidate is an occurrence of it; the strings its anchored automaton stays alive on)
VERIFY = {b"xaa+": (b"xaa", re.compile(rb"xa*")), b"xaa+y": (b"xaa", re.compile(rb"xa{2,}y|xa*")),
          b"aaa+b?": (b"aaa", re.compile(rb"a{2,}b|a*"))}


def verify_labels(chunks, expr):
    """per binding: what k_rx_verify does with every candidate -- or that prefilter_candidates never calls it"""
    start, alive = VERIFY[expr]
    cands = [all_occurrences(c, start, 0) for c in chunks]
    total = sum(len(c) for c in chunks)
    if sum(len(p) for p in cands) * DENSE_PER > total:
        return {"candidates too dense: none is verified"}
    out = set()
    n_all, flagged_at = 0, []
    for c, p in zip(chunks, cands):
        d = np.asarray(c, dtype=np.uint8).tobytes()
        L = len(d)
        for p0 in p.tolist():
            stop = p0 + VERIFY_BUDGET if L - p0 > VERIFY_BUDGET else L
            n = alive.match(d, p0, stop).end() - p0
            if p0 + n < stop:
                out.add("dies one byte short of the budget" if n == VERIFY_BUDGET - 1 else "dies early")
            elif stop == L:
                out.add("alive at the chunk's end, exactly the budget: no flag" if n == VERIFY_BUDGET else "alive at the chunk's end: no flag")
            else:
                out.add("alive at the budget, the chunk one byte longer: flag" if L == p0 + VERIFY_BUDGET + 1 else "alive at the budget: flag")
                flagged_at.append(n_all)
            n_all += 1
    if flagged_at and n_all >= 200:
        if flagged_at[0] == 0:
            out.add("the first of hundreds of candidates outruns the budget")
        if flagged_at[-1] == n_all - 1:
            out.add("the last of hundreds of candidates outruns the budget")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the overlap probe
# ---------------------------------------------------------------------------------------------------------------------
def borders(p):
    """the lengths of p's borders (proper prefixes that are suffixes too), longest first"""
    pi = [0] * len(p)
    k = 0
    for i in range(1, len(p)):
        while k and p[i] != p[k]:
            k = pi[k - 1]
        if p[i] == p[k]:
            k += 1
        pi[i] = k
    out, b = [], pi[-1]
    while b:
        out.append(b)
        b = pi[b - 1]
    return out


def overlap_words(p):
    """set_pattern_plain: one word per border, two occurrences plen - b apart spell it; none if the literal cannot be probed"""
    words = []
    for b in borders(p):
        w = p[:len(p) - b] + p
        if len(words) == MAX_WORDS or len(w) > MAX_PATTERN:
            return []
        words.append(w)
    return words


def probe_labels(chunks, pattern):
    nb = len(borders(pattern))
    words = overlap_words(pattern)
    out = {f"{nb} border{'s' if nb != 1 else ''}" if nb <= MAX_WORDS else "more than three borders: not probed"}
    if nb <= MAX_WORDS and not words:
        out.add("a probe word longer than XSG_MAX_PATTERN: not probed")
    for k, w in enumerate(words):
        if any(np.asarray(c, dtype=np.uint8).tobytes().find(w) >= 0 for c in chunks):
            out.add(f"word {k + 1} finds a pair")
            break
    else:
        if words:
            out.add("no word finds a pair: overlap-free")
    return out


def overlaps_in_data(chunks, pattern, flags):
    plen = len(pattern)
    return any((np.diff(all_occurrences(c, pattern, flags)) < plen).any() for c in chunks)


def known_overlap_free(chunks, pattern, flags):
    """what a synchronous count establishes (include/xsg.h, xsg_count): probed, and no two occurrences overlap in a chunk"""
    return bool(overlap_words(pattern)) and not overlaps_in_data(chunks, pattern, flags)


# ---------------------------------------------------------------------------------------------------------------------
# A. budget and fetch
# ---------------------------------------------------------------------------------------------------------------------
F_LIST = (0, 1, 7, 8, 9, 4088, 4095, 4096, 4097, 4098, 4103, 4104, 4105, 8192, 8193)
BUDGET_PATTERNS = ((b"aa", 0), (b"aaa", 0), (b"a" * 9, 0), (b"aba", 0), (b"abab", 0), (b"[ab]{3}", REGEX), (b"a" * 1025, 0))


def chain_text(pattern, flags, nocc, rng):
    """a text whose occurrences of the pattern are ONE chain of nocc entries"""
    if flags & REGEX:
        return np.frombuffer(b"ab", dtype=np.uint8)[rng.integers(0, 2, size=nocc + 2)].tobytes()
    if set(pattern) == {ord("a")}:
        return b"a" * (nocc - 1 + len(pattern))
    if pattern == b"aba":
        return b"ab" * nocc + b"a"
    if pattern == b"abab":
        return b"ab" * (nocc + 1)
    if pattern == b"abcab":
        return b"abc" * nocc + b"ab"
    if pattern == b"abcabca":
        return b"abc" * (nocc + 1) + b"a"
    raise ValueError(pattern)


def glue_head(pattern, a, b):
    """a then b so that b's first occurrence is a head as close behind a's last as the pattern allows: exactly plen for
    `aba` (abaaba), plen + 1 for the others, whose occurrences cannot lie plen apart without one between them"""
    return a + (b"" if pattern == b"aba" else b"c") + b


def _budget():
    out = []
    for k, (pattern, flags) in enumerate(BUDGET_PATTERNS):
        rng = np.random.default_rng(2000 + k)
        plen = pattern_length(pattern, flags)
        tail = lambda: _fill(rng, plen + 40)
        chunks, solo = [], []
        for F in F_LIST:
            u = chain_text(pattern, flags, F + 1, rng)
            six = chain_text(pattern, flags, 6, rng)
            solo.append(len(chunks))
            chunks.append((f"F={F} last", _chunk(_fill(rng, 40 + F % 5), u, tail())))
            chunks.append((f"F={F} then-head", _chunk(_fill(rng, 41 + F % 7), glue_head(pattern, u, six), tail())))
            solo.append(len(chunks))  # (the six further occurrences in the SAME chain: more residues of the fetch, 4094 and 4101 .. 4111 around the budget)
            chunks.append((f"F={F}+6 same-chain", _chunk(_fill(rng, 42 + F % 3), chain_text(pattern, flags, F + 7, rng), tail())))
        parts = [_fill(rng, 50)]
        for n in (5000, 3, 4098, 1, 10, 9000, 2, 4097, 4, 13):
            parts += [chain_text(pattern, flags, n, rng), _fill(rng, 3 + n % 4, newlines=False)]
        solo.append(len(chunks))
        chunks.append(("several over budget, short chains between", _chunk(*parts, tail())))
        out.append(Binding(f"budget {pattern[:12].decode()}{'...' if len(pattern) > 12 else ''}", pattern, flags, chunks, tuple(solo)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# B. chunk seams
# ---------------------------------------------------------------------------------------------------------------------
def _seams():
    out = []
    for k, (pattern, run) in enumerate(((b"aa", lambda n: b"a" * n), (b"aba", lambda n: (b"ab" * n)[:n | 1]))):
        rng = np.random.default_rng(2100 + k)
        plen = len(pattern)
        f = lambda n: _fill(rng, n)
        chunks = [
            ("ends in a run over budget", _chunk(f(60), run(9000))),
            ("begins with a run over budget", _chunk(run(9000), f(60))),
            ("ends in a short run", _chunk(f(50), run(60))),
            ("empty", _chunk()),
            ("begins with a short run, behind an empty chunk", _chunk(run(61), f(50))),
            ("ends in a run of 4200", _chunk(f(30), run(4200 + plen + 31))),
            ("one occurrence", _chunk(f(50), pattern, f(50))),
            ("begins with a run, behind a chunk of one occurrence", _chunk(run(4300), f(70))),
            ("ends in a run of 9", _chunk(f(64), run(9 + plen + 31))),
            ("shorter than the pattern", _chunk(pattern[:plen - 1])),
            ("begins with a run, behind a chunk shorter than the pattern", _chunk(run(9), f(64))),
            ("a run and nothing else, over budget", _chunk(run(6000))),
            ("a run and nothing else", _chunk(run(100))),
            # the last listed occurrence of one chunk and the first of the next less than plen apart by their offsets IN
            # their chunks: only the chunk numbers keep them apart
            ("last occurrence at 10", _chunk(f(10).replace(b"\n", b"c"), pattern, b"c" * 50)),
            ("first occurrence at 10, a run over budget", _chunk(b"c" * 10, run(5000), f(40))),
            ("last occurrence at 5010", _chunk(b"c" * 5010, pattern, b"c" * 60)),
            ("first occurrence at 5011", _chunk(b"c" * 5011, run(300), f(40))),
            ("last occurrence at 305", _chunk(b"c" * 305, pattern, b"c" * 60)),
            ("first occurrence at " + str(305 + plen - 1), _chunk(b"c" * (305 + plen - 1), run(40), f(40))),
        ]
        out.append(Binding(f"seams {pattern.decode()}", pattern, 0, chunks, ()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. rounds of the closure
# ---------------------------------------------------------------------------------------------------------------------
def kept_behind_sizes():
    return sorted({n for k in range(1, 17) for n in (2 ** k - 1, 2 ** k, 2 ** k + 1)})


def _rounds():
    rng = np.random.default_rng(2200)
    chunks = []
    for n in kept_behind_sizes():
        # `aa` on a run: entries 0 .. F, every other one reported; the head decides entries 1 .. 4096, the n reported
        # ones behind are 4098, 4100, .. 4096 + 2n
        F = BUDGET + 2 * n
        chunks.append((f"{n} reported entries behind the budget", _chunk(_fill(rng, 30 + n % 11), b"a" * (F + 2), _fill(rng, 40))))
    return [Binding("rounds aa", b"aa", 0, chunks, tuple(range(len(chunks))))]


# ---------------------------------------------------------------------------------------------------------------------
# D. the link window
# ---------------------------------------------------------------------------------------------------------------------
LINK_PATTERNS = (b"aa", b"aaa", b"a" * 9, b"aba", b"abab", b"abcab", b"abcabca")


def _links():
    out = []
    for k, pattern in enumerate(LINK_PATTERNS):
        rng = np.random.default_rng(2300 + k)
        plen = len(pattern)
        t = lambda n: chain_text(pattern, 0, n, rng)
        f = lambda n: _fill(rng, n)
        lone = b"".join(pattern + _fill(rng, 2 + i % 5, newlines=False) for i in range(12))  # heads without followers: nxt(i) = i + 1
        cut = t(7000)
        chunks = [
            ("over budget in the bulk, lone occurrences around", _chunk(lone, f(20), t(5000), f(9), lone, f(plen + 40))),
            ("over budget, cut by the chunk's end", _chunk(f(33), cut)),
            ("begins with occurrences", _chunk(cut[len(cut) // 2:], f(50))),
            ("over budget, the list's last entries", _chunk(f(20), lone, t(4600 + k), f(plen + 31))),
        ]
        out.append(Binding(f"links {pattern.decode()}", pattern, 0, chunks, (3,)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# E. newline literals
# ---------------------------------------------------------------------------------------------------------------------
# pattern, flags, the line every text repeats
NEWLINE_PATTERNS = ((b"\n", 0, b"a\n"), (b"\n\n", 0, b"\n"), (b"a\n", 0, b"a\n"), (b"\na", 0, b"a\n"), (b"a\na", 0, b"a\n"),
                    (b"\nab\n", 0, b"ab\n"), (b"A\na", ICASE, b"a\nA\n"))


def line_counts():
    return sorted({1, 2, 3} | {n for k in range(2, 17) for n in (2 ** k - 1, 2 ** k, 2 ** k + 1)})


def _newline():
    out = []
    for k, (pattern, flags, line) in enumerate(NEWLINE_PATTERNS):
        rng = np.random.default_rng(2400 + k)
        plen = len(pattern)
        counts = [n for n in line_counts() if not flags or n <= 4097]
        width = line.index(b"\n") + 1  # (the ignore-case text alternates two lines of this width)
        chunks = [(f"{n} lines", _chunk((line * n)[:n * width])) for n in counts]
        solo = list(range(len(chunks)))
        nonl = _fill(rng, 37, newlines=False)
        body = line * 5
        chunks += [
            ("an occurrence ends with the chunk", _chunk(nonl, b"\n", body, nonl, b"\n" if pattern[0] == NL else b"", pattern)),
            ("empty", _chunk()),
            ("empty again", _chunk()),
            ("the only newline behind the match is the last byte", _chunk(nonl, b"\n", body, pattern, nonl * 3, b"\n")),
            ("no newline at all", _chunk(nonl, b"aaaa ab ab", nonl)),
            ("no newline behind the last match", _chunk(nonl, b"\n", body, pattern, nonl * 3)),
            ("lines, the list's last entries", _chunk(line * 40, nonl * 3)),
        ]
        out.append(Binding(f"newline {pattern!r}{'/i' if flags else ''}", pattern, flags, chunks, tuple(solo)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# F. the verify budget
# ---------------------------------------------------------------------------------------------------------------------
RUNS = tuple(range(VERIFY_BUDGET - 4, VERIFY_BUDGET + 3))  # 4092 .. 4098 bytes of `a` behind the x


def _verify_chunks(rng):
    chunks = []
    for n in RUNS:
        head = _chunk(_fill(rng, 90 + n % 13), b"x", b"a" * n)
        chunks.append((f"x a*{n} y", _chunk(head.tobytes(), b"y", _fill(rng, 70))))
        chunks.append((f"x a*{n} blank", _chunk(head.tobytes(), b" ", _fill(rng, 70))))
        chunks.append((f"x a*{n} chunk end", head))
    return chunks


def _verify():
    """`xaa+`, `xaa+y`: the chunks together, a candidate every few thousand bytes; then one long candidate as the first and
    as the last of the candidate list, 250 short ones and a padding chunk beside it (more than one candidate per 128
    bytes of the binding sends the search to the line walks before any is verified).  `aaa+b?`: every `a` of a run is a
    candidate, so each of its cases is bound with padding chunks that hold none -- and once all together, dense."""
    out = []
    for k, expr in enumerate((b"xaa+", b"xaa+y")):
        rng = np.random.default_rng(2500 + k)
        out.append(Binding(f"verify {expr.decode()}", expr, REGEX, _verify_chunks(rng), ()))
        short = b"".join(b"xaa" + b"a" * (i % 5) + (b"y" if i % 3 else b" ") + _fill(rng, 5 + i % 9) for i in range(250))
        long = b"x" + b"a" * 4200 + b"y"
        pad = ("padding", _chunk(_fill(rng, 60_000)))
        out.append(Binding(f"verify {expr.decode()} long candidate first", expr, REGEX,
                           [("a long candidate, then 250 short ones", _chunk(long, _fill(rng, 9), short)), pad], ()))
        out.append(Binding(f"verify {expr.decode()} long candidate last", expr, REGEX,
                           [pad, ("250 short candidates, then a long one", _chunk(short, long))], ()))
    rng = np.random.default_rng(2502)
    chunks = _verify_chunks(rng)
    out.append(Binding("verify aaa+b? dense", b"aaa+b?", REGEX, chunks, ()))
    pad = [("padding", _chunk(_fill(rng, 150_000))) for _ in range(4)]
    for name, c in chunks:
        tailed = _chunk(c.tobytes()[:-71], b"b", c.tobytes()[-70:]) if name.endswith(" y") else c  # (`y` -> `b`: the optional last byte)
        out.append(Binding(f"verify aaa+b? {name}", b"aaa+b?", REGEX, [(name, tailed)] + pad, ()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# G. the overlap probe
# ---------------------------------------------------------------------------------------------------------------------
def long_literal():
    """about 20 000 bytes with the single border `a`: its probe word (39 999 bytes) exceeds XSG_MAX_PATTERN"""
    rng = np.random.default_rng(2600)
    return b"a" + FILL[rng.integers(0, len(FILL), size=19_998)].tobytes() + b"a"


PROBE_LITERALS = (b"aXa", b"abaXaba", b"aaaa", b"aaaaa", b"abacabadabacaba")
PROBE_DATA = ("no pair", "pair in the bulk", "pair in the tail zone", "pair across a seam")


def _probe():
    out = []
    for k, pattern in enumerate(PROBE_LITERALS + (long_literal(),)):
        plen = len(pattern)
        bs = borders(pattern)
        short = pattern[:12].decode() + ("..." if plen > 12 else "")
        for b in (bs if plen < 100 and len(set(pattern)) > 1 else bs[:1]):  # a pair for every border (all the same for a run of `a`)
            pair = pattern[:plen - b] + pattern
            for j, data in enumerate(PROBE_DATA):
                rng = np.random.default_rng(2610 + len(out))
                f = lambda n: _fill(rng, n)
                plain = lambda: _chunk(f(300), pattern, f(200), pattern, f(plen + 150))
                mid = {"no pair": plain(),
                       "pair in the bulk": _chunk(f(300), pattern, f(100), pair, f(plen + 150)),
                       "pair in the tail zone": _chunk(f(300), pattern, f(400), pair, f(5)),
                       "pair across a seam": _chunk(f(300), pattern, f(200), pattern)}[data]
                nxt = _chunk(pair[plen:], f(250), pattern, f(plen + 99)) if data == "pair across a seam" else plain()
                chunks = [("first", plain()), (data, mid), ("next", nxt)]
                out.append(Binding(f"probe {short} border {b}: {data}", pattern, 0, chunks, ()))
    return out


_BUILD = {"budget": _budget, "seams": _seams, "rounds": _rounds, "links": _links, "newline": _newline, "verify": _verify,
          "probe": _probe}
_cache = {}


def bindings(family):
    """-> list of Binding; the same list on every call"""
    if family not in _cache:
        _cache[family] = _BUILD[family]()
    return _cache[family]


def blocks_of(binding):
    return [c for _, c in binding.chunks]
