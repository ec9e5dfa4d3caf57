"""The occurrence-chain walks at their budget, link and chunk edges: k_greedy_keep, k_greedy_links / k_greedy_jump under
close_chains, k_nlpat_links (x-search_amd/csrc/xsg_list_kernels.hip, xsg_list.cpp), k_rx_verify (xsg_rx_kernels.hip) and
the overlap probe (ensure_overlap_check, xsg_count.cpp).  The shards come from chain_cases.py, whose coverage of the
branches test_chain_cases.py proves without a GPU; every expected value is the oracle's, chunk by chunk.  A binding's
chunks are bound together and every tag, xsg_count_chunks, the stream-ordered counts and XSG_MATCHES are compared; the
cases that are about the END of the occurrence list or the number of closure rounds are then bound alone.  When a result
differs the chunks are bound one at a time and the assertion names the first failing case and the branches the model
says it takes: this file exists to say WHICH edge broke.  Counts are compared before lists, for the reason
test_gpu_rx_spans.py gives: the list passes run only behind counts that are right.  No timing assertions.

What the sweep was seen to catch: each entry a one-line change in a scratch build, this file run once, and the first case
it named.
  k_greedy_keep: `p[u] >= last + plen` -> `>`
      test_budget[aa]: [F=0 then-head] count_matches 3 for 4 (the six occurrences behind the head: 0, 3 kept for 0, 2, 4)
  close_chains stops after 8 rounds
      test_budget[aa]: [F=8192 last], which needs 12 marking rounds: count_matches 2304 for 4097 (2049 from the walk, 255 from
      eight rounds); test_rounds holds the cases of 9 .. 17 rounds one by one
  k_nlpat_links: `m_pos[mid] > behind` -> `>=`
      test_newline[b'\n']: [2 lines] count_lines 2 for 1 (the link goes to the occurrence that IS the newline)
  the probe's word limit 3 -> 2, the list not cleared
      test_probe[aaaaa border 4: no pair]: xsg_count_chunks_async served a literal of four borders, which is never probed;
      with that case deselected, test_probe[abacabadabac... border 1: pair in the bulk]: count_matches 7 for 6 -- only the
      third word spells that pair
  kRxVerifyBudget 4096 -> 4095, the line with the `q < ch.length` test removed (no candidate ever voids the pass)
      test_verify[1-xaa+]: [x a*4095 y] matches (90, 4095) for (90, 4096)
Four changes this file does not notice, because they change no result -- run all the same, and the whole file passed:
  kRxVerifyBudget 4096 -> 4095 with only `q < ch.length` taken out of the flag's condition: more candidates void the pass
      (one byte earlier, and at a chunk's end), the host redoes those searches with the line walks, and the results are the
      same by either route -- which test_verify asserts with XSG_RX_PRE=0.
  the budget test `j - i > kChainBudget` -> `>=`: it is made between fetches of 8, where j - i is 1, 9, .. 4089, 4097 and
      never 4096; both forms give up at 4097.
  the chain-end test `p[u] - prev >= plen` -> `> plen`: the walker then runs on through a head that lies exactly plen
      behind -- and decides it and its followers as that head's own lane does (`p[u] >= last + plen` holds there, since
      last <= prev), writing the same marks; with the budget it only gives up earlier, and the closure finishes the rest.
  the link window `i + 1 + plen` -> `i + plen`: occurrences are distinct offsets, so nxt(i) <= i + plen, and a lower bound
      that finds nothing below `hi` returns `hi`: the answer i + plen is found with either bound.
"""
import pytest

import chain_cases as C
import match_model
import xsg
from gpu_util import GpuSearch, oracle_all_modes, oracle_regex_all_modes

pytestmark = pytest.mark.gpu

LIST_KEYS = ("match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "lines_offsets")
SUM_KEYS = ("count_matches", "count_lines", "newlines", "bytes")


@pytest.fixture(scope="module")
def gs():
    return GpuSearch()


class Async:
    """the stream-ordered counts: device words for the counters, the status and a count per chunk"""

    def __init__(self):
        import torch
        self.torch = torch
        self.counters = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device="cuda:0")
        self.status = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def count(self, shard, mode):
        """-> (the mode's counter, status)"""
        self.counters.fill_(-1)
        self.status.fill_(-1)
        shard.count_async_status(mode, 0, self.counters.data_ptr(), self.status.data_ptr())
        self.torch.cuda.synchronize()
        return int(self.counters[xsg.CTR_MATCHES if mode == xsg.COUNT_MATCHES else xsg.CTR_LINES].item()), int(self.status.item())

    def count_chunks(self, shard, mode):
        """-> (counts per chunk, the mode's counter, status)"""
        per = self.torch.full((max(shard.nchunks, 1),), -1, dtype=self.torch.int64, device="cuda:0")
        self.counters.fill_(-1)
        self.status.fill_(-1)
        shard.count_chunks_async(mode, 0, per.data_ptr(), 0, shard.nchunks, self.counters.data_ptr(), self.status.data_ptr())
        self.torch.cuda.synchronize()
        return per.tolist()[:shard.nchunks], int(self.counters[xsg.CTR_MATCHES].item()), int(self.status.item())


@pytest.fixture(scope="module")
def stream_counts():
    return Async()


def modes_of(b):
    """a literal in both tail modes; an expression has one"""
    return (b.flags,) if b.flags & C.REGEX else (b.flags, b.flags | C.EXACT)


_chunk_want = {}


def chunk_want(oracle, blk, pattern, flags):
    """the oracle's dict for one chunk alone (offsets from 0, line indices from 0), computed once per chunk and pattern"""
    key = (id(blk), pattern, flags)
    if key not in _chunk_want:
        if flags & C.REGEX:
            w, with_lines = oracle_regex_all_modes(oracle, [blk], pattern, bool(flags & C.ICASE))
            assert with_lines
        else:
            w = oracle_all_modes(oracle, [blk], pattern, exact=bool(flags & C.EXACT), ignore_case=bool(flags & C.ICASE))
        w["matches"] = match_model.matches(oracle, [blk], pattern, flags)
        _chunk_want[key] = (blk, w)  # (the chunk is kept alive with its id)
    return _chunk_want[key][1]


def expect(oracle, blocks, pattern, flags):
    """the binding's expected values from its chunks': offsets move by the bytes, line indices by the newlines in front"""
    want = {k: 0 for k in SUM_KEYS}
    want.update({k: [] for k in LIST_KEYS})
    want.update({"chunk_matches": [], "chunk_lines": [], "matches": ([], [], [])})
    goff = nl = 0
    for blk in blocks:
        w = chunk_want(oracle, blk, pattern, flags)
        for k in SUM_KEYS:
            want[k] += w[k]
        for k in ("match_byte_offsets", "line_byte_offsets", "lines_offsets"):
            want[k] += [x + goff for x in w[k]]
        want["line_indices"] += [x + nl for x in w["line_indices"]]
        want["lines"] += w["lines"]
        want["chunk_matches"].append(w["count_matches"])
        want["chunk_lines"].append(w["count_lines"])
        s, o, n = w["matches"]
        want["matches"][0].extend(s)
        want["matches"][1].extend(x + goff for x in o)
        want["matches"][2].extend(n)
        goff += w["bytes"]
        nl += w["newlines"]
    literal_nl = not flags & C.REGEX and b"\n" in pattern
    want["count_matches_plain"] = want["count_matches"]
    want["chunks_totals"] = (want["count_matches"], want["count_lines"])
    want["async_matches"] = (want["count_matches"], 0)
    if not literal_nl:  # (the line walk of a literal that holds a newline is a chain: the stream-ordered entry point refuses it)
        want["async_lines"] = (want["count_lines"], 0)
    return want


COUNT_KEYS = ("count_matches", "newlines", "bytes", "count_matches_plain", "count_lines", "chunk_matches", "chunk_lines",
              "chunks_totals", "async_matches", "async_lines")


def observe_counts(gs, stream_counts, pattern, flags, want, light=False):
    """the synchronous counts first (they raise the flag and close the chains), then the counts per chunk, then the
    stream-ordered ones, where the same chain is walked without a budget"""
    gs.ctx.set_pattern(pattern, flags)
    s = gs.shard
    c = s.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
    got = {"count_matches": int(c[xsg.CTR_MATCHES]), "newlines": int(c[xsg.CTR_NEWLINES]), "bytes": int(c[xsg.CTR_BYTES]),
           "count_matches_plain": int(s.count(xsg.COUNT_MATCHES)[xsg.CTR_MATCHES]),
           "count_lines": int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES])}
    if not light:
        cm, _, tm = s.count_chunks(xsg.COUNT_MATCHES)
        cl, _, tl = s.count_chunks(xsg.COUNT_LINES)
        got.update({"chunk_matches": cm.tolist(), "chunk_lines": cl.tolist(), "chunks_totals": (int(tm[xsg.CTR_MATCHES]), int(tl[xsg.CTR_LINES]))})
    got["async_matches"] = stream_counts.count(s, xsg.COUNT_MATCHES)
    if "async_lines" in want:
        got["async_lines"] = stream_counts.count(s, xsg.COUNT_LINES)
    return got


def compare(gs, stream_counts, pattern, flags, want, light=False):
    """-> (got, keys that differ): counts before lists"""
    got = observe_counts(gs, stream_counts, pattern, flags, want, light)
    bad = [k for k in COUNT_KEYS if k in got and got[k] != want[k]]
    if bad:
        return got, bad
    if light:
        got["match_byte_offsets"] = gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist()
        got["line_byte_offsets"] = gs.shard.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
    else:
        got.update(gs.all_modes(pattern, flags))
        strings, off = gs.shard.search_matches()
        got["matches"] = (strings, off.tolist(), [len(x) for x in strings])
    return got, [k for k in want if k in got and got[k] != want[k]]


def report(got, want, bad, n=4):
    def first(a, b):
        if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) > 6:
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return f"{len(a)} entries for {len(b)}, the first difference at {k}: {str(a[k:k + 3])[:50]} for {str(b[k:k + 3])[:50]}"
        return f"got {str(a)[:70]} want {str(b)[:70]}"
    spans = lambda m: list(zip(m[1], m[2]))  # XSG_MATCHES: offsets and lengths say it, the strings only fill the line
    return "; ".join(f"{k}: {first(spans(got[k]), spans(want[k])) if k == 'matches' else first(got[k], want[k])}" for k in bad[:n])


def model_labels(family, b, blocks, flags):
    if family == "newline":
        return C.nlpat_labels(blocks, [C.raw_occurrences(c, b.pattern, flags) for c in blocks], b.pattern)
    if family == "verify":
        return C.verify_labels(blocks, b.pattern)
    if family == "probe":
        return C.probe_labels(blocks, b.pattern)
    return C.greedy_labels([C.raw_occurrences(c, b.pattern, flags) for c in blocks], C.pattern_length(b.pattern, b.flags))


def localise(gs, stream_counts, oracle, family, b, flags):
    """bind the cases one at a time -> the first whose results differ, with the branches the model says it takes"""
    for name, c in b.chunks:
        gs.bind([c])
        want = expect(oracle, [c], b.pattern, flags)
        got, bad = compare(gs, stream_counts, b.pattern, flags, want)
        if bad:
            return f"first failing case: [{name}] takes {sorted(model_labels(family, b, [c], flags))}; {report(got, want, bad)}"
    return "every case passes when its chunk is bound alone: the difference needs the chunks together"


def check_binding(gs, stream_counts, oracle, family, b, ctx=""):
    for flags in modes_of(b):
        blocks = C.blocks_of(b)
        gs.bind(blocks)
        want = expect(oracle, blocks, b.pattern, flags)
        assert want["count_matches"] >= 1
        got, bad = compare(gs, stream_counts, b.pattern, flags, want)
        if bad:
            padded = any(name == "padding" for name, _ in b.chunks)  # (alone, such a case takes another route)
            where = localise(gs, stream_counts, oracle, family, b, flags) if len(blocks) > 1 and not padded else \
                f"takes {sorted(model_labels(family, b, blocks, flags))}"
            pytest.fail(f"{ctx}{b.name} flags={flags:#x}: {where} -- on the whole binding: {report(got, want, bad, 3)}")
        # what is about the end of the list or the rounds of the closure: the case alone
        for i in b.solo:
            name, c = b.chunks[i]
            gs.bind([c])
            want = expect(oracle, [c], b.pattern, flags)
            got, bad = compare(gs, stream_counts, b.pattern, flags, want, light=True)
            assert not bad, (f"{ctx}{b.name} flags={flags:#x}: [{name}] bound alone takes {sorted(model_labels(family, b, [c], flags))}; "
                             f"{report(got, want, bad)}")


def ids(family):
    return [b.name.split(" ", 1)[1] for b in C.bindings(family)]


@pytest.mark.parametrize("b", C.bindings("budget"), ids=ids("budget"))
def test_budget(gs, stream_counts, oracle, b):
    """A: chains of 0 .. 8193 followers as the list's last entries, in front of a new head and inside a longer chain, through
    xsg_count / xsg_search (budget, flag, closure), xsg_count_async_status (no budget) and xsg_count_chunks"""
    check_binding(gs, stream_counts, oracle, "budget", b)


@pytest.mark.parametrize("b", C.bindings("seams"), ids=ids("seams"))
def test_seams(gs, stream_counts, oracle, b):
    """B: runs at the end of one chunk and at offset 0 of the next, with nothing, an empty chunk, one occurrence and a chunk
    shorter than the pattern between; the same chunks in reverse order"""
    check_binding(gs, stream_counts, oracle, "seams", b)
    rev = C.Binding(b.name + " reversed", b.pattern, b.flags, b.chunks[::-1], ())
    check_binding(gs, stream_counts, oracle, "seams", rev)


def test_rounds(gs, stream_counts, oracle):
    """C: 2^k - 1, 2^k, 2^k + 1 reported entries behind the budget: k and k + 1 marking rounds, each case alone"""
    (b,) = C.bindings("rounds")
    check_binding(gs, stream_counts, oracle, "rounds", b)


@pytest.mark.parametrize("b", C.bindings("links"), ids=ids("links"))
def test_links(gs, stream_counts, oracle, b):
    """D: nxt(i) = i + plen, i + 1, i + 2, i + 3; the window clamped at M; the target in the next chunk"""
    check_binding(gs, stream_counts, oracle, "links", b)


@pytest.mark.parametrize("b", C.bindings("newline"), ids=ids("newline"))
def test_newline(gs, stream_counts, oracle, b):
    """E: the line walk of a literal that holds a newline, 1 .. 65 537 lines, both tail modes, ignore-case on one"""
    check_binding(gs, stream_counts, oracle, "newline", b)


@pytest.mark.parametrize("expr", [b"xaa+", b"xaa+y", b"aaa+b?"], ids=lambda e: e.decode())
@pytest.mark.parametrize("pre", ["1", "0"])
def test_verify(gs, stream_counts, oracle, monkeypatch, pre, expr):
    """F: candidates that die one byte short of the verification budget, at it, and with the chunk's end at and one byte
    behind it; by the prefilter route (XSG_RX_PRE=1) and by the line walks (=0): the same results"""
    monkeypatch.setenv("XSG_RX_PRE", pre)
    assert xsg.regex_prefix(expr)[0] >= 3
    mine = [b for b in C.bindings("verify") if b.pattern == expr]
    assert mine
    for b in mine:
        check_binding(gs, stream_counts, oracle, "verify", b, ctx=f"XSG_RX_PRE={pre} ")


@pytest.mark.parametrize("b", C.bindings("probe"), ids=ids("probe"))
def test_probe(gs, stream_counts, oracle, b):
    """G: what a synchronous count establishes about a bordered literal on this binding, and what the stream-ordered entry
    points do with it (include/xsg.h): xsg_count_async_status serves the literal either way -- from the plain scan once it is
    known overlap-free, through its bounded list otherwise -- and xsg_count_chunks_async serves it only when it is known"""
    blocks = C.blocks_of(b)
    free = C.known_overlap_free(blocks, b.pattern, 0)
    for flags in modes_of(b):
        gs.bind(blocks)  # (a fresh binding: nothing is known yet)
        gs.ctx.set_pattern(b.pattern, flags)
        want = expect(oracle, blocks, b.pattern, flags)
        where = f"{b.name} flags={flags:#x} takes {sorted(C.probe_labels(blocks, b.pattern))}"
        with pytest.raises(xsg.XsgError) as e:  # before any synchronous call
            stream_counts.count_chunks(gs.shard, xsg.COUNT_MATCHES)
        assert e.value.code == xsg.ENOTSUP, where
        c = gs.shard.count(xsg.COUNT_MATCHES)
        assert int(c[xsg.CTR_MATCHES]) == want["count_matches"], where
        assert stream_counts.count(gs.shard, xsg.COUNT_MATCHES) == (want["count_matches"], 0), where
        if free:
            assert stream_counts.count_chunks(gs.shard, xsg.COUNT_MATCHES) == (want["chunk_matches"], want["count_matches"], 0), where
        else:
            with pytest.raises(xsg.XsgError) as e:
                stream_counts.count_chunks(gs.shard, xsg.COUNT_MATCHES)
            assert e.value.code == xsg.ENOTSUP, where
        got, bad = compare(gs, stream_counts, b.pattern, flags, want)
        assert not bad, f"{where}: {report(got, want, bad)}"
        # ... and the same when the first synchronous call is a search
        gs.bind(blocks)
        gs.ctx.set_pattern(b.pattern, flags)
        assert gs.shard.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist() == want["match_byte_offsets"], where
        assert stream_counts.count(gs.shard, xsg.COUNT_MATCHES) == (want["count_matches"], 0), where
        if free:
            assert stream_counts.count_chunks(gs.shard, xsg.COUNT_MATCHES) == (want["chunk_matches"], want["count_matches"], 0), where
