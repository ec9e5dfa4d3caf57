"""Call sequences on ONE context and ONE shard: the operations, a model that predicts every result from what the ABI
promises (include/xsg.h), and a generator with fixed seeds.

A binding carries state from call to call (x-search_amd/csrc/xsg_objects.h: the per-tile arrays and their clean flags,
the newline cache, the choices keyed by pattern_serial, the pending result).  The other GPU suites drive a binding
through one call order (tests/gpu_util.py: GpuSearch.all_modes); here the order is the variable.

An OPERATION is a tuple that prints as a Python literal:
  ("bind", kind, data, layout)   kind: create | smaller | larger_fit | larger_nofit | one_chunk | empty | same_addr | other
                                 data: a key of DATA; layout: 0 offsets and line bases derived, 1 both explicit,
                                 2 explicit offsets, line bases derived (xsg_shard_set_line_base applies)
  ("invalidate", data)           overwrite the bound bytes in place with `data` (same chunk lengths), xsg_shard_invalidate
  ("set_line_base", n)
  ("set_pattern", pattern, flags)
  ("count", tag, with_newlines, via)   tag: matches | lines; via: one of COUNT_VIAS
  ("list", kind)                 one of LIST_KINDS
  ("tune", mode) / ("time_scan", mode, iters)
  ("toggle", NAME, value or None)      an XSG_* variable read through XSG_TOGGLE; None unsets it

The MODEL keeps only: bound blocks, offsets, bases, pattern, flags, line base.  Every expected value comes from
gpu_util.oracle_all_modes / oracle_regex_all_modes, anchor_oracle and invert_model, memoised per (data, layout, pattern,
flags).  It holds no library-internal state: a fresh context must give the same answers.  Where the header leaves an
outcome to such state (the asynchronous match count next to XSG_WITH_NEWLINES of a pattern that may overlap itself, the capacity of the
bounded device-side list after earlier list passes) the model raises Ambiguous and the generator does not go there.

No torch here: tests/test_call_sequences.py checks the generator's reach without a GPU.
"""
import numpy as np

import anchor_oracle
import corpus
import invert_model
import xsg
from gpu_util import oracle_all_modes, oracle_regex_all_modes
from xs_oracle import UnsupportedRegex, compile_class_sequence

TILE = 16384
X, I, R, V = xsg.FLAG_EXACT_TAIL, xsg.FLAG_IGNORE_CASE, xsg.FLAG_REGEX, xsg.FLAG_INVERT

COUNT_VIAS = ("sync", "begin_end", "async", "async_stream", "status")
LIST_KINDS = ("match_byte_offsets", "line_byte_offsets", "line_indices", "lines", "lines_view", "u64_view", "result_newlines")
MATCH_ONLY_LISTS = ("match_byte_offsets",)
REBIND_KINDS = ("smaller", "larger_fit", "larger_nofit", "one_chunk", "empty", "same_addr")
REFUSALS = ("invert_match", "estate", "nonascii", "overflow")
MODES = (xsg.COUNT_MATCHES, xsg.COUNT_LINES, xsg.COUNT_MATCHES | xsg.WITH_NEWLINES, xsg.COUNT_LINES | xsg.WITH_NEWLINES)
# read at every use under XSG_TEST_HOOKS=1 (x-search_amd/csrc/xsg_objects.h: XSG_TOGGLE); none changes a result
TOGGLES = {"XSG_LIST_FAST": ("0", "1"), "XSG_LIST_CAP": ("3", "64"), "XSG_LINES_EAGER": ("0",), "XSG_RX_PRE": ("0", "1"),
           "XSG_RX_FAC": ("0", "1"), "XSG_RX_SKIP": ("0", "1"), "XSG_RX_TRIG": ("0", "1"), "XSG_DENSE_PER": ("64", "1000000"),
           "XSG_CLS_FAST": ("0", "1"), "XSG_CLS_INREG": ("0", "1")}

# the coarse classes of the issue's list; ordered pairs of these must all occur
CLASSES = ("set_pattern", "count", "list", "bind", "measure", "toggle", "refuse")


class Ambiguous(ValueError):
    """the header leaves this call's outcome to state the model does not keep"""


# ---------------------------------------------------------------------------
# data: every set is a pure function of its name
# ---------------------------------------------------------------------------
def _u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8).copy()


def _text(seed, sizes):
    """text in which every needle of the pool sits in some lines and not in others (tests/test_gpu_invert.py: text_blocks)"""
    out = []
    for i, n in enumerate(sizes):
        needle = (b"Sherlock", b"colour", b"locking", b"color")[i % 4]
        if n < 2:
            out.append(_u8(b"e\n"[:n]))
        else:
            out.append(corpus.text_block(seed, i, n, needle=needle, needle_rate=2e-2))
    return out


_MANY = [33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 39, 40, 41] * 3


def _runs():
    """1.2 MiB of 'a' with a newline every 5000 bytes: more raw occurrences of `aa` than the bounded device-side list of
    xsg_count_async holds (2^20, include/xsg.h)"""
    b = np.full(1_200_000, ord("a"), dtype=np.uint8)
    b[4999::5000] = 10
    return [b]


_SPEC = {
    # chunk sizes from tests/test_gpu_fuzz.py: SIZES; the last chunk of most sets is small-alphabet text (`aa`, `abab`)
    "base": lambda s: _text(31 + s, [TILE * 3 + 5, TILE + 1, 4097]) + [corpus.small_alphabet(1 + s, 4095, b"ab \n")],
    "small": lambda s: _text(33 + s, [TILE - 1, 1025]) + [corpus.small_alphabet(3 + s, 1023, b"ab \n")],
    "mid": lambda s: _text(35 + s, [TILE * 2 + 1, TILE * 2 - 1, TILE, 4096, 65]) + [corpus.small_alphabet(5 + s, TILE + 1, b"ab \n")],
    "many": lambda s: _text(37 + s, _MANY),
    "one": lambda s: _text(39 + s, [TILE * 2 + 1]),
    "empty": lambda s: [np.zeros(0, dtype=np.uint8)],
    "nonascii": lambda s: [np.concatenate([_text(41 + s, [TILE + 1])[0], _u8("grüße the\n".encode())]), _text(43 + s, [4097])[0]],
    "runs": lambda s: _runs(),
}
DATA = tuple(_SPEC) + tuple(k + "_alt" for k in _SPEC if k not in ("empty", "runs"))
_blocks_memo = {}


def blocks_of(data: str):
    if data not in _blocks_memo:
        key, alt = (data[:-4], 1) if data.endswith("_alt") else (data, 0)
        _blocks_memo[data] = _SPEC[key](alt)
    return _blocks_memo[data]


def ntiles_of(data: str) -> int:
    return sum((int(b.size) + TILE - 1) // TILE for b in blocks_of(data))


def nbytes_of(data: str) -> int:
    return sum(int(b.size) for b in blocks_of(data))


def layout_of(data: str, layout: int):
    """-> (global_offsets, line_bases) as tests/gpu_util.py: upload takes them"""
    n = len(blocks_of(data))
    go = [10_000_000 * (n - i) + 13 for i in range(n)]  # disjoint, descending, not aligned
    lb = [1000 * i + 7 for i in range(n)]
    return (None, None) if layout == 0 else (go, lb) if layout == 1 else (go, None)


# ---------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------
FAMILIES = ("lit_mask1", "lit_one", "lit_mask2", "lit_two", "lit_long", "bordered", "classseq", "rx_prefix", "rx_factor",
            "anchored", "inverted")


def _long_pattern():
    return blocks_of("base")[0][5000:6100].tobytes()  # longer than the KiB the scan kernel keeps in LDS


def pool():
    """(pattern, flags, family).  Literals of every kind (1-3 bytes, 4, 5-7, 8, longer, one longer than 1 KiB), bordered ones,
    one that contains a newline, ignore_case, both tail modes, a class sequence, automata with a prefix and with a factor,
    the three anchor forms, XSG_FLAG_INVERT on literals and regexes, ascii_only expressions."""
    return [
        (b"e", 0, "lit_mask1"), (b"the", 0, "lit_mask1"), (b"the", X, "lit_mask1"), (b"E", I, "lit_mask1"),
        (b"lock", 0, "lit_one"), (b"from", X, "lit_one"),
        (b"Holmes", 0, "lit_mask2"), (b"Watson", X, "lit_mask2"), (b"which", 0, "lit_mask2"),
        (b"Sherlock", 0, "lit_two"), (b"sHERLOCK", I, "lit_two"), (b"Sherlock", X, "lit_two"),
        (b"detective street", 0, "lit_long"), (b"detective", X, "lit_long"), (b"street\nthe", 0, "lit_long"), (_long_pattern(), 0, "lit_long"),
        (b"aa", 0, "bordered"), (b"abab", 0, "bordered"), (b"that", 0, "bordered"), (b"THAT", I | X, "bordered"),
        (b"She[r ]lock", R, "classseq"), (b"t.e", R, "classseq"), (b"she[r ]LOCK", R | I, "classseq"),
        (b"colou?r", R, "rx_prefix"), (b"lock(ed|s)?", R, "rx_prefix"),
        (b"\\w+ing", R, "rx_factor"),
        (b"(?m)^She", R, "anchored"), (b"(?m)locked$", R, "anchored"), (b"(?m)^[a-z]+$", R, "anchored"), (b"Sher.*k", R, "rx_prefix"),
        (b"the", V, "inverted"), (b"Sherlock", V | X, "inverted"), (b"that", V, "inverted"), (b"She[r ]lock", R | V, "inverted"),
        (b"\\w+ing", R | V, "inverted"), (b"(?m)^She", R | V, "inverted"), (b"t.e", R | V, "inverted"),
    ]


ASCII_ONLY = (b"t.e", b"Sher.*k")
# xsg_set_pattern refuses these (include/xsg.h, XSG_FLAG_INVERT: a pattern that can match '\n'); the context then holds no pattern
REFUSED_PATTERNS = ((b"a\nb", V), (b"She\\s+lock", R | V), (b"\n", V | X))


def has_border(p: bytes) -> bool:
    return any(p[:k] == p[-k:] for k in range(1, len(p)))


def family_of(pat: bytes, flags: int) -> str:
    for p, f, fam in pool():
        if p == pat and f == flags:
            return fam
    raise KeyError((pat, flags))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
_modes_memo = {}


def expected_modes(oracle, data, layout, pat, flags):
    """the dict of gpu_util.oracle_all_modes for this binding and pattern (inverted if the flag is set), or the string
    "nonascii" where an ascii_only expression meets a byte >= 0x80"""
    key = (data, layout, pat, flags)
    if key in _modes_memo:
        return _modes_memo[key]
    blocks = blocks_of(data)
    go, lb = layout_of(data, layout)
    icase = bool(flags & I)
    try:
        if not flags & R:
            plain = oracle_all_modes(oracle, blocks, pat, exact=bool(flags & X), global_offsets=go, line_bases=lb, ignore_case=icase)
        elif pat.startswith(b"(?m)"):
            plain = anchor_oracle.all_modes(blocks, pat, icase, global_offsets=go, line_bases=lb)
        else:
            plain, with_lines = oracle_regex_all_modes(oracle, blocks, pat, icase, global_offsets=go, line_bases=lb)
            assert with_lines, "the pool holds no expression that can match a newline"
        if flags & V:
            inv = invert_model.invert_all_modes(plain, blocks, go, lb)
            inv["plain_count_lines"] = plain["count_lines"]
            plain = inv
    except UnsupportedRegex as e:
        assert "non-ASCII" in str(e), e
        plain = "nonascii"
    _modes_memo[key] = plain
    return plain


class Expect:
    """what one operation must return.  kind: none | counters | value | err | poison | status"""

    def __init__(self, kind, value=None, key=None, refusal=None):
        self.kind, self.value, self.key, self.refusal = kind, value, key, refusal

    value_nonzero = False  # the honesty cap: the expected value is non-empty / non-zero (inverted: R and I both non-empty)


class Model:
    def __init__(self, oracle=None):
        """oracle=None: follow the state only (the generator); expectations then carry no values"""
        self.oracle = oracle
        self.data = None
        self.layout = 0
        self.line_base = 0
        self.pattern = None
        self.flags = 0
        self.max_tiles = 0          # of every binding so far (the grown buffers)
        self.searched = False       # since the last bind / invalidate
        self.runs_listed = False    # a pass that may have taught the shard a list size ran on the 1.2 MiB set
        self.toggles = {}

    # -- facts about the current state -------------------------------------------------
    def inverted(self):
        return bool(self.flags & V)

    def bordered(self):
        return not self.flags & R and has_border(self.pattern.lower() if self.flags & I else self.pattern)

    def may_overlap(self):
        """include/xsg.h, xsg_count_async: "a literal with a border or a class sequence two of whose occurrences may overlap
        (`[a-z]{4}`, `t.e`; the test is conservative)": every fixed-length expression is taken as one that may"""
        if not self.flags & R:
            return self.bordered()
        if self.pattern.startswith(b"(?m)"):
            return False
        try:
            compile_class_sequence(self.pattern, bool(self.flags & I))
            return True
        except UnsupportedRegex:
            return False

    def newline_literal(self):
        return not self.flags & R and b"\n" in self.pattern

    def would_refuse_nonascii(self):
        return self.pattern is not None and self.pattern in ASCII_ONLY and self.data is not None and self.data.startswith("nonascii")

    def would_overflow(self):
        return self.data == "runs" and self.pattern == b"aa"

    def _modes(self):
        return expected_modes(self.oracle, self.data, self.layout, self.pattern, self.flags)

    # -- one operation -----------------------------------------------------------------
    def apply(self, op) -> Expect:
        head = op[0]
        if head == "bind":
            _, kind, data, layout = op
            if kind == "same_addr":
                assert [b.size for b in blocks_of(data)] == [b.size for b in blocks_of(self.data)], "same_addr: other chunk lengths"
            self.data, self.layout, self.searched = data, layout, False
            self.max_tiles = max(self.max_tiles, ntiles_of(data))
            return Expect("none")
        if head == "invalidate":
            assert [b.size for b in blocks_of(op[1])] == [b.size for b in blocks_of(self.data)], "invalidate: other chunk lengths"
            self.data, self.searched = op[1], False
            return Expect("none")
        if head == "set_line_base":
            self.line_base = op[1]
            return Expect("none")
        if head == "toggle":
            self.toggles[op[1]] = op[2]
            return Expect("none")
        if head == "set_pattern":
            _, pat, flags = op
            if (pat, flags) in REFUSED_PATTERNS:
                self.pattern, self.flags = None, 0
                return Expect("err", xsg.ENOTSUP, refusal="bad_pattern")
            self.pattern, self.flags = pat, flags
            return Expect("none")
        if head in ("tune", "time_scan"):
            if self.pattern is None:
                return Expect("err", xsg.ESTATE, refusal="estate")
            return Expect("none")
        if head == "count":
            return self._count(*op[1:])
        if head == "list":
            return self._list(op[1])
        raise ValueError(op)

    def _count(self, tag, with_nl, via):
        asynchronous = via in ("async", "async_stream", "status")
        if self.pattern is None:
            return Expect("err", xsg.ESTATE, refusal="estate")
        if tag == "matches" and self.inverted():
            return Expect("err", xsg.ENOTSUP, refusal="invert_match")
        if tag == "lines" and asynchronous and self.newline_literal():
            return Expect("err", xsg.ENOTSUP, refusal="nl_async")  # include/xsg.h, xsg_set_pattern: "use xsg_count"
        if tag == "matches" and asynchronous and self.may_overlap():
            if with_nl:
                raise Ambiguous("the asynchronous match count with XSG_WITH_NEWLINES of a pattern that may overlap itself: refused, for a "
                                "literal until a synchronous call has established that its occurrences do not overlap, for a class "
                                "sequence by a test the header calls conservative")
            if self.data == "runs":
                if self.searched or self.runs_listed or not self.would_overflow():
                    raise Ambiguous("the capacity of the bounded list depends on the last list pass")
                self.searched = True
                return Expect("status", xsg.STATUS_OVERFLOW, refusal="overflow") if via == "status" else Expect("poison", refusal="overflow")
        self.searched = True
        if self.data == "runs" and not asynchronous and tag == "matches" and self.bordered():
            self.runs_listed = True  # (xsg_count "sizes exactly, remembers the size")
        if self.would_refuse_nonascii():
            if not asynchronous:
                return Expect("err", xsg.ENOTSUP, refusal="nonascii")
            return Expect("status", xsg.STATUS_NONASCII, refusal="nonascii") if via == "status" else Expect("poison", refusal="nonascii")
        e = Expect("counters", key="count_" + tag)
        if self.oracle is not None:
            m = self._modes()
            e.value = {xsg.CTR_MATCHES if tag == "matches" else xsg.CTR_LINES: m["count_" + tag], xsg.CTR_BYTES: m["bytes"]}
            if with_nl:
                e.value[xsg.CTR_NEWLINES] = m["newlines"]
            e.value_nonzero = m["count_" + tag] > 0 and (not self.inverted() or m["plain_count_lines"] > 0)
        return e

    def _list(self, kind):
        if self.pattern is None:
            return Expect("err", xsg.ESTATE, refusal="estate")
        if kind in MATCH_ONLY_LISTS and self.inverted():
            return Expect("err", xsg.ENOTSUP, refusal="invert_match")
        self.searched = True
        self.runs_listed |= self.data == "runs"
        if self.would_refuse_nonascii():
            return Expect("err", xsg.ENOTSUP, refusal="nonascii")
        e = Expect("value", key=kind)
        if self.oracle is not None:
            m = self._modes()
            base = self.line_base if layout_of(self.data, self.layout)[1] is None else 0
            if kind in ("match_byte_offsets", "line_byte_offsets"):
                e.value = m[kind]
            elif kind == "u64_view":
                e.value = m["line_byte_offsets"]
            elif kind == "line_indices":
                e.value = [x + base for x in m["line_indices"]]
            elif kind == "result_newlines":
                e.value = m["newlines"]
            else:
                e.value = (m["lines"], m["lines_offsets"])
            v = e.value[0] if isinstance(e.value, tuple) else e.value
            e.value_nonzero = bool(v) and (not self.inverted() or m["plain_count_lines"] > 0)
        return e


def op_class(op, expect: Expect) -> str:
    """one of CLASSES"""
    if expect.refusal is not None:
        return "refuse"
    return {"bind": "bind", "invalidate": "bind", "set_line_base": "bind", "time_scan": "measure"}.get(op[0], op[0])


def result_kind(op, expect: Expect):
    """the result-producing classes: "count:<via>" / "list:<kind>", or None (also for a refused call)"""
    if expect.kind not in ("counters", "value"):
        return None
    return "count:" + op[3] if op[0] == "count" else "list:" + op[1]


RESULT_KINDS = tuple("count:" + v for v in COUNT_VIAS) + tuple("list:" + k for k in LIST_KINDS)


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
class _Gen:
    """One sequence.  Goals are taken from lists shared by all sequences (sequences() builds them in seed order), so the
    committed seeds together reach every pair tests/test_call_sequences.py asks for; between goals the steps are random."""

    def __init__(self, seed, todo):
        self.rng = np.random.default_rng(4200 + seed)
        self.todo = todo
        self.m = Model()
        self.ops = []
        self.toggled = set()
        self.runs_used = False

    def emit(self, op):
        e = self.m.apply(op)  # raises Ambiguous if the generator went where the header does not decide
        self.ops.append(op)
        return e

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    # -- patterns ---------------------------------------------------------------------
    def patterns(self, family=None, want=None):
        out = []
        for p, f, fam in pool():
            if family is not None and fam != family:
                continue
            if self.m.data == "runs" and (f & R or len(p) > 16):
                continue  # (a 1.2 MiB shard: literals only, the Python regex walks take seconds there)
            if want is not None and not self.serves(p, f, want):
                continue
            out.append((p, f))
        return out

    def serves(self, p, f, want) -> bool:
        """does the pattern give `want` (a result kind) a value on the current data, and unambiguously"""
        if p in ASCII_ONLY and self.m.data.startswith("nonascii"):
            return False
        kind = want.split(":")[1]
        if want.startswith("list:"):
            return not (f & V and kind in MATCH_ONLY_LISTS)
        if kind in ("async", "async_stream", "status"):  # (count goals ask for XSG_COUNT_LINES: served for every pattern but these)
            return not (not f & R and b"\n" in p)
        return True

    def set_pattern(self, family=None, want=None):
        cands = self.patterns(family, want) or self.patterns(None, want)
        p, f = self.pick(cands)
        self.emit(("set_pattern", p, f))

    def ensure_pattern(self, want):
        if self.m.pattern is None or not self.serves(self.m.pattern, self.m.flags, want) or self.m.would_refuse_nonascii():
            self.set_pattern(want=want)

    # -- results ----------------------------------------------------------------------
    def result(self, want=None):
        want = want or self.pick(RESULT_KINDS)
        self.ensure_pattern(want)
        kind = want.split(":")[1]
        if want.startswith("list:"):
            return self.emit(("list", kind))
        tag = "lines"
        if not self.m.inverted() and self.rng.random() < 0.5:
            tag = "matches"
        nl = bool(self.rng.integers(0, 2))
        if tag == "matches" and kind != "sync" and kind != "begin_end" and self.m.may_overlap():
            if self.m.data == "runs":
                tag = "lines"
            nl = False
        if tag == "lines" and kind in ("async", "async_stream", "status") and self.m.newline_literal():
            tag, nl = "matches", False
        return self.emit(("count", tag, nl, kind))

    # -- bindings ---------------------------------------------------------------------
    def bind(self, kind, layout=None):
        layout = int(self.rng.integers(0, 3)) if layout is None else layout
        cur = self.m.data
        if kind == "same_addr":
            if cur in ("empty", "runs"):
                self.bind("other")
                cur = self.m.data
            data = cur[:-4] if cur.endswith("_alt") else cur + "_alt"
            return self.emit(("bind", kind, data, self.m.layout))  # (the same table: offsets and bases stay)
        if kind == "smaller":
            if nbytes_of(cur) <= nbytes_of("small"):
                self.emit(("bind", "other", "base", layout))
            data = self.pick(("small", "small_alt"))
        elif kind == "larger_fit":
            if ntiles_of(cur) >= ntiles_of("mid"):
                self.emit(("bind", "other", "small", layout))
            data = self.pick(("mid", "mid_alt"))
        elif kind == "larger_nofit":
            assert self.m.max_tiles <= 64
            data = self.pick(("many", "many_alt"))
        elif kind == "one_chunk":
            data = self.pick(("one", "one_alt"))
        elif kind == "empty":
            data = "empty"
        else:
            data = self.pick(("base", "base_alt", "mid", "small", "nonascii"))
        return self.emit(("bind", kind, data, layout))

    def invalidate(self):
        cur = self.m.data
        if cur in ("empty", "runs"):
            self.bind("other")
            cur = self.m.data
        self.emit(("invalidate", cur[:-4] if cur.endswith("_alt") else cur + "_alt"))

    # -- the predecessors of the second coverage list -------------------------------------
    def predecessor(self, pred, want):
        """emit `pred` so that `want` can follow directly (refusals that leave no usable pattern: after one set_pattern)"""
        if pred.startswith("rebind:"):
            kind = pred.split(":")[1]
            if kind == "larger_nofit" and self.m.max_tiles > 64:
                return False
            self.ensure_pattern(want)
            self.bind(kind)
            if self.m.would_refuse_nonascii() or not self.serves(self.m.pattern, self.m.flags, want):
                return False
        elif pred == "invalidate":
            self.ensure_pattern(want)
            self.invalidate()
        elif pred == "measure":
            self.ensure_pattern(want)
            self.measure()
        elif pred == "toggle":
            self.ensure_pattern(want)
            self.toggle()
        elif pred == "refuse:invert_match":
            if want in ("list:match_byte_offsets",):
                return False
            cands = [(p, f) for p, f in self.patterns("inverted") if self.serves(p, f, want)]
            self.emit(("set_pattern",) + self.pick(cands))
            if self.rng.random() < 0.5:
                self.emit(("list", "match_byte_offsets"))
            else:
                self.emit(("count", "matches", bool(self.rng.integers(0, 2)), self.pick(COUNT_VIAS)))
        elif pred == "refuse:estate":
            self.emit(("set_pattern",) + self.pick(REFUSED_PATTERNS))
            self.result_raw()
            self.set_pattern(want=want)  # the one repair the header demands: the context holds no pattern
        elif pred == "refuse:nonascii":
            if not self.m.data.startswith("nonascii"):
                self.emit(("bind", "other", self.pick(("nonascii", "nonascii_alt")), int(self.rng.integers(0, 3))))
            p = self.pick(ASCII_ONLY)
            self.emit(("set_pattern", p, R | (V if p == b"t.e" and self.rng.random() < 0.3 else 0)))
            self.result_raw(lines_only=self.m.inverted())
            cands = [(p, f) for p, f in self.patterns(None, want) if p not in ASCII_ONLY]
            self.emit(("set_pattern",) + self.pick(cands))  # without a rebind
        elif pred == "refuse:overflow":
            if self.runs_used:
                return False
            self.runs_used = True
            self.emit(("bind", "other", "runs", 0))
            self.emit(("set_pattern", b"aa", 0))
            self.emit(("count", "matches", False, self.pick(("async", "async_stream", "status"))))
            if want in ("count:async", "count:async_stream", "count:status"):
                self.emit(("count", "lines", bool(self.rng.integers(0, 2)), want.split(":")[1]))
            else:
                self.result(want)
            self.bind("other")
            return None  # (done: the result is emitted)
        return True

    def result_raw(self, lines_only=False):
        """a search call whatever the state (refusals)"""
        k = self.pick(RESULT_KINDS)
        if k.startswith("list:"):
            kind = k.split(":")[1]
            if lines_only and kind in MATCH_ONLY_LISTS:
                kind = "lines"
            self.emit(("list", kind))
        else:
            self.emit(("count", "lines" if lines_only or self.rng.random() < 0.5 else "matches", False, k.split(":")[1]))

    def measure(self):
        if self.m.pattern is None:
            self.set_pattern()
        # (no xsg_shard_tune here: below 1 GiB it keeps the default without a launch; tests/test_gpu_call_sequences.py drives it
        # on a shard it measures)
        self.emit(("time_scan", self.pick(MODES), int(self.rng.integers(1, 4))))

    def toggle(self):
        if self.todo["tog"]:  # every value of every toggle somewhere
            name, value = self.todo["tog"].pop(0)
            self.toggled.add(name)
            return self.emit(("toggle", name, value))
        name = self.pick(sorted(TOGGLES))
        if name in self.toggled and self.rng.random() < 0.5:
            self.toggled.discard(name)
            self.emit(("toggle", name, None))
        else:
            self.toggled.add(name)
            self.emit(("toggle", name, self.pick(TOGGLES[name])))

    # -- goals ------------------------------------------------------------------------
    def goal_pred(self):
        if not self.todo["pred"]:
            return False
        # a binding that outgrows the buffers and the 1.2 MiB shard of the overflow refusal come once per sequence: first
        k = next((k for k, (p, _) in enumerate(self.todo["pred"]) if p == "rebind:larger_nofit" and self.m.max_tiles <= 64), None)
        if k is None:
            k = next((k for k, (p, _) in enumerate(self.todo["pred"]) if p == "refuse:overflow" and not self.runs_used), 0)
        pred, want = self.todo["pred"].pop(k)
        mark = len(self.ops)
        snap = (dict(self.m.__dict__, toggles=dict(self.m.toggles)), set(self.toggled), self.runs_used)
        ok = self.predecessor(pred, want)
        if ok is False:  # not reachable from here: put everything back, try in a later sequence
            del self.ops[mark:]
            self.m.__dict__.update(snap[0])
            self.toggled, self.runs_used = snap[1], snap[2]
            self.todo["pred"].append((pred, want))
            return False
        if ok is True:
            if want.startswith("count:"):
                self.emit(("count", "lines", bool(self.rng.integers(0, 2)), want.split(":")[1]))
            else:
                self.emit(("list", want.split(":")[1]))
        return True

    def goal_families(self):
        if not self.todo["fam"]:
            return False
        a, b = self.todo["fam"].pop(0)
        if self.m.data == "runs" or self.m.data.startswith("nonascii"):
            self.emit(("bind", "other", self.pick(("base", "base_alt", "mid", "small")), int(self.rng.integers(0, 3))))
        for fam in (a, b):  # each searched by a call it serves, so that no other pattern comes between
            want = self.pick([w for w in RESULT_KINDS if self.patterns(fam, w)])
            self.set_pattern(fam, want)
            self.result(want)
        return True

    def goal_first_newlines(self):
        if not self.todo["nl"]:
            return False
        fam = self.todo["nl"].pop(0)
        self.bind(self.pick(("other", "smaller", "larger_fit", "same_addr")))
        if self.m.data.startswith("nonascii"):
            self.emit(("bind", "other", "base", 0))
        self.set_pattern(fam)
        if self.rng.random() < 0.5:
            self.emit(("list", self.pick(("line_indices", "result_newlines"))))
        else:
            nl_vias = COUNT_VIAS if not self.m.newline_literal() else ("sync", "begin_end")
            self.emit(("count", "lines", True, self.pick(nl_vias)))
        for _ in range(3):
            others = [(p, f) for p, f, x in pool() if x != fam and not (p in ASCII_ONLY and self.m.data.startswith("nonascii"))]
            self.emit(("set_pattern",) + self.pick(others))
            if self.rng.random() < 0.5:
                self.emit(("list", self.pick(("line_indices", "result_newlines"))))
            else:
                nl_vias = COUNT_VIAS if not self.m.newline_literal() else ("sync", "begin_end")
                self.emit(("count", "lines", True, self.pick(nl_vias)))
        return True

    def one_of_class(self, cl, inverted):
        if cl == "set_pattern":
            self.set_pattern("inverted" if inverted else None)
        elif cl == "count":
            self.result(self.pick(RESULT_KINDS[:5]))
        elif cl == "list":
            self.result(self.pick([k for k in RESULT_KINDS[5:] if k != "list:match_byte_offsets"]))
        elif cl == "bind":
            self.pick((lambda: self.bind(self.pick(("smaller", "one_chunk", "same_addr"))), self.invalidate,
                       lambda: self.emit(("set_line_base", int(self.rng.integers(0, 100000))))))()
        elif cl == "measure":
            self.measure()
        elif cl == "toggle":
            self.toggle()
        else:  # the cheapest refusal: a match tag under XSG_FLAG_INVERT
            self.emit(self.pick((("list", "match_byte_offsets"), ("count", "matches", False, self.pick(COUNT_VIAS)))))

    def goal_classes(self):
        if not self.todo["cls"]:
            return False
        a, b = self.todo["cls"].pop(0)
        inverted = "refuse" in (a, b)
        if inverted and (self.m.pattern is None or not self.m.inverted()):
            self.set_pattern("inverted")
        if self.m.would_refuse_nonascii() or self.m.data == "runs":
            self.bind("smaller")
        self.one_of_class(a, inverted)
        self.one_of_class(b, inverted)
        return True

    def random_step(self):
        r = self.rng.random()
        if r < 0.40:
            self.result()
        elif r < 0.55:
            self.set_pattern()
        elif r < 0.65:
            self.bind(self.pick([k for k in REBIND_KINDS if k != "larger_nofit"]))
        elif r < 0.70:
            self.invalidate()
        elif r < 0.75:
            self.emit(("set_line_base", int(self.rng.integers(0, 100000))))
        elif r < 0.83:
            self.measure()
        elif r < 0.93:
            self.toggle()
        else:
            self.predecessor(self.pick(("refuse:invert_match", "refuse:estate", "refuse:nonascii")), self.pick(RESULT_KINDS[:5]))

    def run(self, length):
        self.emit(("bind", "create", self.pick(("base", "small", "mid", "one")), int(self.rng.integers(0, 3))))
        self.set_pattern()
        if self.todo["once"]:  # the documented refusal that leaves everything usable: XSG_COUNT_LINES of a literal with '\n', stream-ordered
            self.todo["once"].pop()
            self.emit(("set_pattern", b"street\nthe", 0))
            for via in ("async", "async_stream", "status"):
                self.emit(("count", "lines", via == "status", via))
            self.emit(("count", "lines", True, "sync"))
        while len(self.ops) < length:
            r = self.rng.random()
            if not ((r < 0.40 and self.goal_pred()) or (r < 0.65 and self.goal_families()) or (r < 0.75 and self.goal_first_newlines())
                    or (r < 0.85 and self.goal_classes())):
                self.random_step()
        if self.m.pattern is None:
            self.set_pattern()
        for name in sorted(self.toggled):  # every toggle back to unset at the end of its sequence
            self.emit(("toggle", name, None))
        return self.ops


PREDECESSORS = tuple("rebind:" + k for k in REBIND_KINDS) + ("invalidate", "measure", "toggle") + tuple("refuse:" + k for k in REFUSALS)
# a match tag cannot follow the refusal of a match tag under the same inverted pattern (include/xsg.h, XSG_FLAG_INVERT)
UNREACHABLE_PRED = {("refuse:invert_match", "list:match_byte_offsets")}

N_SEQUENCES = 12
SEQUENCE_LENGTH = 150
_sequences = None


def sequences():
    """the committed sequences, by seed 0 .. N_SEQUENCES - 1 (built together: the goal lists run through all of them)"""
    global _sequences
    if _sequences is None:
        order = np.random.default_rng(99)
        pred = [(p, w) for p in PREDECESSORS for w in RESULT_KINDS if (p, w) not in UNREACHABLE_PRED]
        fam = [(a, b) for a in FAMILIES for b in FAMILIES]
        order.shuffle(pred)
        order.shuffle(fam)
        todo = {"pred": [tuple(x) for x in pred], "fam": [tuple(x) for x in fam], "nl": list(FAMILIES),
                "cls": [(a, b) for a in CLASSES for b in CLASSES], "once": ["nl_async"],
                "tog": [(n, v) for n in sorted(TOGGLES) for v in TOGGLES[n]]}
        _sequences = [_Gen(seed, todo).run(SEQUENCE_LENGTH) for seed in range(N_SEQUENCES)]
        assert not todo["fam"] and not todo["nl"] and not todo["cls"] and not todo["tog"], (len(todo["fam"]), todo["nl"], todo["cls"])
        assert not todo["pred"], todo["pred"]
    return _sequences


def walk(ops, oracle=None):
    """-> [(index, op, Expect)] of a sequence under a fresh model"""
    m = Model(oracle)
    return [(i, op, m.apply(op)) for i, op in enumerate(ops)]


# ---------------------------------------------------------------------------
# tile_last across the wrap of its 16-bit epoch (x-search_amd/csrc/xsg_count.cpp: prepare_tiles)
# ---------------------------------------------------------------------------
def walk_from(oracle, data, pat: bytes, start: int) -> int:
    """matches the reference's walk (search_wrappers.h:29-52) finds from `start` on: findNext, resume at the match's end"""
    n, shift = 0, int(start)
    while shift < len(data):
        m = oracle.find_next(pat, data, shift)
        if m < 0:
            break
        n += 1
        shift = m + len(pat)
    return n


def epoch_wrap_case():
    """-> (chunk, A, end of A's last match, B).  One chunk of one tile.  A = `aab` has its last bulk match late in the tile: the
    scan leaves the end of that match in the tile's tile_last word.  B = `ba` (lossy tail mode, 2 bytes) has no occurrence
    before the chunk's tail zone and one at its first byte: the walk finds it when it enters the zone from the chunk's start
    (B has no bulk match) and loses it when it enters at A's end, one byte further on."""
    n = 1000
    d = np.full(n, ord("x"), dtype=np.uint8)
    d[99::100] = 10
    d[n - 1] = ord("x")
    d[n - 35:n - 28] = np.frombuffer(b"aabaaab", dtype=np.uint8)  # `aab` at n - 35 (bulk), `ba` at n - 33 (the zone's first byte)
    return d, b"aab", n - 32, b"ba"
