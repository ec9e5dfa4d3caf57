"""tests/class_paths.py without a GPU: the compiler's choices as the hook reports them, the path every directed
expression is there for, and the census -- over the directed list and the committed seeds every path k_scan can take
is reached by at least five expressions whose texts hold, on that path, a true match, a filter-passing decoy that is
rejected and (with several alternatives) a rejected crossover.  That is a condition on the INPUTS of
tests/test_gpu_class_paths.py, checked with the oracle alone; the oracle's walk is in turn pinned against CPython's
re.finditer for every one of these long expressions, in both cases."""
import os
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import class_paths as CP
import packing as P
import xsg
from xs_oracle import compile_class_sequence

ROOT = Path(__file__).resolve().parents[1]
MIN_PER_CELL = 5


@pytest.fixture(scope="module")
def texts():
    return CP.all_texts()


@pytest.fixture(scope="module")
def censuses(texts, oracle):
    return {label: CP.census(t.info, t.case.blocks, CP.true_starts(oracle, t.info, t.case.blocks)) for label, t in texts.items()}


def test_the_hook_is_no_part_of_the_abi():
    assert "xsg_test_class_fields" not in (ROOT / "include" / "xsg.h").read_text()
    assert "xsg_test_class_fields" not in xsg.EXPORTS
    # without XSG_TEST_HOOKS=1 it answers nothing (the switch is read once per process: a fresh one)
    code = ("import sys; sys.path[:0] = %r; import class_paths as CP, xsg\n"
            "try:\n    CP.class_fields(b'[a-z]{3}Sherlock')\nexcept xsg.XsgError as e:\n    print('refused', e.code)\n"
            % [str(ROOT / "tests"), str(ROOT / "x-search_amd"), str(ROOT / "oracle")])
    env = dict(os.environ, XSG_TEST_HOOKS="0", XSG_NO_TORCH_PRELOAD="1")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.stdout.strip() == f"refused {xsg.ENOTSUP}", (r.stdout, r.stderr[-2000:])


def test_the_hook_agrees_with_regex_info(texts):
    """plen, nalt and ascii_only, case-sensitive and not (info_of asserts it), and the window lies inside the expression"""
    for t in texts.values():
        for flags in (0, CP.IC):
            info = CP.info_or_none(t.info.expr, flags)
            if info is None:
                assert flags and t.info.f.plen <= 8, t.info.expr
                continue
            f = info.f
            assert 1 <= f.plen <= 32 and 1 <= f.nalt <= 8 and f.nalt * f.plen <= 64 and f.koff + min(8, f.plen) <= max(f.plen, 8), (info.expr, f)
            assert f.koff == 0 or f.koff + 8 <= f.plen, (info.expr, f)
            assert f.has_newline == int(bool(info.union[:, 10].any())), info.expr
            assert not (f.cls_inreg and f.cls_exact) and (not (f.cls_inreg or f.cls_exact) or (f.nalt == 1 and f.plen <= 8 and f.koff == 0)), (info.expr, f)
            for i in range(8):  # the window's mask and value are those of the union's members at koff + i
                k = f.koff + i
                members = np.flatnonzero(info.union[k]) if k < f.plen else np.zeros(0, dtype=np.int64)
                if members.size:
                    assert ((members & info.agree[i]) == info.value[i]).all(), (info.expr, i)
                else:
                    assert info.agree[i] == 0 and info.value[i] == 0, (info.expr, i)


def test_the_hook_refuses_what_the_class_compiler_hands_on():
    for expr in CP.OVER_LIMIT + [CP.FACTOR_EXPR, b"colou?r", b"(?m)^She[r ]lock", b"a\\.b"]:
        with pytest.raises(xsg.XsgError) as e:
            CP.class_fields(expr)
        assert e.value.code == xsg.ENOTSUP, expr
    # the automaton route's factor of the directed expression is the 16-position sequence the tests build its text from
    n, sets = xsg.regex_factor(CP.FACTOR_EXPR)
    assert n == 16 and xsg.regex_prefix(CP.FACTOR_EXPR)[0] == 0
    assert (sets == xsg.regex_info(CP.FACTOR_OF)[3][0]).all()
    assert CP.paths_of(CP.class_fields(CP.FACTOR_OF)) >= {"memory:long"}


FACTS = [  # (expression, positions, alternatives, koff or None: whatever the compiler picks, as long as it is > 0)
    (b"[a-z]{3}Sherlock", 11, 1, 3), (b"[a-z]{5} Sherlock Holmes", 21, 1, None), (b"Sherlock [A-Z][a-z]{5}", 15, 1, 0),
    (b"[0-9]{4}-[0-9]{2}-[0-9]{2}T[0-9]{2}:[0-9]{2}", 16, 1, None), (b"\\w{8}ing \\w{4}", 16, 1, None),
    (b"(Sherlock|detectiv) (Holmes|street)", 15, 4, None), (b"a{32}|b{32}", 32, 2, 0), (CP.ALT8x8, 8, 8, 0), (CP.ALT7x9, 9, 7, 0),
    (b"x.{11}y", 13, 1, 0), (b"x.{12}y", 14, 1, 0), (b"[^a]{13}", 13, 1, 0), (b"[ab]{9}", 9, 1, 0), (b"a[ab]{15}", 16, 1, 0),
    (b"[ab]{31}b", 32, 1, 24), (b"Sherlock [a-z]{3}", 12, 1, 0), (b"Sherlock [a-z]{4}", 13, 1, 0),
]


def test_every_directed_expression_takes_its_path():
    listed = {d.expr for d in CP.DIRECTED}
    for d in CP.DIRECTED:
        f = CP.class_fields(d.expr)
        assert CP.paths_of(f) == d.paths, (d.expr, f)
    for expr, plen, nalt, koff in FACTS:
        f = CP.class_fields(expr)
        assert expr in listed and (f.plen, f.nalt) == (plen, nalt), (expr, f)
        assert f.koff == koff if koff is not None else f.koff > 0, (expr, f)
    for expr in (b"x.{11}y", b"x.{12}y", b"[^a]{13}", b"x.{10}y"):
        assert CP.class_fields(expr).ascii_only == 1
    assert CP.class_fields(b"[^a]{13}").has_newline == 1
    by = {d.expr: d for d in CP.DIRECTED}
    assert CP.class_fields(CP.KOFF_POSITIVE).koff > 0 and CP.class_fields(CP.MULTI_ALT).nalt == 4 and by[CP.DENSE_OVERLAP].alphabet == CP.DENSE
    # the path model at the edges of its two conditions
    f = CP.class_fields(b"[a-z]{4}Sherlock")
    assert [CP.path_of(f, b) for b in (0, 3, 4, 15)] == ["memory:before-unit"] * 2 + ["view"] * 2
    f = CP.class_fields(b"[a-z]{5}Sherlock")
    assert [CP.path_of(f, b) for b in (0, 4, 5, 15)] == ["memory:before-unit"] * 2 + ["memory:long"] * 2


def test_the_limits_are_as_the_header_says():
    for expr in CP.OVER_LIMIT:
        compile_class_sequence(expr)  # (the oracle keeps up to 256 sets)
        assert xsg.regex_info(expr)[:2] == (0, 0) and xsg.regex_check(expr)[0] == 0, expr
        xsg.regex_dfa(expr)
    for expr, plen, nalt in CP.AT_LIMIT:
        assert xsg.regex_info(expr)[:2] == (plen, nalt) and xsg.regex_check(expr)[0] == plen, expr


def test_the_generator():
    """9..32 positions, at most 8 alternatives and 64 sets; neither parser refuses anything it makes; koff varies"""
    koffs, plens, nalts, dotty = Counter(), Counter(), Counter(), 0
    rng = np.random.default_rng(424242)
    for _ in range(400):
        expr = CP.rand_long_expr(rng)
        cs = compile_class_sequence(expr)
        f = CP.class_fields(expr)  # raises if the product's compiler refuses
        assert (cs.plen, bool(cs.ascii_only)) == (f.plen, bool(f.ascii_only)) and 9 <= f.plen <= 32 and f.nalt <= 8 and f.nalt * f.plen <= 64, (expr, f)
        assert len(expr) <= xsg.MAX_REGEX
        re.compile(expr)
        koffs[f.koff] += 1
        plens[f.plen] += 1
        nalts[f.nalt] += 1
        dotty += f.ascii_only
    assert set(plens) == set(range(9, 33)) and set(range(1, 7)) <= set(nalts) <= set(range(1, 8)), (plens, nalts)  # (9 positions x 7 = 63 sets; 8 alternatives: the directed list)
    assert set(koffs) == set(range(0, 25)), sorted(koffs)
    assert 60 < dotty < 200, dotty


def test_the_texts(texts, oracle):
    """what build_text promises: chunk sizes, a match at offset 0 of a chunk and one that ends at L, and the plants at the
    geometry edges -- for the directed texts every one the issue names, at B and at 2 B, each a match the oracle
    reports where it was planted"""
    for label, t in texts.items():
        f = t.info.f
        sizes = [b.size for b in t.case.blocks]
        assert 1 <= len(sizes) and max(sizes) <= CP.MAX_CHUNK, label
        directed = label.startswith("directed")
        assert sizes == CP.lengths_directed(f.plen, f.koff) if directed else len(sizes) <= 5, label
        allowed = set(P.GEOMETRY) | {CP.MAX_CHUNK, f.plen - 1, f.plen, f.plen + 31, f.plen + 32}
        assert set(sizes) <= allowed, label
        whats = Counter(w.split()[0] for _, _, w in t.plants)
        assert whats["member"] == 16 and whats["edge"] >= 12, (label, whats)
        assert whats["start"] >= 1, (label, whats)  # a whole match at offset 0 of a chunk
        assert all(t.case.blocks[c][:f.plen].tobytes() != b"" and CP.accepts(t.info, t.case.blocks[c][:f.plen].tobytes())
                   for c, pos, w in t.plants if w == "start" and pos == 0), label
        rels = CP.edge_rels(f.plen, f.koff)
        assert {-f.plen, -1, 0, -8 - f.koff, -1 - f.koff, -f.koff} | {j - f.koff for j in range(f.koff)} == set(rels)
        assert not [m for m in t.missed if m[0] == P.UNIT], (label, t.missed)
        if not directed:
            continue
        assert t.missed == [], (label, t.missed)
        assert whats["end"] >= 2 and whats["tail"] >= 3 and (whats["head"] >= 3 or f.koff == 0), (label, whats)
        edge = {}
        for c, pos, w in t.plants:
            if w.startswith("edge "):
                _, B, r, x = w.split()
                edge.setdefault((int(B), int(r), int(x[1:])), []).append((c, pos))
        want = {(B, r, x) for B in CP.EDGES for r in rels for x in (1, 2)}
        assert set(edge) == want and all(len(v) == 1 for v in edge.values()), (label, sorted(want ^ set(edge))[:8])
        true = CP.true_starts(oracle, t.info, t.case.blocks)
        for (B, r, x), [(c, pos)] in edge.items():
            assert pos % B == r % B and (B == P.UNIT or pos == x * B + r), (label, B, r, x, pos)
            assert CP.accepts(t.info, t.case.blocks[c][pos:pos + f.plen].tobytes()), (label, B, r, x)
            # reported there, unless a match that began in the bytes in front of it covers its start (`[^a]{13}`, the dense alphabets)
            assert pos in true[c] or any(pos - f.plen < s < pos for s in true[c]), (label, B, r, x, pos)


def test_the_census(texts, censuses):
    """every path, crossed with one / several alternatives and koff == 0 / > 0 where the combination exists, is reached
    by at least five expressions; and every expression reaches every path its fields allow"""
    cells = Counter()
    for label, t in texts.items():
        f = t.info.f
        got = CP.reached(t.info, censuses[label])
        assert set(got) == CP.paths_of(f), (label, t.info.expr, f, censuses[label])
        for p in got:
            cells[(p, f.nalt > 1, f.koff > 0)] += 1
    want = [("exact", False, False), ("inreg", False, False)]
    want += [("view", a, k) for a in (False, True) for k in (False, True)]
    want += [("memory:long", a, k) for a in (False, True) for k in (False, True)]
    want += [("memory:before-unit", a, True) for a in (False, True)]
    assert set(cells) == set(want), sorted(cells)
    assert all(cells[c] >= MIN_PER_CELL for c in want), sorted(cells.items())


def test_the_oracles_walk_is_re_finditer(texts, oracle):
    """leftmost, non-overlapping, for every long expression and its text, case-sensitive and not
    (tests/test_oracle_regex.py pins the oracle for expressions of up to 8 positions only)"""
    for label, t in texts.items():
        expr = t.info.expr
        for icase in (False, True):
            pyre = re.compile(expr, re.IGNORECASE if icase else 0)
            cs = compile_class_sequence(expr, icase)
            with_lines = not any(cs.accepts(k, 10) for k in range(cs.plen))
            total = 0
            for b in t.case.blocks:
                data = b.tobytes()
                hay = oracle.lower(b) if icase else b
                want = [m.start() for m in pyre.finditer(data)]
                assert oracle.regex_byte_offsets_match(hay, cs).tolist() == want, (label, expr, icase)
                assert oracle.regex_count(hay, cs, False) == len(want)
                total += len(want)
                if with_lines:  # one match per line: the first of every line that has one
                    first, nl = [], -1
                    for s in want:
                        if s > nl:
                            first.append(s)
                            e = data.find(b"\n", s + cs.plen)
                            nl = e if e >= 0 else len(data)
                    assert oracle.regex_byte_offsets_match(hay, cs, True).tolist() == first, (label, expr, icase)
            assert total > 0, (label, icase)


def test_every_fill_misleads_a_reader_that_looks_koff_bytes_before_a_chunk(texts, oracle):
    """tests/test_packing.py is about the bytes BEHIND a chunk; a window in the first koff bytes of a chunk sends the
    kernel koff bytes in FRONT of it.  Under every hostile fill a reader that starts there gets some chunk wrong: it
    finds a match that begins outside (`complete`; `stale` where the text in front allows), counts a newline that is
    not the chunk's (`nl`, `stale`), or meets a byte >= 0x80 (`hi`: a refusal for an ASCII-only expression).  Under
    zeros it sees nothing in front of the first chunk: the control."""
    picked = [(label, t) for label, t in texts.items() if t.info.f.koff > 0 and label.startswith("directed")]
    assert len(picked) >= 10
    for label, t in picked:
        f = t.info.f
        heads = [c for c, (j, k) in enumerate(t.case.plan) if j]
        assert heads and heads[0] == 0, (label, t.case.plan)
        small = [c for c, b in enumerate(t.case.blocks) if b.size <= 5000]
        for fill in P.FILLS:
            pk = P.pack_case(t.case, fill)
            found = {"match": 0, "nl": 0, "refused": 0, "hi": 0}
            for c in sorted(set(heads) | set(small)):
                straddle, extra_nl = CP.reader_koff_before(oracle, t, pk, c)
                o = pk.base + int(pk.offsets[c])
                if fill == "zero" and c == 0:
                    assert straddle == [] and extra_nl == 0, (label, "the control is hostile")
                found["refused"] += straddle is None
                found["match"] += bool(straddle)
                found["nl"] += bool(extra_nl)
                found["hi"] += bool((pk.host[o - f.koff:o] >= 0x80).any())
            if fill == "complete":
                assert found["match"] >= len(heads), (label, fill, found, heads)  # every head is completed from outside
            if fill == "nl":
                assert found["nl"] >= 1 + len(small) // 2, (label, fill, found)
            if fill == "hi":
                assert found["hi"] >= 1 and (found["refused"] >= 1 or not f.ascii_only), (label, fill, found)
            if fill == "stale":
                assert found["nl"] + found["match"] >= 1, (label, fill, found)
        # the chunk in front, where it has no pad, ends with the koff bytes that complete the window at the next chunk's start
        carried = [c for c in range(1, len(t.case.plan)) if t.case.blocks[c - 1].size % 16 == 0 and t.case.plan[c - 1][1] == f.koff == t.case.plan[c][0]]
        assert carried, (label, t.case.plan)
        # and the pad behind a chunk completes the match that would end at L + 1 (reader (a) of tests/packing.py)
        pk = P.pack_case(t.case, "complete")
        tails = [c for c, (j, k) in enumerate(t.case.plan) if k == f.plen - 1 and t.case.blocks[c].size % 16 and t.case.blocks[c].size <= 5000]
        assert tails, label
        for c in tails:
            inside, _ = P.reader_past_end(oracle, t.case.kind, pk, c)
            assert inside != P.spans(oracle, t.case.kind, t.case.blocks[c]), (label, c)
