"""The generator of tests/call_sequences.py reaches what tests/test_gpu_call_sequences.py relies on: checked here from the
committed sequences themselves, with the oracle alone and without a GPU."""
import ast

import pytest

import call_sequences as cs
import xsg

BINDS = ("bind", "invalidate")


@pytest.fixture(scope="module")
def walks(oracle):
    return [cs.walk(ops, oracle) for ops in cs.sequences()]  # (raises Ambiguous if a sequence leaves what the header decides)


def test_sequences_are_reproducible_literals(walks):
    first = cs.sequences()
    cs._sequences = None
    assert cs.sequences() == first, "the generator is not a pure function of its seeds"
    for ops in first:
        assert 100 <= len(ops) <= 200
        for op in ops:
            assert ast.literal_eval(repr(op)) == op
        assert ops[0][:2] == ("bind", "create")
    sizes = [cs.nbytes_of(d) for d in cs.DATA if d != "runs"]
    assert max(sizes) < 400_000, sizes  # the oracle answers in milliseconds; `runs` (the overflow refusal) is the one exception


def test_the_pool_covers_every_kind_of_pattern():
    pool = cs.pool()
    lits = [(p, f) for p, f, _ in pool if not f & cs.R]
    for lo, hi in ((1, 3), (4, 4), (5, 7), (8, 8), (9, 1024), (1025, xsg.MAX_PATTERN)):
        assert any(lo <= len(p) <= hi and not cs.has_border(p) for p, f in lits), (lo, hi)
    assert {b"aa", b"abab", b"that"} <= {p for p, f in lits if cs.has_border(p)}
    assert any(b"\n" in p for p, f in lits)
    for flag in (cs.I, cs.X):
        assert any(f & flag for p, f in lits)
    assert any(not f & cs.X for p, f in lits)
    for p, f, fam in pool:
        if fam in ("lit_mask1", "lit_one", "lit_mask2", "lit_two", "lit_long"):
            assert not cs.has_border(p.lower()) and not f & (cs.R | cs.V), p
            assert fam == ("lit_mask1" if len(p) < 4 else "lit_one" if len(p) == 4 else "lit_mask2" if len(p) < 8 else
                           "lit_two" if len(p) == 8 else "lit_long"), p
        if fam == "bordered":
            assert cs.has_border(p.lower()) and not f & (cs.R | cs.V)
        if fam == "inverted":
            assert f & cs.V
        if fam == "classseq":
            assert xsg.regex_check(p, f & ~cs.R)[0] > 0, p  # fixed length: the scan kernel's matcher
        if fam in ("rx_prefix", "rx_factor", "anchored"):
            body = p[4:].lstrip(b"^").rstrip(b"$") if p.startswith(b"(?m)") else p
            info = xsg.regex_dfa(body, f & ~cs.R)[0]
            if fam == "rx_prefix":
                assert info.prefix_positions > 0, p
            if fam == "rx_factor":
                assert info.prefix_positions == 0 and info.factor_positions > 0, p
    assert {p[:5] for p, f, fam in pool if fam == "anchored"} >= {b"(?m)^"} and any(p.endswith(b"$") and p[4:5] != b"^" for p, f, fam in pool if fam == "anchored")
    assert any(p[4:5] == b"^" and p.endswith(b"$") for p, f, fam in pool if fam == "anchored")
    inv = [(p, f) for p, f, fam in pool if fam == "inverted"]
    assert any(f & cs.R for p, f in inv) and any(not f & cs.R for p, f in inv)
    for p in cs.ASCII_ONLY:
        assert xsg.regex_info(p)[2] if xsg.regex_check(p)[0] else xsg.regex_dfa(p)[0].ascii_only, p
    for p, f in cs.REFUSED_PATTERNS:
        assert f & cs.V and (b"\n" in p or b"\\s" in p)


def test_every_ordered_pair_of_operation_classes_occurs(walks):
    seen = set()
    for w in walks:
        cl = [cs.op_class(op, e) for _, op, e in w]
        seen.update(zip(cl, cl[1:]))
    forbidden = set()  # include/xsg.h forbids no pair of these classes: a refusal leaves the binding usable
    missing = {(a, b) for a in cs.CLASSES for b in cs.CLASSES} - seen - forbidden
    assert not missing, sorted(missing)


def test_every_call_form_and_toggle_occurs(walks):
    ops = [op for w in walks for _, op, _ in w]
    for via in cs.COUNT_VIAS:
        for tag in ("matches", "lines"):
            for nl in (False, True):
                assert ("count", tag, nl, via) in ops, (tag, nl, via)
    for kind in cs.LIST_KINDS:
        assert ("list", kind) in ops
    for kind in cs.REBIND_KINDS:
        for layout in (0, 1, 2):
            assert any(op[:2] == ("bind", kind) and op[3] == layout for op in ops), (kind, layout)
    assert any(op[0] == "set_line_base" for op in ops)
    for mode in cs.MODES:
        assert any(op[:2] == ("time_scan", mode) for op in ops), mode
    assert not any(op[0] == "tune" for op in ops), "xsg_shard_tune does nothing below 1 GiB: it would count as a measuring call and be none"
    for name, values in cs.TOGGLES.items():
        for v in values:
            assert ("toggle", name, v) in ops, (name, v)
    for p, f, _ in cs.pool():
        assert ("set_pattern", p, f) in ops, (p, f)
    refusals = {e.refusal for w in walks for _, _, e in w}
    assert refusals >= set(cs.REFUSALS) | {"bad_pattern", "nl_async"}, refusals
    kinds = {(e.refusal, e.kind) for w in walks for _, _, e in w if e.refusal in ("nonascii", "overflow")}
    assert kinds >= {("nonascii", "err"), ("nonascii", "poison"), ("nonascii", "status"), ("overflow", "poison"), ("overflow", "status")}, kinds


def test_toggles_are_restored_and_larger_bindings_are_what_they_claim(walks):
    for w in walks:
        env, tiles, cur = {}, 0, None
        for _, op, _ in w:
            if op[0] == "toggle":
                assert op[1] in cs.TOGGLES
                env[op[1]] = op[2]
            if op[0] == "bind":
                n = cs.ntiles_of(op[2])
                if op[1] == "smaller":
                    assert cs.nbytes_of(op[2]) < cs.nbytes_of(cur)
                if op[1] == "larger_fit":
                    # "fits" is meant for d_tile_cnt and d_tile_last, one u32 per tile: DevBuf rounds an allocation up to 256
                    # bytes, so 64 tiles (d_tile_sum, kWaves words per tile, may grow earlier; which buffers really kept their
                    # size is asserted on the GPU: test_rebind_after_a_list_pass_inside_the_grown_buffers_and_past_them)
                    assert cs.ntiles_of(cur) < n <= 256 // 4
                if op[1] == "larger_nofit":
                    assert tiles <= 64 < n
                if op[1] == "one_chunk":
                    assert len(cs.blocks_of(op[2])) == 1 and n > 1
                if op[1] == "empty":
                    assert cs.nbytes_of(op[2]) == 0
                if op[1] == "same_addr":
                    assert op[2] != cur and [b.size for b in cs.blocks_of(op[2])] == [b.size for b in cs.blocks_of(cur)]
                    assert any((a != b).any() for a, b in zip(cs.blocks_of(op[2]), cs.blocks_of(cur)))
                tiles, cur = max(tiles, n), op[2]
            if op[0] == "invalidate":
                assert any((a != b).any() for a, b in zip(cs.blocks_of(op[1]), cs.blocks_of(cur)))
                nl = [(a == 10).nonzero()[0].tolist() for a in cs.blocks_of(op[1])]
                assert nl != [(a == 10).nonzero()[0].tolist() for a in cs.blocks_of(cur)], "the newline positions must move"
                cur = op[1]
        assert all(v is None for v in env.values()), env


def predecessor_kind(op, e):
    if op[0] == "bind" and op[1] in cs.REBIND_KINDS:
        return "rebind:" + op[1]
    if op[0] == "invalidate":
        return "invalidate"
    if op[0] == "time_scan":
        return "measure"
    if op[0] == "toggle":
        return "toggle"
    if e.refusal in cs.REFUSALS:
        return "refuse:" + e.refusal
    return None


def test_every_result_follows_every_rebind_refusal_measurement_and_toggle(walks):
    """DIRECTLY after it -- except behind the two refusals that leave the context without a usable pattern (XSG_ESTATE: no
    pattern at all; non-ASCII data: every search of the expression is refused): there one xsg_set_pattern stands between,
    and no rebind."""
    seen = set()
    for w in walks:
        for k in range(len(w) - 1):
            _, op, e = w[k]
            pred = predecessor_kind(op, e)
            if pred is None:
                continue
            nxt = k + 1
            if pred in ("refuse:estate", "refuse:nonascii") and w[nxt][1][0] == "set_pattern" and w[nxt][2].kind == "none":
                nxt += 1
            if nxt < len(w):
                rk = cs.result_kind(w[nxt][1], w[nxt][2])
                if rk is not None:
                    seen.add((pred, rk))
    want = {(p, r) for p in cs.PREDECESSORS for r in cs.RESULT_KINDS}
    assert cs.UNREACHABLE_PRED == {("refuse:invert_match", "list:match_byte_offsets")}
    missing = want - seen - cs.UNREACHABLE_PRED
    assert not missing, sorted(missing)


def test_every_ordered_pair_of_pattern_families_occurs_on_one_binding(walks):
    """f1 searched, xsg_set_pattern, f2 searched, and no rebind or invalidate anywhere between"""
    seen = set()
    for w in walks:
        prev, cur, searched = None, None, False
        for _, op, e in w:
            if op[0] in BINDS:
                prev, searched = None, False
                continue
            if op[0] == "set_pattern":
                if searched:
                    prev = cur
                cur = cs.family_of(op[1], op[2]) if e.kind == "none" else None
                if cur is None:
                    prev = None
                searched = False
            elif cs.result_kind(op, e) is not None and cur is not None:
                if prev is not None:
                    seen.add((prev, cur))
                searched = True
    missing = {(a, b) for a in cs.FAMILIES for b in cs.FAMILIES} - seen
    assert not missing, sorted(missing)


def wants_newlines(op, inverted):
    """does this call make the library count the binding's newlines: it asks for them, the complement needs them, or it
    times the newline-counting kernel (which writes the per-tile counts, though it does not mark them cached)"""
    if op[0] == "time_scan":
        return bool(op[1] & xsg.WITH_NEWLINES)
    if op[0] == "count":
        return op[2] or inverted
    return op[0] == "list" and (op[1] in ("line_indices", "result_newlines") or inverted)


def test_every_family_is_the_first_to_produce_newline_counts(walks):
    seen = set()
    for w in walks:
        first, fam = None, None  # family of the first pass of this binding that wanted newline counts
        for _, op, e in w:
            if op[0] in BINDS:
                first = None
            elif op[0] == "set_pattern":
                fam = cs.family_of(op[1], op[2]) if e.kind == "none" else None
            elif op[0] == "list" and e.kind == "value" and fam == "inverted" and first is None:
                first = fam  # (the replay compares a synchronous count first: under XSG_FLAG_INVERT that one counts the newlines)
            elif op[0] == "time_scan" and wants_newlines(op, False) and first is None:
                first = fam
            elif cs.result_kind(op, e) is not None and wants_newlines(op, fam == "inverted"):
                if first is None:
                    first = fam
                elif fam != first and (op[0] == "count" and op[2] or op[0] == "list" and op[1] in ("line_indices", "result_newlines")):
                    seen.add(first)
    assert seen >= set(cs.FAMILIES), set(cs.FAMILIES) - seen


def test_at_least_half_of_the_expected_results_are_not_empty(walks):
    results = [e for w in walks for _, op, e in w if cs.result_kind(op, e) is not None]
    assert len(results) >= 500
    assert 2 * sum(e.value_nonzero for e in results) >= len(results), (sum(e.value_nonzero for e in results), len(results))
    checked = 0
    for w in walks:  # under XSG_FLAG_INVERT a result counts only if the plain and the inverted lists are both non-empty
        m = cs.Model()
        for _, op, e in w:
            m.apply(op)
            if cs.result_kind(op, e) is not None and m.inverted() and e.value_nonzero:
                modes = cs.expected_modes(None, m.data, m.layout, m.pattern, m.flags)  # (memoised by the walk above)
                assert modes["plain_count_lines"] > 0 and modes["count_lines"] > 0
                checked += 1
    assert checked >= 20, checked


def test_a_stale_tile_last_word_changes_the_walk(oracle):
    """the data of test_gpu_call_sequences.py::test_tile_last_across_the_epoch_wrap: B's count from the chunk's start (what
    a pass that reads only its own epoch's words computes) differs from its count from the end of A's last match (what a
    word of A's pass, taken for this pass's, would make it)"""
    d, a, a_end, b = cs.epoch_wrap_case()
    assert d.size <= cs.TILE and a_end < 1 << 16
    za, zb = d.size - (len(a) + 31), d.size - (len(b) + 31)
    a_at = [int(x) for x in oracle.byte_offsets_match(d, a)]
    assert a_at and a_at[-1] + len(a) == a_end and a_at[-1] < za, "A's last match belongs to the bulk scan and ends at a_end"
    occ = [i for i in range(d.size - len(b) + 1) if d[i:i + len(b)].tobytes() == b]
    assert occ and all(o >= zb for o in occ), "B has no occurrence before its tail zone"
    fresh, stale = cs.walk_from(oracle, d, b, 0), cs.walk_from(oracle, d, b, a_end)
    assert fresh == oracle.count(d, b, False) == 1 and stale == 0, (fresh, stale)
    # ... and A's own count needs ITS word: behind its last bulk match the walk finds nothing more, though a second `aab` stands
    # in the tail zone (the lossy scalar search loses it); a pass that did not read the word as its own would report it
    assert oracle.count(d, a, False) == len(a_at) and cs.walk_from(oracle, d, a, a_end) == 0
    assert d[a_end + 1:a_end + 4].tobytes() == a and a_end + 1 not in a_at and a_end + 1 >= za
