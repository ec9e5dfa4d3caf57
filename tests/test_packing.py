"""tests/packing.py without a GPU: every layout that tests/test_gpu_packed.py binds keeps include/xsg.h's requirements
to the letter, and every hostile layout IS hostile -- for each (pattern kind, fill) there is a chunk on which a model
of a kernel that reads past the chunk's ends (packing.reader_*) reports something else than the search of the chunk
alone.  A fill that no reader can tell from zeros would test nothing on the GPU."""
import numpy as np
import pytest

import packing as P
from xs_oracle import RegexProgram

KIND_IDS = [k.name for k in P.KINDS]


@pytest.fixture(scope="module")
def cases():
    return {k.name: P.build_case(k) for k in P.KINDS}


def bindings(case):
    """everything the GPU file binds of a case: the shard and the four single chunks"""
    return [("shard", case)] + [(f"single {n}", P.single_case(case, n)) for n in P.SINGLES]


def test_the_tables():
    """the fixed tables of the issue: lengths, kinds, fills"""
    names = [k.pat for k in P.KINDS]
    for n in (1, 2, 4, 8, 16, 110):
        assert sum(1 for k in P.KINDS if k.family == "lit" and len(k.pat) == n and not k.flags & P.IC) >= 2, n
    assert any(len(p) > 1024 for p in names) and P.LIT110.count(b"\n") == 0 and P.LIT1500.count(b"\n") == 0
    for pat in (b"that", b"aa", b"street\nthe"):
        assert {k.flags for k in P.KINDS if k.pat == pat} == {0, P.X}, pat
    assert sum(1 for k in P.KINDS if k.flags & P.IC) == 2
    for expr in (b"She[r ]lock", b"t.e", b"[^a-z]he", b"colou?r", b"\\w+ing", b"Sher.*mes", b"(?m)^She", b"(?m)locked$", b"She\\s+lock"):
        assert expr in names, expr
    for k in P.KINDS:
        if k.family == "rx" and not k.pat.startswith(b"(?m)"):
            assert RegexProgram(k.pat).ascii_only == k.ascii_only, k.name
        lengths = P.lengths_of(k)
        p = P.plen_of(k)
        assert set(P.GEOMETRY) | {p - 1, p, p + 31, p + 32} == set(lengths) and set(P.SINGLES) <= set(lengths)
    assert P.FILLS == ("zero", "nl", "hi", "stale", "complete")


@pytest.mark.parametrize("name", KIND_IDS)
def test_layout_keeps_the_headers_requirements(cases, name):
    case = cases[name]
    for what, sub in bindings(case):
        assert [b.size for b in sub.blocks] == (P.lengths_of(case.kind) if what == "shard" else [int(what.split()[1])])
        for fill in P.FILLS:
            pk = P.pack_case(sub, fill)
            off, ln = pk.offsets.astype(np.int64), pk.lengths.astype(np.int64)
            assert pk.base % 16 == 0 and pk.base >= P.GUARD and pk.host.size == pk.base + pk.capacity + P.GUARD
            assert (off % 16 == 0).all(), "an offset is no multiple of 16"
            assert (np.diff(off) >= 0).all() and off[0] == 0, "offsets do not increase"
            ends = off + (ln + 15) // 16 * 16
            assert (ends[:-1] == off[1:]).all(), "chunks overlap or leave a gap: not tightly packed"
            assert ends[-1] == pk.capacity, "the last chunk's rounded end is not the capacity"
            for c, b in enumerate(sub.blocks):
                o = pk.base + int(off[c])
                assert (pk.host[o:o + b.size] == b).all(), f"{fill}: chunk {c} differs from its block"
    ends_nl = [bool(b.size) and b[-1] == 10 for b in case.blocks]
    assert any(ends_nl) and not all(ends_nl[c] for c, b in enumerate(case.blocks) if b.size)
    pk = P.pack_case(case, "nl")
    assert any(b.size and b[-1] != 10 and b.size % 16 and pk.host[pk.base + int(pk.offsets[c]) + b.size] == 10
               for c, b in enumerate(case.blocks)), "no unterminated chunk with a '\\n' pad byte right behind it"


def test_fills_do_not_reach_the_truth(cases):
    """the blocks of a case are the same objects whatever the fill: the truth cannot depend on it (and `zero` differs
    from every hostile fill somewhere in the pads, or the control would control nothing)"""
    for case in cases.values():
        zero = P.pack_case(case, "zero")
        for fill in P.HOSTILE:
            pk = P.pack_case(case, fill)
            assert pk.capacity == zero.capacity and (pk.offsets == zero.offsets).all()
            inside = np.zeros(pk.host.size, dtype=bool)
            for c, b in enumerate(case.blocks):
                o = pk.base + int(pk.offsets[c])
                inside[o:o + b.size] = True
            assert (pk.host[inside] == zero.host[inside]).all()
            pads = ~inside
            pads[:pk.base] = pads[pk.base + pk.capacity:] = False
            assert (pk.host[pads] != zero.host[pads]).any(), (case.kind.name, fill)


@pytest.mark.parametrize("name", KIND_IDS)
def test_every_hostile_fill_is_hostile(cases, oracle, name):
    case = cases[name]
    kind = case.kind
    for fill in P.HOSTILE:
        pk = P.pack_case(case, fill)
        h = P.hostility(oracle, kind, pk, case.blocks)
        where = f"{name} {fill}: {({k: len(v) for k, v in h.items()})}"
        # (d_line -- the byte in front of a chunk is no '\n' -- holds under zeros too: it proves nothing about a fill)
        assert any(v for k, v in h.items() if k != "d_line"), where
        if fill == "complete":
            # a match that the bytes outside finish or begin; a one-byte needle cannot straddle an edge: there the pad holds it whole
            assert (h["a"] or h["d"]) if len(kind.witness) > 1 else h["pad"], where
            if len(kind.witness) > 1:
                assert len(h["a"]) >= 3 or kind.pat in (P.LIT1500,), where
        if fill == "nl":
            assert len(h["b"]) >= 10, where
        if fill == "hi":
            # `hi` is hostile through reader (c) alone: 0xFF is no '\n' and part of no witness, so it can change a
            # result only where the non-ASCII verdict is taken -- the ASCII-only kinds; for the others it is a second control
            assert len(h["c"]) >= 10 and not (h["b"] or h["pad"]), where
        if fill == "stale":
            # (a needle of 1500 bytes finds no room in a pad or among the plen + 31 bytes behind a chunk: newlines only)
            assert h["b"] and (h["a"] or h["pad"] or h["d"] or kind.pat == P.LIT1500), where
    zero = P.hostility(oracle, kind, P.pack_case(case, "zero"), case.blocks)
    # (the searching readers see the neighbouring chunks as well, whatever the fill; the others see zeros as nothing)
    assert not (zero["b"] or zero["c"]), f"{name}: the control is hostile: {zero}"


def test_single_chunk_bindings_are_hostile_too(cases, oracle):
    """the four lengths bound alone: between them every (kind, fill) pair has a chunk a reader gets wrong"""
    for name, case in cases.items():
        for fill in P.HOSTILE:
            found = {}
            for n in P.SINGLES:
                sub = P.single_case(case, n)
                h = P.hostility(oracle, case.kind, P.pack_case(sub, fill), sub.blocks, max_len=40_000)
                for k, v in h.items():
                    found[k] = found.get(k, 0) + len(v)
            assert any(v for k, v in found.items() if k != "d_line"), (name, fill, found)
            if fill == "nl":
                assert found["b"] >= 2, (name, found)  # (16384 has no pad; 15, 4097 and 32769 do)


def test_the_pipeline_file_leaves_hostile_bytes_behind_its_chunks(oracle):
    """the reused device buffer of the file pipeline, simulated: buf[:len_k] = chunk_k in chunk order.  For every
    pipeline pattern reader (a) or (b), fed what then lies behind a chunk's end, gets some chunk wrong."""
    chunks = P.pipeline_chunks()
    sizes = [len(c) for c in chunks]
    assert all(11_000 < n < 13_000 for n in sizes[0::2]) and all(4096 <= n < 4200 for n in sizes[1::2])
    snaps = P.reused_buffer(chunks)
    for pat, flags, _ in P.PIPELINE_PATTERNS:
        kind = next(k for k in P.KINDS if k.pat == pat and k.flags == flags)
        a, b = [], []
        for i, (c, snap) in enumerate(zip(chunks, snaps)):
            pk = P.as_packed(snap, len(c))
            inside, in_pad = P.reader_past_end(oracle, kind, pk, 0)
            if inside != P.spans(oracle, kind, P.u8(c)):
                a.append(i)
            naive, true = P.reader_newlines(pk, 0)
            if naive != true:
                b.append(i)
        assert a or b, pat
        assert len(b) == 3, b  # every long chunk but the first: the '\n' of the one before lies in its pad
        if pat in (b"street\nthe", b"that", b"colou?r"):
            assert a, pat  # `the` behind `street\n`; the lossy tail zone moved off `ththat`; `ur` behind `colo`


def test_the_host_sequences_leave_hostile_bytes(oracle):
    """the one-slot host searcher's buffer, simulated, for every kind the GPU file runs: behind at least two of the four
    short chunks a reader goes wrong.  A witness of two bytes or more is finished by the long chunk's bytes (reader (a))
    or followed by its '\\n' (reader (b)); a one-byte needle cannot straddle the end: there the '\\n' behind the odd
    short chunks misleads reader (b), and the needle itself lies in the pad of every short chunk."""
    for kind in P.KINDS:
        chunks = P.host_sequence(kind)
        snaps = P.reused_buffer([c.tobytes() for c in chunks])
        a = b = pad = 0
        for i in range(1, len(chunks), 2):
            pk = P.as_packed(snaps[i], chunks[i].size)
            assert chunks[i].size % 16, "a short chunk without a pad"
            inside, in_pad = P.reader_past_end(oracle, kind, pk, 0)
            naive, true = P.reader_newlines(pk, 0)
            a += inside != P.spans(oracle, kind, chunks[i])
            b += naive != true
            pad += bool(in_pad)
            if kind.ascii_only:
                assert P.reader_non_ascii(pk, 0), kind.name
        if len(kind.witness) > 1:
            assert a + b >= 2 and (a or kind.ascii_only), (kind.name, a, b, pad)
        else:
            assert b >= 2 and pad >= 2, (kind.name, a, b, pad)
