"""The host side of a literal list (include/xsg.h: xsg_set_literals, xsg_literals_info) -- no GPU: what the list compiler
accepts and refuses, the filter's no-false-negative property, the compiler and the verify step under the sanitizers as a
stand-alone program, tests/set_model.py pinned to the oracle, and xsgrep's argument handling."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import set_cases as SC
import set_model
import xsg
from gpu_util import oracle_rx_all_modes
from xs_oracle import RegexProgram, UnsupportedRegex

ROOT = Path(__file__).resolve().parents[1]
IC = xsg.FLAG_IGNORE_CASE


def info(literals, flags=0, final_newline=False):
    return xsg.literals_info(xsg.literal_list(literals) + (b"\n" if final_newline else b""), flags)


def test_what_the_list_compiler_accepts():
    assert info([b"Sherlock"]) == {"count": 1, "min_len": 8, "max_len": 8, "gram": 4, "filter_bits_set": 1}
    assert info([b"ab", b"abc"], final_newline=True) == {"count": 2, "min_len": 2, "max_len": 3, "gram": 2, "filter_bits_set": 1}
    assert info([b"foo", b"bar", b"foo", b"foo"])["count"] == 4  # duplicates are allowed
    many = [b"w%04d" % i for i in range(xsg.MAX_LITERALS)]
    assert info(many)["count"] == xsg.MAX_LITERALS and info(many, final_newline=True)["count"] == xsg.MAX_LITERALS
    long = bytes(range(11, 11 + 245)) + b"0123456789"
    assert len(long) == xsg.MAX_LITERAL_BYTES and info([long, b"abcde"])["max_len"] == 255
    for shortest, g in ((1, 1), (2, 2), (3, 3), (4, 4), (9, 4)):
        got = info([b"x" * 20, b"q" * shortest, b"y" * 12])
        assert (got["count"], got["min_len"], got["max_len"], got["gram"]) == (3, shortest, 20, g)
    for flags in (xsg.FLAG_EXACT_TAIL, IC, xsg.FLAG_INVERT, xsg.flag_context(2, 3), xsg.FLAG_INVERT | xsg.flag_context(4095, 4095) | IC):
        assert info([b"a", b"bc"], flags)["gram"] == 1


@pytest.mark.parametrize("lst,flags,word", [
    (b"", 0, "empty"),
    (b"a\n\nb", 0, "empty literal"),
    (b"\na", 0, "empty literal"),
    (b"a\n\n", 0, "empty literal"),
    (b"\n".join(b"w%04d" % i for i in range(xsg.MAX_LITERALS + 1)), 0, "more than 4096"),
    (b"ok\n" + b"x" * (xsg.MAX_LITERAL_BYTES + 1), 0, "longer than 255"),
    (b"\n".join([b"y" * 255] * 129), 0, "longer than 32768"),  # 129 * 256 - 1 bytes > XSG_MAX_PATTERN
    (b"a|b", xsg.FLAG_REGEX, "XSG_FLAG_REGEX"),
    (b"a", 0x10, "unknown pattern flags"),
    (b"a", 0x80, "unknown pattern flags"),
])
def test_what_the_list_compiler_refuses(lst, flags, word):
    with pytest.raises(xsg.XsgError) as e:
        xsg.literals_info(lst, flags)
    assert e.value.code == xsg.EINVAL and word in str(e.value)


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("shortest", [1, 2, 3, 4, 7])
def test_the_filter_has_no_false_negative(shortest, icase):
    """the gram bit of every literal is set, and no other bit: filter_bits_set counts the distinct hashes"""
    rng = np.random.Generator(np.random.PCG64(100 + shortest))
    for n in (1, 5, 300, 4096):
        lits = []
        for i in range(n):
            length = shortest if i == 0 else int(rng.integers(shortest, 8 if n == 4096 else 41))  # (4096 of them within XSG_MAX_PATTERN)
            lit = bytes(int(x) for x in rng.integers(0, 256, size=length)).replace(b"\n", b"\x0b")
            lits.append(lit)
        d, filt = xsg.literals_info(xsg.literal_list(lits), IC if icase else 0, with_filter=True)
        g = d["gram"]
        assert g == min(shortest, 4) and d["count"] == n
        bits = set()
        for lit in lits:
            gram = (lit.lower() if icase else lit)[:g]  # (bytes.lower folds ASCII letters only)
            h = xsg.literal_gram_hash(int.from_bytes(gram, "little"), g)
            assert (int(filt[h >> 5]) >> (h & 31)) & 1, (lit, h)
            bits.add(h)
        assert d["filter_bits_set"] == len(bits) == sum(bin(int(w)).count("1") for w in filt)


def test_compiler_filter_and_verify_step_under_the_sanitizers(tmp_path):
    """tests/cpp/set_selftest.cpp includes csrc/xsg_set.h/.cpp: a stand-alone program, nothing is loaded into Python"""
    exe = tmp_path / "set_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "set_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "set_selftest ok" in r.stdout


def _utf8_cases():
    cases = [("text-%d-%s" % (k, "icase" if ic else "plain"), SC.text_blocks, SC.word_list(k), ic)
             for k in SC.LIST_SIZES for ic in (False, True)]
    cases += [("order-" + name, (lambda b=blocks: b), lits, False) for name, lits, blocks in SC.ORDER_CASES]
    cases += [("align-%d" % g, SC.align_blocks, SC.align_list(g), False) for g in (1, 2, 3, 4)]
    cases += [("end-%d-%s" % (g, "icase" if ic else "plain"), (lambda g=g: SC.end_blocks(g)), SC.END_LITS[g], ic)
              for g in (1, 2, 3, 4) for ic in (False, True)]
    cases += [("dense", SC.dense_blocks, SC.DENSE_LIST, False)]
    return cases


@pytest.mark.parametrize("name,blocks,lits,icase", _utf8_cases(), ids=[c[0] for c in _utf8_cases()])
def test_the_model_is_the_oracle(oracle, name, blocks, lits, icase):
    """tests/set_model.py against the oracle's regex reader on E(S), on every case of tests/test_gpu_set.py that the
    reader accepts; XSG_MATCHES' strings against the walk of the oracle's own expression"""
    blocks = list(blocks())
    prog = RegexProgram(set_model.expression(lits), icase)
    assert set_model.all_modes(blocks, lits, icase) == oracle_rx_all_modes(oracle, blocks, prog)
    strings, offsets, lengths = set_model.matches(blocks[:2], lits, icase)
    want, goff = [], 0
    for b in blocks[:2]:
        d, pos = b.tobytes(), 0
        while (m := prog.re.search(d, pos)) is not None:
            want.append((goff + m.start(), d[m.start():m.end()]))
            pos = m.end()
        goff += len(d)
    assert list(zip(offsets, strings)) == want and lengths == [len(s) for s in strings]


@pytest.mark.parametrize("icase", [False, True], ids=["plain", "icase"])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_the_chunk_end_layout_is_hostile(g, icase):
    """the packed buffer of test_gpu_set.py::test_chunk_ends, before a GPU sees it: a reader that goes on past a chunk's
    end finds a match more in every chunk the plan cuts (the completing bytes do lie behind the end) and nothing more in
    any other; what it finds more begins inside the chunk and ends behind it"""
    import packing
    blocks, lits = SC.end_blocks(g), SC.END_LITS[g]
    packed = packing.pack_tight(blocks, SC.end_fill(g))
    cut = SC.end_cut_chunks(g)
    assert len(cut) >= (6 if g == 1 else 12)
    tails = set()
    for c, b in enumerate(blocks):
        alone = set_model.Occurrences(b, lits, icase).spans()
        more = [s for s in SC.end_naive_spans(g, icase, packed, c) if s not in alone]
        assert bool(more) == (c in cut), (c, more)
        for start, n in more:
            assert start < b.size < start + n
            tails.add((lits.index(b.tobytes()[start:].lower() + SC.end_plan(g)[c][1]), b.size - start, b.size % 16 == 0))
    # `needle` cut after 5, 1 and 3 bytes, each completed by a pad and by the chunk that follows
    assert {(1, k, nopad) for k in (5, 1, 3) for nopad in (False, True)} <= tails
    if g > 1:  # the shortest literal cut one byte short: its only gram straddles the end
        assert {(0, g - 1, False), (0, g - 1, True)} <= tails
    # whole occurrences that end exactly at a chunk's end, and stale matches in the pads behind chunks
    assert blocks[0].tobytes().endswith(lits[1]) and blocks[1].tobytes().endswith(lits[0])
    pads = b"".join(packed.host[packed.base + int(o) + int(n):packed.base + int(o) + packing.round_up16(n)].tobytes()
                    for o, n in zip(packed.offsets, packed.lengths))
    assert lits[1] in pads and lits[0] in pads


def test_the_oracle_refuses_what_only_the_model_reads(oracle):
    with pytest.raises(UnsupportedRegex):
        RegexProgram(set_model.expression(SC.RAW_LIST))
    blocks = SC.raw_blocks()
    want = set_model.all_modes(blocks, SC.RAW_LIST)
    assert SC.expected(oracle, blocks, SC.RAW_LIST) == want
    assert want["match_byte_offsets"][:4] == [100, 5000, 5002, SC.TILE - 1]  # caf\xe9, \xff\xfe twice, one across the tile edge
    assert set_model.all_modes(blocks, SC.RAW_LIST, True)["count_matches"] == want["count_matches"] + 1  # CAF\xe9


def test_the_binding_and_the_header_agree():
    header = (ROOT / "include" / "xsg.h").read_text()
    for name in ("xsg_set_literals", "xsg_literals_info", "xsg_host_searcher_create_list"):
        assert name in xsg.EXPORTS and name + "(" in header
    assert "#define XSG_MAX_LITERALS %du" % xsg.MAX_LITERALS in header
    assert "#define XSG_MAX_LITERAL_BYTES %du" % xsg.MAX_LITERAL_BYTES in header
    assert "#define XSG_LITERAL_FILTER_BYTES %du" % xsg.LITERAL_FILTER_BYTES in header
    lib = xsg.load()
    o = xsg.JobOpts()
    o.pattern_is_list = 7
    lib.xsg_job_opts_init(o)
    assert o.pattern_is_list == 0 and o.struct_size == 56 and xsg.JobOpts.pattern_is_list.offset == 48
    assert lib.xsg_abi_version() == 4


@pytest.mark.parametrize("args,word", [
    (["-e", "a", "-e", "b", "FILE"], "needs -F"),
    (["-E", "-e", "a", "-e", "b", "FILE"], "needs -F"),
    (["-F", "-x", "-e", "a", "-e", "b", "FILE"], "excludes -x"),
    (["-F", "-e", "a", "-e", "", "FILE"], "empty pattern"),
    (["-F", "-f", "/nonexistent/words", "FILE"], "cannot read"),
    (["-F", "-e", "a", "-e", "b"], "usage"),
    (["-F", "-e", "a", "-e", "b", "FILE", "MORE"], "unexpected argument"),
])
def test_xsgrep_refuses_before_it_needs_a_device(args, word):
    exe = ROOT / "tools" / "build" / "xsgrep"
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)


def test_xsgrep_reads_a_pattern_file_without_patterns_as_an_error(tmp_path):
    words = tmp_path / "none.txt"
    words.write_bytes(b"")
    r = subprocess.run([str(ROOT / "tools" / "build" / "xsgrep"), "-F", "-f", str(words), "FILE"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "no pattern" in r.stderr
