"""Without a GPU: every binding of tests/gate_wave_cases.py reaches the edge of the wave form's dealing it is named after --
which wave owns which candidate, how many (tile, span) pairs that wave holds (the locator's masks by span_sketch_model),
and that in the last round some wave of the grid has no group while another has."""
import pytest

import gate_wave_cases as gw
import span_sketch_model as spm
from gate_wave_cases import GROUP, TILE, WAVES


@pytest.fixture(scope="module")
def text():
    return gw.make_text()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return spm.load(tmp_path_factory.mktemp("gate_wave_cases_model"))


def holding_tiles(blocks, pat):
    """binding tile -> number of window starts (filter window at 0) in it"""
    out, t0 = {}, gw.tile0_of(blocks)
    for b, first in zip(blocks, t0):
        for o in spm.occurrences(b, pat):
            out[first + o // TILE] = out.get(first + o // TILE, 0) + 1
    return out


def pairs_by_wave(model, blocks, pat, grid):
    """(workgroup, wave) -> [(round, tile, span mask)] of the candidates that hold an occurrence"""
    ntiles, t0, out = sum(gw.tiles_of(blocks)), gw.tile0_of(blocks), {}
    held = holding_tiles(blocks, pat)
    for b, first in zip(blocks, t0):
        sp = None
        for t in sorted(t for t in held if first <= t < first + (int(b.size) + TILE - 1) // TILE):
            sp = spm.build(model, b) if sp is None else sp
            wg, w, r = gw.owner(ntiles, t, grid)
            out.setdefault((wg, w), []).append((r, t, spm.mask(model, sp, t - first, pat)))
    return out


def test_the_dealing_covers_every_group_once():
    for ntiles in (1, 63, 64, 65, 255, 256, 257, 1630, 8192 * 256 + 1):
        for grid in (None, 1, 3):
            if ntiles > 10000 and grid:
                continue
            d = gw.deal(ntiles, grid)
            assert len(d) == gw.ngroups(ntiles) and len(set(d)) == len(d)
            G = gw.grid_of(ntiles, grid)
            assert all(wg < G and w < WAVES for wg, w, _ in d)
            # the static stride: group g of round r belongs to the wave that had group g - G * 4 in round r - 1
            assert all(d[g][:2] == d[g - G * WAVES][:2] and d[g][2] == d[g - G * WAVES][2] + 1 for g in range(G * WAVES, len(d)))


@pytest.mark.parametrize("chunked", (False, True))
@pytest.mark.parametrize("ntiles", gw.GROUP_EDGE_TILES)
def test_group_edges_hold_the_needle_in_first_and_last_tile(text, ntiles, chunked):
    blocks, pat, _ = gw.group_edges(text, ntiles, chunked)
    assert sum(gw.tiles_of(blocks)) == ntiles and (len(blocks) > 1) == chunked
    held = set(holding_tiles(blocks, pat))
    for g in range(gw.ngroups(ntiles)):
        assert g * GROUP in held and min(g * GROUP + GROUP - 1, ntiles - 1) in held
    assert ntiles - 1 in held and max(held) == ntiles - 1
    assert 4 * len(held) < ntiles  # the verdict's quarter
    if ntiles % GROUP:  # a partial last group: its lanes at and beyond ntiles have no tile
        assert gw.ngroups(ntiles) * GROUP > ntiles


@pytest.mark.parametrize("grid", (1, 3))
def test_many_groups_leave_waves_idle_in_the_last_round(model, text, grid):
    blocks, pat, _ = gw.many_groups(text)
    ntiles = sum(gw.tiles_of(blocks))
    assert ntiles == gw.MANY_GROUPS_TILES >= 577 and len(blocks) == 3
    d = gw.deal(ntiles, grid)
    waves = gw.grid_of(ntiles, grid) * WAVES
    assert waves == 4 * grid and len(d) % waves != 0
    per_wave = {}
    for wg, w, r in d:
        per_wave.setdefault((wg, w), []).append(r)
    assert len(per_wave) == waves and min(len(v) for v in per_wave.values()) >= 2  # every wave takes several groups
    last = max(r for _, _, r in d)
    busy_last = {k for k, v in per_wave.items() if last in v}
    assert busy_last and len(busy_last) < waves  # some waves have nothing to do in the last round while others scan
    by_wave = pairs_by_wave(model, blocks, pat, grid)
    assert any(r == last for k in busy_last for r, _, _ in by_wave.get(k, []))  # ... and scan: a needle in a last-round group
    assert set(by_wave) == set(per_wave)  # every wave has candidates with an occurrence


@pytest.mark.parametrize("name,busy", (("one_busy_wave", (2,)), ("three_busy_waves", (0, 1, 3))))
def test_all_the_work_in_some_waves(model, text, name, busy):
    blocks, pat, _ = gw.BINDINGS[name](text)
    ntiles = sum(gw.tiles_of(blocks))
    by_wave = pairs_by_wave(model, blocks, pat, 1)
    assert set(by_wave) == {(0, w) for w in busy}
    for w in busy:
        first = [(t, m) for r, t, m in by_wave[(0, w)] if r == 0]
        assert [t for t, _ in first] == list(range(w * GROUP, (w + 1) * GROUP)) and len(first) == len(by_wave[(0, w)])
        assert sum(bin(m).count("1") for _, m in first) == 4 * GROUP  # 256 (tile, span) pairs in one wave, one round
    assert 4 * GROUP * len(busy) < ntiles  # under the verdict's quarter


@pytest.mark.parametrize("plen", (28, 32, 40))
def test_long_needles_lie_in_groups_of_waves_1_2_3(text, plen):
    blocks, pat, flags = gw.long_staged(text, plen)
    assert len(pat) == plen and bool(flags) == (plen == 40)
    ntiles = sum(gw.tiles_of(blocks))
    held = holding_tiles(blocks, pat)
    owners = {gw.owner(ntiles, t, 1)[1:] for t in held}
    assert owners == {(w, r) for w in (1, 2, 3) for r in (0, 1)}  # never wave 0
    raw = blocks[0].tobytes()
    for koff in range(plen - 7):  # a decoy for every filter window: the window's bytes, the rest altered
        d = bytearray(b"~" * plen)
        d[koff:koff + 8] = pat[koff:koff + 8]
        assert raw.count(bytes(d)) == len(held) == 18
    assert raw.count(pat) == 18


@pytest.mark.parametrize("plen", (4, 8, 32))
def test_zone_pairs_end_64_tiles_apart_in_waves_1_2_3(text, plen):
    blocks, pat, _ = gw.zone_pairs(text, plen)
    ntiles, t0 = sum(gw.tiles_of(blocks)), gw.tile0_of(blocks)
    ends = [t - 1 for t in t0[1:-1]]  # the last tile of every chunk but the filler
    assert ends == [73, 137, 168, 232, 340, 404]
    owners = [gw.owner(ntiles, t, 1) for t in ends]
    assert owners == [(0, 1, 0), (0, 2, 0), (0, 2, 0), (0, 3, 0), (0, 1, 1), (0, 2, 1)]
    for a, b in zip(owners[::2], owners[1::2]):  # two waves of one workgroup in the same round
        assert a[0] == b[0] and a[1] != b[1] and a[2] == b[2]
    kinds = []
    for b in blocks[:-1]:
        L = int(b.size)
        Z = L - plen - 31
        occ = spm.occurrences(b, pat)
        kinds.append((any(o >= Z for o in occ), any(o < Z for o in occ)))
        assert all(o // TILE == (L - 1) // TILE for o in occ)  # all in the chunk's last tile: that tile looks at the zone
    assert kinds == [(True, False)] * 2 + [(False, True)] * 2 + [(True, True)] * 2  # zone only, ahead only, both


def test_span_patterns_give_one_wave_several_spans(model, text):
    blocks, pat, _ = gw.BINDINGS["span_patterns"](text)
    by_wave = pairs_by_wave(model, blocks, pat, None)
    assert set(by_wave) == {(0, 0)}  # every planted tile lies in group 0: one wave reads all their spans in turn
    masks = {t: m for _, t, m in by_wave[(0, 0)]}
    assert masks[20] == 15 and [masks[t] for t in (2, 5, 8, 11)] == [1, 2, 4, 8]
