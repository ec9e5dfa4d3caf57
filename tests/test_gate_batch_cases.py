"""Without a GPU: every binding of tests/gate_batch_cases.py reaches the edge of the wave form's batches it is named after,
for B = 2, 4 and 8 -- which (workgroup, wave, batch, place) every planted tile lands in, how many tiles of a batch hold the
needle (the batch's candidates are a superset: the gate may let a tile through that holds none), and that fewer than a
quarter of the tiles hold the needle, the verdict's condition."""
import pytest

import gate_batch_cases as gb
import gate_wave_cases as gw
import span_sketch_model as spm
from gate_batch_cases import BATCHES
from gate_wave_cases import GROUP, TILE, WAVES
from test_gate_wave_cases import holding_tiles


@pytest.fixture(scope="module")
def text():
    return gw.make_text()


def by_batch(blocks, pat, B, grid=1):
    """(workgroup, wave, batch) -> [(place, tile)] of the tiles that hold the needle, in (round, lane) order"""
    ntiles, out = sum(gw.tiles_of(blocks)), {}
    for t in sorted(holding_tiles(blocks, pat)):
        wg, w, b, j = gb.place(ntiles, t, B, grid)
        out.setdefault((wg, w, b), []).append((j, t))
    return {k: sorted(v) for k, v in out.items()}


@pytest.mark.parametrize("B", BATCHES)
def test_a_batch_is_the_next_rounds_of_one_wave(B):
    for ntiles, grid in ((1, 1), (64 * 4 * B + 1, 1), (1630, 3), (2000, 1)):
        G = gw.grid_of(ntiles, grid)
        seen = {}
        for g in range(gw.ngroups(ntiles)):
            wg, w, b, j = gb.place(ntiles, g * GROUP, B, grid)
            assert g == wg * WAVES + w + (b * B + j) * G * WAVES and j < B
            seen.setdefault((wg, w, b), []).append(j)
        assert all(v == list(range(len(v))) for v in seen.values())  # a batch's places are its rounds in order, no gap


@pytest.mark.parametrize("B", BATCHES)
def test_round_counts_full_partial_and_one_more(text, B):
    cases = gb.round_cases(B)
    assert B in cases and B + 1 in cases and any(r % B for r in cases)
    for k, nrounds in enumerate(cases):
        blocks, pat, _ = gb.BINDINGS[f"rounds{k}"](text, B)
        ntiles = sum(gw.tiles_of(blocks))
        assert ntiles == gb.rounds_ntiles(B, nrounds) and ntiles % GROUP  # the last real group is partial
        per_wave = {}
        for wg, w, r in gw.deal(ntiles, 1):
            per_wave.setdefault(w, []).append(r)
        assert [len(per_wave[w]) for w in range(WAVES)] == [nrounds, nrounds, nrounds - 1, nrounds - 1]
        held = holding_tiles(blocks, pat)
        assert max(held) == ntiles - 1 and 4 * len(held) < ntiles
        got = by_batch(blocks, pat, B)
        last = (nrounds - 1) // B
        # waves 0 and 1 scan in their last batch ...
        assert all((0, w, last) in got for w in (0, 1))
        n_last = (nrounds - 1) % B + 1  # groups of that batch: it reaches past ngroups unless it is full
        assert max(j for j, _ in got[(0, 1, last)]) == n_last - 1 and gb.place(ntiles, ntiles - 1, B, 1) == (0, 1, last, n_last - 1)
        if nrounds % B == 1:  # ... while waves 2 and 3 have none
            assert (0, 2, last) not in got and (0, 3, last) not in got and (0, 2, last - 1) in got
        # every batch with groups holds the needle, in every one of its groups
        for (wg, w, b), v in got.items():
            assert {j for j, _ in v} == set(range(min(B, len(per_wave[w]) - b * B)))
        # the groups of one batch lie in different chunks: a candidate needs its own group's tile_chunk
        t0 = gw.tile0_of(blocks)
        chunk_of = lambda t: max(c for c in range(len(blocks)) if t0[c] <= t)
        for v in got.values():
            chunks = [{chunk_of(t) for j, t in v if j == p} for p in sorted({j for j, _ in v})]
            assert all(not (a & b) for i, a in enumerate(chunks) for b in chunks[i + 1:])
        assert len(blocks) > 2 * gw.ngroups(ntiles)


@pytest.mark.parametrize("B", BATCHES)
def test_candidate_counts_of_a_batch(text, B):
    blocks, pat, _ = gb.BINDINGS["counts"](text, B)
    ntiles = sum(gw.tiles_of(blocks))
    got = by_batch(blocks, pat, B)
    plan = gb.count_plan(B)
    totals = sorted(sum(v) for v in plan.values())
    assert totals == [0, 1, 1, 63, 64, 64, 65, 65]
    for (w, b), per_group in plan.items():
        have = [sum(1 for j, _ in got.get((0, w, b), []) if j == p) for p in range(B)]
        assert have == per_group, (w, b)
    assert set(got) == {(0, w, b) for (w, b), v in plan.items() if sum(v)}  # every other batch holds nothing
    assert ntiles // (GROUP * WAVES) > 2 * B  # ... and there are such batches behind the planned ones
    assert 4 * len(holding_tiles(blocks, pat)) < ntiles
    # 64 in one group and none in the next, then one: 65 takes its groups one at a time, 64 fills the row
    assert plan[(1, 0)][0] == 64 and plan[(1, 0)][-1] == 1 and sum(plan[(0, 0)]) == gb.ROW


@pytest.mark.parametrize("B", BATCHES)
def test_a_batch_of_64_B_candidates_with_all_four_spans(tmp_path_factory, text, B):
    blocks, pat, _ = gb.BINDINGS["full"](text, B)
    ntiles = sum(gw.tiles_of(blocks))
    got = by_batch(blocks, pat, B)
    assert set(got) == {(0, 0, 0)} and len(got[(0, 0, 0)]) == 64 * B
    assert [sum(1 for j, _ in got[(0, 0, 0)] if j == p) for p in range(B)] == [64] * B
    assert 4 * 64 * B < ntiles
    if B == 2:  # (the locator's model is slow: one B) every span of every tile passes
        model = spm.load(tmp_path_factory.mktemp("gate_batch_cases_model"))
        sp = spm.build(model, blocks[0])
        assert all(spm.mask(model, sp, t, pat) == 15 for _, t in got[(0, 0, 0)][::16])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("plen", (4, 8, 32))
def test_two_zone_looks_by_one_wave_inside_one_batch(text, B, plen):
    blocks, pat, _ = gb.BINDINGS[f"zones{plen}"](text, B)
    ntiles, t0 = sum(gw.tiles_of(blocks)), gw.tile0_of(blocks)
    ends = [t - 1 for t in t0[1:-1]]
    where = [gb.place(ntiles, t, B, 1) for t in ends]
    per_batch = {}
    for wg, w, b, j in where:
        per_batch.setdefault((wg, w, b), []).append(j)
    assert per_batch[(0, 1, 0)] == [0, 1] and sorted(per_batch[(0, 2, 0)]) == [0, 0, 1]  # rounds 0 and 1 of one batch
    assert 4 * len(holding_tiles(blocks, pat)) < ntiles


@pytest.mark.parametrize("B", BATCHES)
def test_the_long_needle_lies_in_rounds_0_and_1_of_waves_1_2_3(text, B):
    blocks, pat, _ = gb.BINDINGS["long32"](text, B)
    ntiles = sum(gw.tiles_of(blocks))
    where = {gb.place(ntiles, t, B, 1)[1:] for t in holding_tiles(blocks, pat)}
    assert where == {(w, 0, j) for w in (1, 2, 3) for j in (0, 1)}  # one batch a wave, rounds 0 and 1, never wave 0
    assert 4 * len(holding_tiles(blocks, pat)) < ntiles
