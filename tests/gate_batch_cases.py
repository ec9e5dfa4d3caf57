"""The batches of the wave form of the finishing gated count (x-search_amd/csrc/xsg_kernels.hip: gated_pass_waves), restated
in Python, and the bindings that tests/test_gpu_gate_batch.py runs on them.

The dealing is gate_wave_cases.deal: wave w of workgroup b owns the groups b * 4 + w + r * grid * 4 for rounds r = 0, 1, ...
A batch is the wave's next B rounds (B = kGateBatch of the build, named by the kernel: " in batches of B"): round r is place
r % B of batch r // B.  Per batch the wave selects all its groups at once, compacts the passing (round, lane) pairs in that
order into a row of 64 entries -- a batch with more takes its groups one at a time -- locates them in one round trip and
scans them.  tests/test_gate_batch_cases.py proves without a GPU that every binding below reaches the edge it is named after,
for B = 2, 4 and 8.

Every binding is a function of one text (gate_wave_cases.make_text) and B alone: -> (blocks, pattern, flags); all of them are
meant for XSG_GATE_GRID=1 (four waves) unless they say otherwise.
"""
import numpy as np

import gate_wave_cases as gw
from gate_wave_cases import GROUP, TEXT_TILES, TILE, UNIT, WAVES
from test_gpu_gate_spans import SPAN, needle
from test_gpu_sketch_select import plant

BATCHES = (2, 4, 8)
ROW = 64  # entries of a wave's candidate row


def batch_tag(B):
    return f" in batches of {B}" if B > 1 else ""


def place(ntiles, tile, B, grid=None):
    """-> (workgroup, wave, batch, place in the batch) of the wave and batch that test and scan `tile`"""
    wg, w, r = gw.owner(ntiles, tile, grid)
    return wg, w, r // B, r % B


def long_text(text, ntiles):
    """`ntiles` tiles of filler cut from the 700-tile text (five bytes short of the last tile's end)"""
    parts, have, i = [], 0, 0
    while have < ntiles:
        n = min(ntiles - have, TEXT_TILES - 80)
        parts.append(text[(37 * i % 70) * TILE:][:n * TILE])
        have, i = have + n, i + 1
    return np.concatenate(parts)[:ntiles * TILE - 5].copy()


def cut(whole, ntiles, sizes):
    """chunks of sizes[0], sizes[1], ... tiles (cyclic), every chunk but the last three bytes short of its last tile's end"""
    blocks, t, k = [], 0, 0
    while t < ntiles:
        n = min(sizes[k % len(sizes)], ntiles - t)
        blocks.append(whole[t * TILE:(t + n) * TILE - (3 if t + n < ntiles else 0)].copy())
        t, k = t + n, k + 1
    return blocks


# ---- round counts ----------------------------------------------------------------------------------------------------------
def rounds_ntiles(B, rounds):
    """under grid 1: waves 0 and 1 take `rounds` rounds, waves 2 and 3 one fewer; the last group holds 41 tiles"""
    return ((rounds - 1) * WAVES + 2) * GROUP - 23


def rounds_spots(ntiles):
    """two tiles of every group, the first tile of every fourth, and the binding's last tile"""
    t = set()
    for g in range(gw.ngroups(ntiles)):
        t |= {g * GROUP + l for l in (5 + g % 20, 30 + g % 4) if g * GROUP + l < ntiles}
        if g % 4 == 1:
            t.add(g * GROUP)
    return sorted(t | {ntiles - 1})


def rounds(text, B, nrounds):
    """chunks of 1, 2, 3, ... 7 tiles, so that the groups of one batch lie in different chunks and tile_chunk decides every
    candidate's geometry; the needle in the tiles of rounds_spots, the last of them the binding's last tile"""
    ntiles = rounds_ntiles(B, nrounds)
    pat = needle(8)
    whole = long_text(text, ntiles)
    plant(whole, pat, [t * TILE + (t % 4) * SPAN + 100 + t % 900 for t in rounds_spots(ntiles)])
    return cut(whole, ntiles, (1, 2, 3, 4, 5, 6, 7)), pat, 0


def round_cases(B):
    """rounds of waves 0 and 1 (waves 2 and 3: one fewer): exactly B (the others a partial only batch), B + 1 (a second batch
    of one group while waves 2 and 3 have none), and a partial last batch behind a full one"""
    return sorted({B, B + 1, B + max(B // 2, 1) + 1})


# ---- candidate counts of a batch -------------------------------------------------------------------------------------------
def count_plan(B):
    """(wave, batch) -> the number of tiles that hold the needle in each of the batch's B groups"""
    z = [0] * B
    return {
        (0, 0): [64] + z[1:],                    # 64: the row exactly full, all from one group, none in the next
        (1, 0): [64] + z[1:-1] + [1],            # 65: one group at a time
        (2, 0): [31] + z[1:-1] + [32],           # 63
        (3, 0): z[:-1] + [1],                    # 1, in the batch's last group
        (0, 1): [1] + z[1:],                     # 1, in the batch's first group
        (1, 1): z,                               # 0
        (2, 1): [1] + z[1:-1] + [63],            # 64 from two groups
        (3, 1): [33] + z[1:-1] + [32],           # 65 from two groups
    }


def lanes_of(n):
    """which n lanes of a group hold the needle"""
    if n == 64:
        return list(range(64))
    if n == 1:
        return [63]
    return list(range(1, 2 * n, 2)) if 2 * n <= 64 else list(range(n))


def full_plan(B):
    """wave 0's first batch holds the needle in all four spans of all 64 tiles of all B groups: 64 * B candidates, 256 * B
    (tile, span) pairs (the busy_waves recipe); nothing anywhere else"""
    return {(0, 0): [64] * B}


def counts(text, B, plan_of=count_plan):
    """two batches a wave with the candidate counts of count_plan (or full_plan's one), then quiet groups (batches without
    a candidate) that keep the share of passing tiles under the verdict's quarter"""
    pat = needle(8)
    plan = plan_of(B)
    held = sum(sum(v) for v in plan.values())
    nbatches = 1 + max(b for _, b in plan)
    ntiles = max(nbatches * B * UNIT, 4 * held + GROUP) + UNIT
    ntiles += (-ntiles) % UNIT
    whole = long_text(text, ntiles)
    spots = []
    for (w, b), per_group in plan.items():
        for j, n in enumerate(per_group):
            g = (b * B + j) * WAVES + w
            for l in lanes_of(n):
                t = g * GROUP + l
                for s in (range(4) if plan_of is full_plan else (t % 4,)):
                    spots.append(t * TILE + s * SPAN + 200 + 3 * l + s)
    plant(whole, pat, spots)
    return cut(whole, ntiles, (ntiles,)), pat, 0


BINDINGS = {"counts": counts, "full": lambda t, B: counts(t, B, full_plan)}
for _k in (0, 1, 2):
    BINDINGS[f"rounds{_k}"] = lambda t, B, k=_k: rounds(t, B, round_cases(B)[min(k, len(round_cases(B)) - 1)])
BINDINGS.update({
    "zones4": lambda t, B: gw.zone_pairs(t, 4), "zones8": lambda t, B: gw.zone_pairs(t, 8), "zones32": lambda t, B: gw.zone_pairs(t, 32),
    "long32": lambda t, B: gw.long_staged(t, 32),
})
