#!/usr/bin/env python3
"""What xsg_count_literals costs (profiles/literal_counts_ab.jsonl, DESIGN.md sections 3.5e and 5).

2 GiB of resident corpus.py text in 128 chunks of 16 MiB (the shard of scripts/bench_literal_set.py), four lists: the 8
lexicon words and the 300 words of that script, 4096 seven-byte literals with 4096 distinct grams, and the dense list
`e`, `th`.  For each list, on one binding in one process, --runs interleaved runs of
  parent xsg_count        xsg_count(XSG_COUNT_MATCHES) of the PARENT build (--parent TREE: a checkout of the parent commit
                          with its library built)
  new xsg_count           the same call of this build
  parent count_literals   xsg_count_literals of the parent build, where it has one
  count_literals          xsg_count_literals of this build (keys in LDS, candidates compacted: the one form there is)
a run = --calls timed synchronous calls (host clock) behind --warm untimed ones.  `scan_ms` is xsg_time_scan_kernel of
the list: k_set_scan's count pass alone, the same loads and the same filter, the floor of any one-pass design.  One JSON
line per (list, call) with every run's median, the ratio to the parent's xsg_count and to the scan, that call's own
max / min spread, for this build's calls the parent's run medians of the same call, the ratio to it (`ratio_to_same`)
and the parent's spread of it (the runs alternate between the listed order and its reverse, so that neither build always
runs behind the other), and the share of positions that are candidates (from the filter image, on one 16 MiB template).  The two builds'
results are compared word for word before anything is timed.

--list-flags N (XSG_LIST_WHOLE_WORDS = 1; profiles/literal_words_ab.jsonl) adds a third side: this
build with the same list set through xsg_set_literals_opts(..., N), on a context and a binding of its own over the same
memory.  Its calls, `xsg_count opts` and `count_literals opts`, run interleaved with the others; their `same` is this
build's call WITHOUT the option, so `ratio_to_same` is the option's cost, and `occurrences_opts` / `list_matches_opts` say
how much it leaves standing.  The parent and this build without the option are compared as before."""
import argparse
import importlib.util
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ["XSG_TEST_HOOKS"] = "1"  # the A/B switches are re-read at every call
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "scripts")]


def load_xsg(tree: Path, name: str):
    """the binding of `tree` under its own module name, bound to that tree's library"""
    spec = importlib.util.spec_from_file_location(name, tree / "x-search_amd" / "xsg.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    old = os.environ.get("XSG_LIB")
    os.environ["XSG_LIB"] = str(tree / "x-search_amd" / "lib" / "libxsg.so")
    try:
        mod.load()
    finally:
        os.environ.pop("XSG_LIB", None)
        if old is not None:
            os.environ["XSG_LIB"] = old
    return mod


def lists():
    import bench_literal_set
    named = dict(bench_literal_set.lists())
    rng = np.random.Generator(np.random.PCG64(4096))
    grams = rng.permutation(26 ** 4)[:4096]  # 4096 distinct lower-case 4-grams
    distinct = []
    for v in grams:
        gram = bytes(97 + (int(v) // 26 ** k) % 26 for k in range(4))
        distinct.append(gram + bytes(rng.integers(97, 123, size=3).astype(np.uint8)))
    return [("8-words", named["8-words"]), ("300-words", named["300-words"]), ("4096-distinct-grams", distinct),
            ("dense e, th", [b"e", b"th"])]


def candidate_rate(xsg, block, lits):
    d, filt = xsg.literals_info(xsg.literal_list(lits), 0, with_filter=True)
    g = d["gram"]
    n = block.size - g + 1
    v = np.zeros(n, dtype=np.uint64)
    for k in range(g):
        v |= block[k:k + n].astype(np.uint64) << np.uint64(8 * k)
    h = v if g <= 2 else ((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    bits = (filt[(h >> np.uint64(5)).astype(np.int64)] >> (h & np.uint64(31)).astype(np.uint32)) & 1
    return float(bits.mean()), g


def timed(fn, warm, calls):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="", help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--list-flags", type=int, default=0, help="also time this build with these list_flags (1: whole words)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import corpus
    new = load_xsg(ROOT, "xsg_new")
    parent = load_xsg(Path(a.parent).resolve(), "xsg_parent") if a.parent else None
    dev = torch.device("cuda:0")
    blocks = [corpus.text_block(a.seed, i, (16 << 20) + 1 + corpus._mix(a.seed, 1000 + i) % 61) for i in range(a.templates)]
    nchunks = int(round(a.gib * 2**30 / (16 << 20)))
    plan = np.array([corpus._mix(a.seed ^ 0xC0FFEE, c) % a.templates for c in range(nchunks)])
    off, ln, cap = corpus.chunk_table(np.array([blocks[p].size for p in plan]))
    t = torch.empty(cap, dtype=torch.uint8, device=dev)
    dev_t = [torch.from_numpy(b).to(dev) for b in blocks]
    for c in range(nchunks):
        t[int(off[c]):int(off[c]) + int(ln[c])].copy_(dev_t[int(plan[c])])
    torch.cuda.synchronize()
    del dev_t
    total = int(ln.sum())
    sides = {}
    for label, mod in (("parent", parent), ("new", new), ("opts", new if a.list_flags else None)):
        if mod is None:
            continue
        ctx = mod.Context(0)
        ctx.set_pattern(b"x")
        sides[label] = (mod, ctx, mod.Shard(ctx, t.data_ptr(), cap, mod.make_chunks(off, ln)))
    sink = open(a.out, "a") if a.out else None

    for name, lits in lists():
        lst = new.literal_list(lits)
        for label, (_, ctx, _) in sides.items():
            if label == "opts":
                ctx.set_literals(lst, 0, a.list_flags)
            else:
                ctx.set_literals(lst, 0)
        ns = sides["new"][2]
        rate, g = candidate_rate(new, blocks[0], lits)
        calls = {}
        if parent:
            ps = sides["parent"][2]
            calls["parent xsg_count"] = lambda ps=ps: ps.count(parent.COUNT_MATCHES)
        calls["new xsg_count"] = lambda: ns.count(new.COUNT_MATCHES)
        if parent and hasattr(ps, "count_literals"):
            calls["parent count_literals"] = lambda ps=ps: ps.count_literals()
        calls["count_literals"] = lambda: ns.count_literals()
        if "opts" in sides:
            os_ = sides["opts"][2]
            calls["xsg_count opts"] = lambda os_=os_: os_.count(new.COUNT_MATCHES)
            calls["count_literals opts"] = lambda os_=os_: os_.count_literals()
        ref = calls["count_literals"]().tolist()
        # parity: the two builds agree word for word, call by call
        for k in [k for k in calls if k.startswith("parent ")]:
            if calls[k]().tolist() != calls[k.replace("parent ", "new " if k.endswith("xsg_count") else "")]().tolist():
                raise SystemExit(f"PARITY FAILURE ({name}): {k[7:]} of the two builds differs")
        matches = int(calls["new xsg_count"]()[new.CTR_MATCHES])
        med = {k: [] for k in calls}
        for r in range(a.runs):  # interleaved: one run of each, a.runs times over, every other time in reverse order
            for k, fn in (list(calls.items()) if r % 2 == 0 else list(calls.items())[::-1]):
                med[k].append(float(np.median(timed(fn, a.warm, a.calls))))
        scan_ms = ns.time_scan_kernel(new.COUNT_MATCHES, 10)
        base_key = "parent xsg_count" if parent else "new xsg_count"
        base = float(np.median(med[base_key]))
        for k, v in med.items():
            m = float(np.median(v))
            same = "parent " + k.replace("new ", "")  # the parent's same call, for this build's
            if k.endswith(" opts"):  # ... and this build's call without the option, for the option's
                same = "new xsg_count" if k.startswith("xsg_count") else "count_literals"
            row = {"what": "literal_counts", "list": name, "literals": len(lits), "gram": g, "candidate_rate": round(rate, 5),
                   "call": k, "bytes": total, "chunks": int(len(ln)), "list_matches": matches, "occurrences": int(sum(ref)),
                   "literals_that_occur": int(np.count_nonzero(ref)), "runs": a.runs, "calls_per_run": a.calls,
                   "run_median_ms": [round(x, 4) for x in v], "ms": round(m, 4), "ratio_to": base_key,
                   "ratio": round(m / base, 4), "max_over_min": round(max(v) / min(v), 4), "scan_ms": round(scan_ms, 4),
                   "ratio_to_scan": round(m / scan_ms, 3)}
            if k.endswith(" opts"):
                row.update({"list_flags": a.list_flags, "same": same, "list_matches_opts": int(calls["xsg_count opts"]()[new.CTR_MATCHES]),
                            "occurrences_opts": int(sum(calls["count_literals opts"]().tolist()))})
            if same in med and same != k:
                row.update({"same_run_median_ms": [round(x, 4) for x in med[same]], "same_ms": round(float(np.median(med[same])), 4), "ratio_to_same": round(m / float(np.median(med[same])), 4),
                            "same_max_over_min": round(max(med[same]) / min(med[same]), 4)})
            line = json.dumps(row)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()


if __name__ == "__main__":
    main()
