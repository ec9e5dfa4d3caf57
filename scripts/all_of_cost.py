#!/usr/bin/env python3
"""What XSG_LIST_ALL_OF costs against what it replaces (profiles/all_of_ab.jsonl).

2 GiB of resident corpus.py text in one chunk table of 128 chunks of 16 MiB (the shard of scripts/literal_counts_cost.py),
lists of 2, 3 and 8 literals, once of RARE words (the planted needle and words the text does not hold: next to no
candidate survives the verify step) and once of FREQUENT ones (lexicon words of five bytes and more: each stands in about
one line in eleven).  For each list, on one binding in one process, --runs interleaved runs of
  all-of count      xsg_count(XSG_COUNT_LINES) of the list set with XSG_LIST_ALL_OF
  all-of search     xsg_search(XSG_LINE_BYTE_OFFSETS) of it, the result fetched
  k counts          what a user of the parent commit runs for the count: k searches of lists of one and the intersection
  k searches        ... and for the list: k x xsg_search(XSG_LINE_BYTE_OFFSETS) of a list of one, each result fetched, and
                    numpy.intersect1d over the k arrays on the host
The k searches run on the PARENT build where --parent TREE names a checkout of the parent commit with its library built
(a context and a binding of its own over the same memory), on this build otherwise; their code is the same either way.
a run = --calls timed synchronous calls (host clock) behind --warm untimed ones; the runs alternate between the listed
order and its reverse.  One JSON line per (list, call): every run's median, their median, max / min over the runs, and for
the all-of calls the ratio to the k-fold call they replace.  The results are compared element for element before anything
is timed.  With --list-flags-parity the script also times xsg_count(XSG_COUNT_LINES) and xsg_search(XSG_LINE_BYTE_OFFSETS)
of each list with list_flags 0 and 1 on both builds: the calls this change must leave alone."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "x-search_amd"), str(ROOT / "scripts")]

from literal_counts_cost import load_xsg, timed  # noqa: E402

RARE = [b"Sherlock", b"zeppelin", b"quagmire", b"Moriarty", b"xylophone", b"Baskerville", b"juxtapose", b"kumquat"]
FREQUENT = [b"Holmes", b"Watson", b"detective", b"street", b"which", b"their", b"would", b"there"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="", help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--list-flags-parity", action="store_true")
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

    def side(mod):
        ctx = mod.Context(0)
        ctx.set_pattern(b"x")
        return mod, ctx, mod.Shard(ctx, t.data_ptr(), cap, mod.make_chunks(off, ln))

    nmod, nctx, ns = side(new)
    bmod, bctx, bs = side(parent) if parent else (nmod, nctx, ns)  # the side of the k searches
    sink = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def measure(calls):
        med = {k: [] for k in calls}
        for r in range(a.runs):
            for k, fn in (list(calls.items()) if r % 2 == 0 else list(calls.items())[::-1]):
                med[k].append(float(np.median(timed(fn, a.warm, a.calls))))
        return med

    for kind, words in (("rare", RARE), ("frequent", FREQUENT)):
        for k in (2, 3, 8):
            lits = words[:k]
            ones = [new.literal_list((l,)) for l in lits]

            def all_of_count():
                nctx.set_literals(new.literal_list(lits), 0, new.LIST_ALL_OF)
                return int(ns.count(new.COUNT_LINES)[new.CTR_LINES])

            def all_of_search():
                nctx.set_literals(new.literal_list(lits), 0, new.LIST_ALL_OF)
                return ns.search_u64(new.LINE_BYTE_OFFSETS)

            def k_searches():
                arrs = []
                for one in ones:
                    bctx.set_literals(one, 0)
                    arrs.append(bs.search_u64(bmod.LINE_BYTE_OFFSETS))
                out = arrs[0]
                for x in arrs[1:]:
                    out = np.intersect1d(out, x, assume_unique=True)
                return out

            def k_counts():
                return int(k_searches().size)  # (no count of the parent gives the conjunction: the lists are needed)

            want = k_searches()
            got = all_of_search()
            if got.tolist() != want.tolist() or all_of_count() != int(want.size):
                raise SystemExit(f"PARITY FAILURE ({kind}, k={k}): the all-of result differs from the intersection of the k searches")
            per_literal = []
            for one in ones:
                bctx.set_literals(one, 0)
                per_literal.append(int(bs.count(bmod.COUNT_LINES)[bmod.CTR_LINES]))
            calls = {"all-of count": all_of_count, "all-of search": all_of_search, "k counts": k_counts, "k searches": k_searches}
            med = measure(calls)
            for name, v in med.items():
                m = float(np.median(v))
                row = {"what": "all_of", "list": f"{kind}-{k}", "literals": k, "call": name, "bytes": total, "chunks": int(len(ln)),
                       "baseline_build": "parent" if parent else "this", "selected_lines": int(want.size), "lines_per_literal": per_literal,
                       "runs": a.runs, "calls_per_run": a.calls, "run_median_ms": [round(x, 4) for x in v], "ms": round(m, 4),
                       "max_over_min": round(max(v) / min(v), 4)}
                if name.startswith("all-of"):
                    base = "k counts" if name.endswith("count") else "k searches"
                    b = float(np.median(med[base]))
                    row.update({"ratio_to": base, "ratio": round(m / b, 4), "baseline_ms": round(b, 4),
                                "baseline_max_over_min": round(max(med[base]) / min(med[base]), 4)})
                emit(row)
            if a.list_flags_parity and parent:
                for lf in (0, 1):
                    lst = new.literal_list(lits)
                    nctx.set_literals(lst, 0, lf)
                    bctx.set_literals(lst, 0, lf)
                    if ns.search_u64(new.LINE_BYTE_OFFSETS).tolist() != bs.search_u64(bmod.LINE_BYTE_OFFSETS).tolist():
                        raise SystemExit(f"PARITY FAILURE ({kind}, k={k}, list_flags={lf}): the two builds differ")
                    calls = {"parent count": lambda: bs.count(bmod.COUNT_LINES), "new count": lambda: ns.count(new.COUNT_LINES),
                             "parent search": lambda: bs.search_u64(bmod.LINE_BYTE_OFFSETS), "new search": lambda: ns.search_u64(new.LINE_BYTE_OFFSETS)}
                    med = measure(calls)
                    for name, v in med.items():
                        m = float(np.median(v))
                        row = {"what": "list_flags_parity", "list": f"{kind}-{k}", "literals": k, "list_flags": lf, "call": name, "bytes": total,
                               "runs": a.runs, "calls_per_run": a.calls, "run_median_ms": [round(x, 4) for x in v], "ms": round(m, 4),
                               "max_over_min": round(max(v) / min(v), 4)}
                        if name.startswith("new "):
                            p = med["parent " + name[4:]]
                            row.update({"parent_ms": round(float(np.median(p)), 4), "ratio_to_parent": round(m / float(np.median(p)), 4),
                                        "parent_max_over_min": round(max(p) / min(p), 4)})
                        emit(row)


if __name__ == "__main__":
    main()
