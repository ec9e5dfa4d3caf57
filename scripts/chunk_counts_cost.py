#!/usr/bin/env python3
"""What xsg_count_chunks costs (profiles/chunk_counts_ab.jsonl).  XSG_SKETCH=0 throughout: scan +
finish on both sides.

  ab      the bench-shaped shard (bench.py's templates and chunk plan, 16 MiB chunks, 10 GiB by default), `Sherlock`,
          XSG_COUNT_MATCHES and XSG_COUNT_LINES: xsg_count of the PARENT build (--parent TREE: a checkout of the parent
          commit with its library built) against xsg_count_chunks and xsg_count of this build, on the same device buffer
          in the same process, interleaved: --runs runs of each, a run = --calls timed calls (host clock around the
          synchronous call, which ends in a stream sync) behind --warm untimed ones.  One JSON line per (mode, build, call)
          with every run's median, and the ratio of the medians' medians against the parent with the parent's own
          max / min spread beside it.
  cuts    the same 2 GiB of text bound as 1 chunk, as 128 x 16 MiB and as 131072 x 16 KiB, `Sherlock`, then the dense
          needle `e` on the 131072-chunk binding: --calls calls of xsg_count_chunks(XSG_COUNT_MATCHES) each, then as many
          of xsg_count (k_count_finish on the same binding: what the chunk part costs without the boundaries).  Run it under
          `rocprofv3 --kernel-trace --output-format csv` in a run of its own; it writes the order of its cases to --cases.
  kernel  reads that trace (--trace CSV) and the cases file and prints one JSON line per case: the time of k_count_chunks,
          of k_count_finish and of the scan in front, per call.
"""
import argparse
import csv
import importlib.util
import json
import os
import sys
import time
import types
from pathlib import Path

import numpy as np

os.environ["XSG_SKETCH"] = "0"
ROOT = Path(__file__).resolve().parents[1]


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


def timed(fn, warm, calls):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def bench_shard(torch, gib, templates):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "x-search_amd"))
    import bench
    import corpus
    args = types.SimpleNamespace(chunk_mib=16, templates=templates, seed=0x5EED)
    blocks = bench.template_blocks(args, b"Sherlock")
    tbytes = np.array([b.size for b in blocks], dtype=np.int64)
    nchunks = max(1, int(round(gib * 2**30 / (16 << 20))))
    plan = bench.chunk_plan(args, 0, nchunks)
    off, ln, cap = corpus.chunk_table(tbytes[plan])
    dev = torch.device("cuda", 0)
    t = torch.empty(cap, dtype=torch.uint8, device=dev)
    dev_templates = [torch.from_numpy(b).to(dev) for b in blocks]
    for c in range(nchunks):
        src = dev_templates[int(plan[c])]
        t[int(off[c]):int(off[c]) + src.numel()].copy_(src)
    torch.cuda.synchronize()
    return t, off, ln, cap


def cmd_ab(a):
    import torch
    new = load_xsg(ROOT, "xsg_new")
    parent = load_xsg(Path(a.parent).resolve(), "xsg_parent")
    t, off, ln, cap = bench_shard(torch, a.gib, a.templates)
    sides = {}
    for label, mod in (("parent", parent), ("new", new)):
        ctx = mod.Context(0)
        ctx.set_pattern(b"Sherlock")
        sides[label] = (mod, ctx, mod.Shard(ctx, t.data_ptr(), cap, mod.make_chunks(off, ln)))
    out = []
    for mode_name in ("count_matches", "count_lines"):
        mode = new.COUNT_MATCHES if mode_name == "count_matches" else new.COUNT_LINES
        key = new.CTR_MATCHES if mode_name == "count_matches" else new.CTR_LINES
        ps, ns = sides["parent"][2], sides["new"][2]
        want = ps.count(mode).tolist()
        counts, _, totals = ns.count_chunks(mode)
        if totals.tolist() != want or int(counts.sum()) != want[key] or ns.count(mode).tolist() != want:
            raise SystemExit(f"PARITY FAILURE ({mode_name}): parent {want}, totals {totals.tolist()}, sum {int(counts.sum())}")
        calls = {"parent xsg_count": lambda: ps.count(mode), "new xsg_count_chunks": lambda: ns.count_chunks(mode),
                 "new xsg_count": lambda: ns.count(mode)}
        med = {k: [] for k in calls}
        for _ in range(a.runs):  # interleaved: one run of each, a.runs times over
            for k, fn in calls.items():
                med[k].append(float(np.median(timed(fn, a.warm, a.calls))))
        base = float(np.median(med["parent xsg_count"]))
        spread = max(med["parent xsg_count"]) / min(med["parent xsg_count"])
        for k, v in med.items():
            out.append({"what": "ab", "mode": mode_name, "call": k, "needle": "Sherlock", "sketch": 0, "gib": a.gib, "templates": a.templates, "bytes": int(ln.sum()),
                        "chunks": int(len(ln)), "result": want[key], "runs": a.runs, "calls_per_run": a.calls,
                        "run_median_ms": [round(x, 4) for x in v], "ms": round(float(np.median(v)), 4),
                        "ratio_to_parent": round(float(np.median(v)) / base, 4), "parent_max_over_min": round(spread, 4)})
    for line in out:
        print(json.dumps(line), flush=True)


CUTS = (("1 chunk", 1), ("128 x 16 MiB", 128), ("131072 x 16 KiB", 131072))


def cmd_cuts(a):
    import torch
    sys.path.insert(0, str(ROOT / "x-search_amd"))
    import corpus
    xsg = load_xsg(ROOT, "xsg_new")
    total = 2 << 30
    tpl = [torch.from_numpy(corpus.text_block(0x5EED, i, 16 << 20)).to("cuda:0") for i in range(4)]
    t = torch.empty(total + 256, dtype=torch.uint8, device="cuda:0")
    for c in range(128):
        t[c << 24:(c + 1) << 24].copy_(tpl[c % 4])
    torch.cuda.synchronize()
    ctx = xsg.Context(0)
    shard, cases = None, []
    for needle in (b"Sherlock", b"e"):
        ctx.set_pattern(needle)
        for name, n in CUTS if needle == b"Sherlock" else CUTS[2:]:
            ln = np.full(n, total // n, dtype=np.uint64)
            off = np.arange(n, dtype=np.uint64) * np.uint64(total // n)
            chunks = xsg.make_chunks(off, ln)
            if shard is None:
                shard = xsg.Shard(ctx, t.data_ptr(), total, chunks)
            else:
                shard.rebind(t.data_ptr(), total, chunks)
            ms = timed(lambda: shard.count_chunks(xsg.COUNT_MATCHES), a.warm, a.calls)
            counts, _, totals = shard.count_chunks(xsg.COUNT_MATCHES)
            assert int(counts.sum()) == int(totals[xsg.CTR_MATCHES])
            plain = timed(lambda: shard.count(xsg.COUNT_MATCHES), a.warm, a.calls)  # the yardstick: k_count_finish on the same binding
            cases.append({"needle": needle.decode(), "cut": name, "chunks": n, "launches": a.warm + a.calls + 1,
                          "finish_launches": a.warm + a.calls, "count_call_ms_median": round(float(np.median(plain)), 4),
                          "matches": int(totals[xsg.CTR_MATCHES]), "chunks_with_a_match": int(np.count_nonzero(counts)),
                          "call_ms_median": round(float(np.median(ms)), 4)})
            print(json.dumps(cases[-1]), flush=True)
    Path(a.cases).parent.mkdir(parents=True, exist_ok=True)
    Path(a.cases).write_text(json.dumps(cases))


def cmd_kernel(a):
    cases = json.loads(Path(a.cases).read_text())
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    fin = [i for i, r in enumerate(rows) if "k_count_chunks" in r[2]]
    if len(fin) != sum(c["launches"] for c in cases):
        raise SystemExit(f"{len(fin)} launches of k_count_chunks in the trace, the cases file has {sum(c['launches'] for c in cases)}")
    plain = [i for i, r in enumerate(rows) if "k_count_finish" in r[2]]
    if len(plain) != sum(c["finish_launches"] for c in cases):
        raise SystemExit(f"{len(plain)} launches of k_count_finish in the trace, the cases file has {sum(c['finish_launches'] for c in cases)}")
    at = pat = 0
    for c in cases:
        mine = fin[at + 1:at + c["launches"]]  # (without the case's first launch: the first pass over a new binding)
        at += c["launches"]
        fus = [(rows[i][1] - rows[i][0]) / 1e3 for i in plain[pat + 1:pat + c["finish_launches"]]]
        pat += c["finish_launches"]
        c = {**c, "k_count_finish_us": {"min": round(min(fus), 2), "median": round(float(np.median(fus)), 2), "max": round(max(fus), 2)}}
        us = [(rows[i][1] - rows[i][0]) / 1e3 for i in mine]
        scan = [(rows[i - 1][1] - rows[i - 1][0]) / 1e3 for i in mine]  # the launch in front of it: the scan
        print(json.dumps({"what": "kernel", **c, "k_count_chunks_us": {"min": round(min(us), 2), "median": round(float(np.median(us)), 2),
                                                                      "max": round(max(us), 2)},
                          "scan_in_front": rows[mine[0] - 1][2][:60], "scan_us_median": round(float(np.median(scan)), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="what", required=True)
    p = sub.add_parser("ab")
    p.add_argument("--parent", required=True, help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
    p.add_argument("--gib", type=float, default=10.0)
    p.add_argument("--templates", type=int, default=32)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warm", type=int, default=3)
    p = sub.add_parser("cuts")
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--cases", default="chunk_counts_cases.json")
    p = sub.add_parser("kernel")
    p.add_argument("--trace", required=True)
    p.add_argument("--cases", default="chunk_counts_cases.json")
    a = ap.parse_args()
    {"ab": cmd_ab, "cuts": cmd_cuts, "kernel": cmd_kernel}[a.what](a)


if __name__ == "__main__":
    main()
