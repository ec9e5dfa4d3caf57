#!/usr/bin/env python3
"""What a row limit buys and what it costs the searches without one: this build against the PARENT commit's, interleaved
in one session ("Row limit"; results in profiles/max_count_ab.jsonl, one JSON line per figure).

  resident  2 GiB in 128 chunks on the device (one 16 MiB block of corpus text, repeated), XSG_LINE_BYTE_OFFSETS of a sparse
            needle (`Sherlock`) and of `e`, N = 1: xsg_set_max_count(1) + xsg_search on this build against what a caller does
            on the parent build -- the full search, xsg_result_chunk_ptr and a cut on the host; xsg_count with and without
            the limit; and one exact-route list search without a limit (`that`, XSG_LINE_INDICES) on both builds.
  file      `xsgrep --max-count=1 Sherlock` and `xsgrep -l Sherlock` on a file in the page cache (--file-gib, 10) whose only
            hit lies early, in the last chunk, or nowhere, against the parent's `xsgrep -c`, `xsgrep -l` and plain `xsgrep`;
            every run a fresh process.
  bench     the plain `python bench.py --gpus 1` line of both trees.

Every figure is a median of --runs (>= 5) with the spread max / min beside it; the two builds alternate run by run.
--parent TREE: a checkout of the parent commit with its library and tools built (required: the baseline is the parent)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CHUNK = 16 << 20


def child_resident(a):
    tree = Path(a.tree)
    sys.path[:0] = [str(tree / "x-search_amd")]
    import numpy as np
    import torch

    import corpus
    import xsg
    nchunks = a.gib * 1024 // 16
    block = torch.from_numpy(corpus.text_block(7, 0, CHUNK, needle_rate=2e-6)).to("cuda:0")
    text = block.repeat(nchunks)
    off = np.arange(nchunks, dtype=np.uint64) * np.uint64(CHUNK)
    chunks = xsg.make_chunks(off, np.full(nchunks, CHUNK, dtype=np.uint64), off, None)
    ctx = xsg.Context(0)
    shard = xsg.Shard(ctx, text.data_ptr(), text.numel(), chunks)
    limited = hasattr(ctx, "set_max_count")

    def timed(fn):
        fn()
        t = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return t

    def host_cut():
        v = shard.search_u64(xsg.LINE_BYTE_OFFSETS)
        rows = shard.result_chunk_ptr()
        first = rows[:-1][np.diff(rows.astype(np.int64)) > 0]
        return v[first.astype(np.int64)]

    out = []
    for needle in (b"Sherlock", b"e"):
        ctx.set_pattern(needle, 0)
        want = host_cut()
        out.append({"what": "full search + chunk_ptr + host cut", "needle": needle.decode(), "ms": timed(host_cut), "entries": int(want.size)})
        out.append({"what": "xsg_count, no limit", "needle": needle.decode(), "ms": timed(lambda: shard.count(xsg.COUNT_LINES))})
        if limited:
            ctx.set_max_count(1)
            got = shard.search_u64(xsg.LINE_BYTE_OFFSETS)
            assert np.array_equal(got, want), "the limited search and the host cut differ"
            out.append({"what": "xsg_set_max_count(1) + search", "needle": needle.decode(), "ms": timed(lambda: shard.search_u64(xsg.LINE_BYTE_OFFSETS)),
                        "entries": int(got.size)})
            out.append({"what": "xsg_count, limit 1", "needle": needle.decode(), "ms": timed(lambda: shard.count(xsg.COUNT_LINES))})
    ctx.set_pattern(b"that", 0)  # (a lexicon word: millions of lines, far beyond the one-sync route's capacity -- the exact route)
    out.append({"what": "exact-route list search, no limit", "needle": "that", "mode": "line_indices",
                "ms": timed(lambda: shard.search_u64(xsg.LINE_INDICES))})
    print(json.dumps(out))


def summarise(ms):
    return {"median_ms": round(statistics.median(ms), 3), "spread": round(max(ms) / max(min(ms), 1e-9), 2), "runs": len(ms)}


def run_cli(tree, args, env):
    t0 = time.perf_counter()
    r = subprocess.run([str(Path(tree) / "tools" / "build" / "xsgrep"), *args], capture_output=True, env=env)
    return (time.perf_counter() - t0) * 1e3, r.returncode, len(r.stdout)


def poke(path, offset, data):
    """writes `data` at `offset`, -> the bytes that stood there"""
    with open(path, "r+b") as f:
        f.seek(offset)
        old = f.read(len(data))
        f.seek(offset)
        f.write(data)
    return old


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="", help="a tree of the parent commit with its library and tools built")
    ap.add_argument("--parts", default="resident,file,bench")
    ap.add_argument("--gib", type=int, default=2)
    ap.add_argument("--file-gib", type=int, default=10)
    ap.add_argument("--dir", default="/tmp/xsg_max_count_ab")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--deadline-s", type=float, default=0, help="start no further bench run after this many seconds (0: no deadline)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "max_count_ab.jsonl"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "resident":
        return child_resident(a)
    if not a.parent:
        sys.exit("--parent TREE is required: the baseline is the parent commit's build")
    trees = {"this": str(ROOT), "parent": str(Path(a.parent).resolve())}
    t_start = time.monotonic()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    open(a.out, "w").close()

    def record(**kw):  # (a line is on file as soon as it exists: a run that is cut short keeps what it had)
        print(json.dumps(kw), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(kw) + "\n")

    def check(rc, what):  # a process that died (a signal, an abort) ends the session: nothing more is started on the device
        if rc < 0 or rc >= 124:
            record(part="aborted", what=what, returncode=rc)
            sys.exit(f"{what}: exit status {rc}; stopping")

    parts = a.parts.split(",")
    if "resident" in parts:
        # two processes per build, alternating: a figure's runs come from both
        got = {}
        for rep in range(2):
            for side, tree in trees.items():
                env = dict(os.environ, XSG_LIB=str(Path(tree) / "x-search_amd" / "lib" / "libxsg.so"))
                r = subprocess.run([sys.executable, __file__, "--child", "resident", "--tree", tree, "--gib", str(a.gib), "--runs", str(a.runs)],
                                   check=True, capture_output=True, text=True, env=env)
                for row in json.loads(r.stdout.strip().splitlines()[-1]):
                    key = (side, row["what"], row["needle"])
                    got.setdefault(key, {**row, "ms": []})["ms"] += row["ms"]
        for (side, what, needle), row in got.items():
            record(part="resident", build=side, what=what, needle=needle, gib=a.gib, chunks=a.gib * 64, entries=row.get("entries"), **summarise(row["ms"]))
    if "file" in parts:
        d = Path(a.dir)
        d.mkdir(parents=True, exist_ok=True)
        if shutil.disk_usage(d).free < (a.file_gib + 2) << 30:
            record(part="file", not_taken=f"less than {a.file_gib + 2} GiB free under {d}")
        else:
            sys.path[:0] = [str(ROOT / "x-search_amd")]
            import corpus
            block = corpus.text_block(11, 0, 64 << 20, needle=b"Watson", lexicon=corpus.LEXICON_NOSH).tobytes()
            path = d / "corpus.txt"
            nblocks = a.file_gib * 16
            with open(path, "wb") as f:
                for _ in range(nblocks):
                    f.write(block)
            size = nblocks * len(block)
            env = dict(os.environ)
            for case, at in (("no hit", None), ("hit early", 4096), ("hit in the last chunk", size - (1 << 20))):
                old = poke(path, at, b" Sherlock ") if at is not None else b""  # (over a few words of one place of the file)
                subprocess.run(["cat", str(path)], stdout=subprocess.DEVNULL)  # into the page cache
                runs = {("this", "--max-count=1"): ["--max-count=1", "Sherlock", str(path)], ("this", "-l"): ["-l", "Sherlock", str(path)],
                        ("this", "-q"): ["-q", "Sherlock", str(path)], ("parent", "-c"): ["-c", "Sherlock", str(path)],
                        ("parent", "-l"): ["-l", "Sherlock", str(path)], ("parent", "plain"): ["Sherlock", str(path)]}
                ms = {k: [] for k in runs}
                for _ in range(a.runs):
                    for k, args in runs.items():
                        t, rc, nout = run_cli(trees[k[0]], args, env)
                        check(rc, "xsgrep " + " ".join(args[:-1]))
                        ms[k].append(t)
                for k in runs:
                    record(part="file", case=case, build=k[0], command="xsgrep " + k[1] + " Sherlock", file_gib=a.file_gib, **summarise(ms[k]))
                if at is not None:  # put the bytes back: the next case starts from the file without a hit
                    poke(path, at, old)
            path.unlink()
    if "bench" in parts:
        vals = {s: [] for s in trees}
        for _ in range(a.runs):
            for side, tree in trees.items():
                if a.deadline_s and time.monotonic() - t_start > a.deadline_s:
                    break
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"], cwd=tree, capture_output=True, text=True)
                check(r.returncode, f"bench.py ({side})")
                row = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                vals[side].append(row)
        for side, rows in vals.items():
            if not rows:
                record(part="bench", build=side, not_taken="no run fitted the deadline")
                continue
            keys = [k for k, v in rows[0].items() if isinstance(v, (int, float)) and not isinstance(v, bool)]
            record(part="bench", build=side, runs=len(rows),
                   metrics={k: {"median": statistics.median(r[k] for r in rows),
                                "spread": round(max(r[k] for r in rows) / max(min(r[k] for r in rows), 1e-12), 3)}
                            for k in keys if all(k in r for r in rows)})


if __name__ == "__main__":
    main()
