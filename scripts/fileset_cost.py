#!/usr/bin/env python3
"""What a file set costs against what it replaces: one xsg.Job per file (profiles/fileset_ab.jsonl).

Generated text (corpus.py) written as files under --dir, three shapes:
  small   --small-files files of 4-64 KiB            (default 20 000)
  medium  256 files of 4 MiB
  large   4 files of 64 MiB                          (larger than chunk_bytes: the file set delegates them to the job
                                                      pipeline, so parity within the spread is the expectation)
and three searches: count-lines and lines of a rare literal (the planted needle), and count-lines of an 8-word list.
Two SIDES do the same work on the same files with the same CPUs:
  fileset   this build: ONE xsg.FileSet over all paths, joined, every file's result fetched
  jobs      the PARENT commit's library (--parent TREE: a checkout of the parent with its library built): a loop of one
            xsg.Job per file, joined, its result fetched
Every timed run is a process of its own (`--child`), so each side loads its own library; the sides alternate, --runs runs
each, and the order flips from run to run.  A child opens its device and searches one small file before the clock starts
(HIP start-up is not what is compared), and the files are read once before the first run (a warm page cache on both
sides).  The two sides' results are compared for equality at the sizes timed before a number is written.  One JSON line per
(shape, search): every run's seconds per side, medians, max / min per side, and the ratio of the medians."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
RARE = b"Sherlock"
WORDS = [b"Sherlock", b"zeppelin", b"quagmire", b"Moriarty", b"xylophone", b"Baskerville", b"juxtapose", b"kumquat"]
SEARCHES = {"count_lines": ("count", RARE, False), "lines": ("lines", RARE, False), "count_lines_list8": ("count", b"\n".join(WORDS), True)}


def make_files(root: Path, shape: str, small_files: int, seed: int):
    sys.path.insert(0, str(ROOT / "x-search_amd"))
    import corpus
    d = root / shape
    if (d / "DONE").exists():
        return sorted(str(p) for p in d.rglob("*.txt"))
    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    if shape == "small":
        sizes = rng.integers(4 << 10, (64 << 10) + 1, size=small_files)
    elif shape == "medium":
        sizes = np.full(256, 4 << 20)
    else:
        sizes = np.full(4, 64 << 20)
    # slices of a few generated templates, each made to end in a newline: the text is corpus.py's, the cost of making it is not 20 000-fold
    templates = [corpus.text_block(seed, i, (64 << 20) + 4096, needle_rate=2e-5) for i in range(2)]
    for i, n in enumerate(sizes):
        t = templates[i % len(templates)]
        at = int(rng.integers(0, t.size - int(n)))
        b = t[at:at + int(n)].copy()
        b[-1] = 10
        sub = d / f"{i // 1000:03d}"
        sub.mkdir(exist_ok=True)
        (sub / f"f{i:06d}.txt").write_bytes(b.tobytes())
    (d / "DONE").write_text("ok\n")
    return sorted(str(p) for p in d.rglob("*.txt"))


def child(a):
    """one timed run of one side: prints {"seconds": ..., "digest": ..., "total": ...}"""
    tree = Path(a.parent) if a.child == "jobs" else ROOT
    sys.path.insert(0, str(tree / "x-search_amd"))
    import xsg  # this side's binding and library
    paths = Path(a.paths).read_text().split("\n")
    kind, pat, is_list = SEARCHES[a.search]
    mode = xsg.COUNT_LINES if kind == "count" else xsg.LINES
    xsg.Job(pat, paths[0], mode, pattern_is_list=is_list).result()  # the device is open, the code objects are loaded
    h = hashlib.sha256()
    total = 0
    t0 = time.perf_counter()
    if a.child == "fileset":
        fs = xsg.FileSet(pat, paths, mode, pattern_is_list=is_list, num_readers=a.readers).join()
        assert not fs.status().any()
        counts = fs.counts()
        if kind == "lines":
            for line in fs._entries(0, int(fs.file_ptr()[-1])):
                h.update(line + b"\n")
        seconds = time.perf_counter() - t0
        h.update(counts.tobytes())
        total = int(counts.sum())
    else:
        counts = np.zeros(len(paths), dtype=np.uint64)
        for f, p in enumerate(paths):
            j = xsg.Job(pat, p, mode, num_threads=1, num_max_readers=1, pattern_is_list=is_list)
            r = j.result()
            if kind == "lines":
                counts[f] = len(r)
                for line in r:
                    h.update(line + b"\n")
            else:
                counts[f] = r
            j.close()
        seconds = time.perf_counter() - t0
        h.update(counts.tobytes())
        total = int(counts.sum())
    print(json.dumps({"seconds": seconds, "digest": h.hexdigest(), "total": total}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="", help="a tree of the parent commit with x-search_amd/lib/libxsg.so built")
    ap.add_argument("--dir", default="/tmp/xsg_fileset_cost")
    ap.add_argument("--shapes", default="small,medium,large")
    ap.add_argument("--searches", default=",".join(SEARCHES))
    ap.add_argument("--small-files", type=int, default=20_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--readers", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fileset_ab.jsonl"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--paths", default="", help=argparse.SUPPRESS)
    ap.add_argument("--search", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent:
        sys.exit("--parent TREE is required: the baseline is the parent commit's library")
    root = Path(a.dir)
    with open(a.out, "a") as out:
        for shape in a.shapes.split(","):
            paths = make_files(root, shape, a.small_files, a.seed)
            nbytes = 0
            for p in paths:  # a warm page cache for both sides
                nbytes += len(Path(p).read_bytes())
            plist = root / f"{shape}.paths"
            plist.write_text("\n".join(paths))
            for search in a.searches.split(","):
                secs = {"fileset": [], "jobs": []}
                digests = set()
                for run in range(a.runs):
                    for side in (("fileset", "jobs") if run % 2 == 0 else ("jobs", "fileset")):
                        cmd = [sys.executable, __file__, "--child", side, "--parent", a.parent, "--paths", str(plist), "--search", search,
                               "--readers", str(a.readers)]
                        # (a child needs no torch: without it a process is up in a fraction of the time)
                        r = subprocess.run(cmd, check=True, capture_output=True, text=True, env=dict(os.environ, XSG_NO_TORCH_PRELOAD="1"))
                        r = json.loads(r.stdout.strip().split("\n")[-1])
                        secs[side].append(r["seconds"])
                        digests.add((r["digest"], r["total"]))
                assert len(digests) == 1, f"{shape} {search}: the two sides report different results"
                med = {s: float(np.median(v)) for s, v in secs.items()}
                rec = {"shape": shape, "files": len(paths), "bytes": nbytes, "search": search, "results": next(iter(digests))[1],
                       "cpus": len(os.sched_getaffinity(0)), "runs": a.runs, "seconds": secs, "median": med,
                       "max_over_min": {s: max(v) / min(v) for s, v in secs.items()}, "fileset_over_jobs": med["fileset"] / med["jobs"]}
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()


if __name__ == "__main__":
    main()
