#!/usr/bin/env python3
"""profiles/<tag>_pmc_traffic.json from the rocprofv3 --pmc passes of scripts/gpu_profiles.sh (FETCH_SIZE and WRITE_SIZE,
collected separately, one pair of passes per kernel instantiation): HBM bytes per k_scan launch, with the gfx950
correction of MI355X_MICROARCH.md's HBM section (FETCH_SIZE counts a 128-byte request as 64 bytes -> read bytes =
2 x FETCH_SIZE x 1024; WRITE_SIZE x 1024 is exact).
Usage: pmc_traffic.py [--gated] <BENCH json> <tag> <fetch csv> <write csv> [<fetch csv> <write csv> ...]
--gated: the timed pass is the sketch-gated one, one kernel per step -- k_scan<..., GATED>, a bounded grid of persistent
workgroups that selects and scans, or its finishing form k_scan_fin<KIND, LOADS, ALIGNED> (a plain match count's only
launch).  Only those launches are averaged (the same run also launches ungated k_scan at full size); where the run holds
k_scan_fin launches they are the timed pass and the storing form is left out.  The BENCH json may be a plain run's line
(no roofline block: the algorithmic bytes are the shard's).  k_sketch_build's traffic, once per binding, is reported
beside it where the passes saw it."""
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def is_gated(name):
    """k_scan<KIND, NL, LINES, EMIT, LOADS, ICASE, ALIGNED, GATED>: the eighth template argument"""
    args = name.split("k_scan<", 1)[1].split(">", 1)[0].split(",")
    return len(args) == 8 and args[7].strip() == "true"


def avg_counter(path, counter, kernel="k_scan<", gated=False, name=None):
    """average over the FULL-SHARD launches of `kernel` only (largest grid): the library's hot-filter probe also launches
    k_scan, on a 2 GiB prefix of the shard"""
    rows, fin = [], []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if row["Counter_Name"] != counter:
                continue
            if name is not None and row["Kernel_Name"] != name:
                continue
            rec = (int(row["Grid_Size"]), float(row["Counter_Value"]), row["Kernel_Name"])
            if gated and kernel == "k_scan<" and "k_scan_fin<" in row["Kernel_Name"]:
                fin.append(rec)
            elif kernel in row["Kernel_Name"] and not (gated and kernel == "k_scan<" and not is_gated(row["Kernel_Name"])):
                rows.append(rec)
    rows = fin or rows  # the finishing form, where it ran, is the timed pass
    if not rows:
        raise SystemExit(f"no {counter} rows for {kernel} in {path}")
    full = max(g for g, _, _ in rows)
    vals = [v for g, v, _ in rows if g == full]
    names = sorted({n for g, _, n in rows if g == full})
    return sum(vals) / len(vals), len(vals), names


def main():
    argv = [x for x in sys.argv[1:] if x != "--gated"]
    gated = "--gated" in sys.argv[1:]
    bench_json, tag = argv[0:2]
    pairs = argv[2:]
    bench = json.loads(Path(bench_json).read_text().splitlines()[-1])
    alg = bench["roofline"]["algorithmic_bytes_per_launch"] if "roofline" in bench else bench["config"]["bytes_per_gpu"]
    build = {}
    by = {}
    for fetch_csv, write_csv in zip(pairs[0::2], pairs[1::2]):
        _, _, names = avg_counter(fetch_csv, "FETCH_SIZE", gated=gated)
        if len(names) != 1 and not gated:
            raise SystemExit(f"{fetch_csv}: full-shard launches of more than one instantiation: {names}")
        for name in names:  # (a gated run that tunes launches both hot-filter instantiations at full size: one entry each)
            fetch_kb, nf, _ = avg_counter(fetch_csv, "FETCH_SIZE", gated=gated, name=name)
            write_kb, nw, _ = avg_counter(write_csv, "WRITE_SIZE", gated=gated, name=name)
            rd, wr = 2.0 * fetch_kb * 1024.0, write_kb * 1024.0
            key = name.replace("void ", "").split("(")[0]  # "xsg::k_scan<3, false, false, false, 4, false, true>"
            by[key] = {"FETCH_SIZE_KB_avg": fetch_kb, "WRITE_SIZE_KB_avg": write_kb, "launches_averaged": [nf, nw],
                       "hbm_read_bytes_per_launch": rd, "hbm_write_bytes_per_launch": wr, "hbm_bytes_per_launch": rd + wr,
                       "ratio_traffic_over_algorithmic": (rd + wr) / alg}
        if gated:  # the sketch build of the binding, where the passes saw it
            try:
                bf, nbf, bn = avg_counter(fetch_csv, "FETCH_SIZE", kernel="k_sketch_build")
                bw, nbw, _ = avg_counter(write_csv, "WRITE_SIZE", kernel="k_sketch_build")
                build[bn[0].replace("void ", "").split("(")[0]] = {
                    "launches_averaged": [nbf, nbw], "hbm_read_bytes_per_launch": 2.0 * bf * 1024.0, "hbm_write_bytes_per_launch": bw * 1024.0}
            except SystemExit:
                pass
    out = {
        "timed_kernel": bench["roofline"]["kernel"] if "roofline" in bench else sorted(by),
        "pattern": bench["config"]["pattern"],
        "config": bench["config"]["workload"],
        "bytes_per_gpu": bench["config"]["bytes_per_gpu"],
        "algorithmic_bytes_per_launch": alg,
        "correction": "HBM read bytes = 2 x FETCH_SIZE x 1024 (gfx950 counts 128-B requests as 64 B, "
                      "MI355X_MICROARCH.md HBM section); WRITE_SIZE x 1024 exact",
        "by_kernel": by,
        **({"sketch_build": build} if build else {}),
        "collected": (f"rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes of the bench command (plain, or "
                      f"`XSG_HOT=0 python3 bench.py --full --steps 2 --warmup 1 --kernel-iters 1 --no-cpu-baseline --e2e-gib 0 "
                      f"--configs-gib 0 --no-regex --cli-gib 0`); only the gated pass's launches are averaged (k_scan_fin where "
                      f"it ran, else the GATED k_scan); written by this script, nothing edited by hand") if gated else
                     f"rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes per instantiation, pinned with "
                     f"XSG_HOT / XSG_TUNE at the timed run's stagger (scripts/gpu_profiles.sh {tag}); written by this script, "
                     f"nothing edited by hand",
    }
    (ROOT / "profiles" / f"{tag}_pmc_traffic.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
