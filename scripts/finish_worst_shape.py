#!/usr/bin/env python3
"""The worst shape for the finishing form of the gated count (k_scan_fin): the bench shard (bench.py's templates and chunk
plan, 50 GiB by default) with the needle planted as the LAST WORD of every chunk, so that every chunk's end-of-chunk zone
holds an occurrence and its home tile walks the zone from an entry it has to look back for.  Times xsg_count_async of the
bench needle on the tuned binding (its verdict: the gate is on) and prints one JSON line; run it in the tree of either
build.
Usage: finish_worst_shape.py [--root TREE] [--gib 50] [--calls 10] [--build LABEL]"""
import argparse
import json
import sys
import types
from pathlib import Path

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]), help="the tree whose library and bench.py are used")
    ap.add_argument("--gib", type=float, default=50.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--build", default=None, help="a label copied into the line")
    a = ap.parse_args()
    root = Path(a.root).resolve()
    for p in (root, root / "x-search_amd", root / "oracle"):
        sys.path.insert(0, str(p))
    import torch

    import bench
    import corpus
    import xsg
    from xs_oracle import Oracle

    args = types.SimpleNamespace(chunk_mib=16, templates=32, seed=0x5EED)
    needle = b"Sherlock"
    blocks = [b.copy() for b in bench.template_blocks(args, needle)]
    for b in blocks:  # the needle as the chunk's last word
        b[b.size - len(needle):] = np.frombuffer(needle, dtype=np.uint8)
    orc = Oracle()
    tcount = np.array([orc.count(b, needle, False) for b in blocks], dtype=np.int64)
    tbytes = np.array([b.size for b in blocks], dtype=np.int64)
    nchunks = max(1, int(round(a.gib * 2**30 / (16 << 20))))
    plan = bench.chunk_plan(args, 0, nchunks)
    off, ln, cap = corpus.chunk_table(tbytes[plan])
    dev = torch.device("cuda", 0)
    shard_t = torch.empty(cap, dtype=torch.uint8, device=dev)
    dev_templates = [torch.from_numpy(b).to(dev) for b in blocks]
    for c in range(nchunks):
        t = dev_templates[int(plan[c])]
        shard_t[int(off[c]):int(off[c]) + t.numel()].copy_(t)
    torch.cuda.synchronize()
    del dev_templates
    goffs = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    ctx = xsg.Context(0)
    ctx.set_pattern(needle)
    shard = xsg.Shard(ctx, shard_t.data_ptr(), cap, xsg.make_chunks(off, ln, goffs))
    shard.tune(xsg.COUNT_MATCHES)  # builds the sketch, takes the verdict
    kernel = shard.scan_kernel_name(xsg.COUNT_MATCHES)
    stream = torch.cuda.Stream(device=dev)
    out = torch.zeros(xsg.NUM_COUNTERS, dtype=torch.int64, device=dev)
    expected = int(tcount[plan].sum())
    ms = []
    for i in range(a.calls + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out.fill_(-1)
        torch.cuda.synchronize()
        e0.record(stream)
        shard.count_async(xsg.COUNT_MATCHES, stream.cuda_stream, out.data_ptr())
        e1.record(stream)
        stream.synchronize()
        got = int(out[xsg.CTR_MATCHES].item())
        if got != expected:
            raise SystemExit(f"PARITY FAILURE: {got} != {expected}")
        if i >= 2:  # two untimed calls
            ms.append(e0.elapsed_time(e1))
    print(json.dumps({"build": a.build, "needle": "Sherlock", "shape": "the needle ends every chunk", "gib": a.gib, "bytes": int(ln.sum()),
                      "chunks": nchunks, "matches": expected, "kernel": kernel, "calls": a.calls, "ms": [round(x, 4) for x in ms],
                      "ms_min": round(min(ms), 4), "ms_median": round(float(np.median(ms)), 4), "ms_max": round(max(ms), 4)}), flush=True)


if __name__ == "__main__":
    main()
