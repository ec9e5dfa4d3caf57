#!/usr/bin/env python3
"""Stores the reference's four .meta fixtures (test/files/sample{,.xslz4,.xslz4hc,.xszst}.meta, 3 060 484 bytes each)
compactly enough to commit, so that the tests can rebuild them byte for byte without the reference tree.

Usage: extract_ref_metafiles.py <reference>/test/files

Layout of a metafile (little-endian, packed): int32 compression_type, then per chunk the five u64 words
original_offset, actual_offset, original_size, actual_size, n, and n x {u64 byte offset, u64 line index}.

The four files carry the same mapping table and differ only in their compression type and chunk records, so:
  tests/golden/ref_metafiles.json        per file: compression type, chunk records, size and sha256 of the whole file
  tests/golden/ref_metafile_mappings.xz  the shared table, delta-coded: u16 byte-offset deltas of every entry, then u8
                                         line-index deltas of every entry (the first entry's deltas are from (0, 0))
golden_util.ref_metafile() rebuilds a file and checks its sha256.  Only data is taken.
"""
import hashlib
import json
import lzma
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
NAMES = ("sample.meta", "sample.xslz4.meta", "sample.xslz4hc.meta", "sample.xszst.meta")


def parse(raw: bytes):
    ct = int(np.frombuffer(raw[:4], "<i4")[0])
    pos, records, maps = 4, [], []
    while pos < len(raw):
        rec = [int(x) for x in np.frombuffer(raw[pos:pos + 40], "<u8")]
        pos += 40
        maps.append(np.frombuffer(raw[pos:pos + 16 * rec[4]], "<u8").reshape(-1, 2))
        pos += 16 * rec[4]
        records.append(rec)
    return ct, records, np.concatenate(maps)


def main(src: Path):
    files, table = {}, None
    for name in NAMES:
        raw = (src / name).read_bytes()
        ct, records, maps = parse(raw)
        if table is None:
            table = maps
        assert np.array_equal(maps, table), f"{name}: mapping table differs from {NAMES[0]}'s"
        files[name] = {"compression_type": ct, "records": records, "file_bytes": len(raw),
                       "sha256": hashlib.sha256(raw).hexdigest()}
    d = np.diff(table.astype(np.int64), axis=0, prepend=0)
    assert d.min() >= 0 and d[:, 0].max() < 1 << 16 and d[:, 1].max() < 1 << 8
    blob = d[:, 0].astype("<u2").tobytes() + d[:, 1].astype("u1").tobytes()
    (OUT / "ref_metafile_mappings.xz").write_bytes(lzma.compress(blob, preset=9 | lzma.PRESET_EXTREME))
    doc = {"generator": "tests/golden/extract_ref_metafiles.py", "source": "reference test/files/*.meta",
           "mappings": "ref_metafile_mappings.xz", "n_mappings": int(len(table)), "files": files}
    (OUT / "ref_metafiles.json").write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(table)} mappings, {(OUT / 'ref_metafile_mappings.xz').stat().st_size} bytes compressed")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
