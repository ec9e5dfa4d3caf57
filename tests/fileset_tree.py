"""The temp tree the file-set tests search (tests/test_gpu_fileset.py, tests/test_gpu_fileset_cli.py) and what the oracle
says about every file of it.  About 60 files: an empty one, files of 1, 15, 16 and 17 bytes, one without a final newline,
one with bytes >= 0x80, one of 200 KiB (with CHUNK_BYTES = 64 KiB it is larger than a chunk: the delegated path), and
seeded word salad of 100 bytes to 12 KiB in two directory levels."""
import os

import numpy as np

import xsg
from per_chunk_model import file_results

CHUNK_BYTES = 64 << 10
BATCH_BYTES = 128 << 10  # several batches, the cuts between files

WORDS = [b"that", b"That", b"colour", b"color", b"COLOUR", b"running", b"going", b"x", b"aa", b"aaa", b"plain", b"words",
         b"zebra", b"the", b"thet", b"sing", b"THAT", b"Sherlock", b"Sher ock"]


def words_text(rng, nbytes: int, terminated: bool = True) -> bytes:
    out, size = [], 0
    while size < nbytes:
        w = WORDS[int(rng.integers(0, len(WORDS)))] + (b"\n" if rng.random() < 0.25 else b" ")
        out.append(w)
        size += len(w)
    b = bytearray(b"".join(out)[:nbytes])
    if terminated and b:
        b[-1] = 10
    return bytes(b)


def build(root) -> dict:
    """writes the tree under `root` -> {relative path: bytes}, in the byte-wise sorted depth-first order of xsgrep -r"""
    rng = np.random.default_rng(4711)
    files = {
        "a_empty.txt": b"",
        "a_len01.txt": b"x",
        "a_len15.txt": b"that colour aa\n",
        "a_len16.txt": b"x that colour a\n",
        "a_len17.txt": b"running that aa\n\n",
        "b_no_final_newline.txt": words_text(rng, 700) + b"x that colour running",
        "b_non_ascii.txt": words_text(rng, 900) + "grüße that colour\nSherlock über running\n".encode() + words_text(rng, 300),
        "c_large.txt": words_text(rng, 200 << 10),
    }
    for i in range(52):
        sub = ("", "d1/", "d1/deep/", "d2/")[i % 4]
        files[f"{sub}f{i:02d}.txt"] = words_text(rng, int(rng.integers(100, 12_000)), terminated=i % 7 != 0)
    files["d2/no_match.txt"] = b"plain words\nplain\n" * 20
    for rel, data in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    return {rel: files[rel] for rel in walk_order(root)}


def walk_order(root, rel=""):
    """xsgrep -r: depth-first, the entries of a directory in byte-wise sorted order, regular files only, links not followed"""
    out = []
    for name in sorted(os.listdir(os.path.join(root, rel)), key=os.fsencode):
        r = rel + name
        p = os.path.join(root, r)
        if os.path.islink(p):
            continue
        if os.path.isdir(p):
            out += walk_order(root, r + "/")
        elif os.path.isfile(p):
            out.append(r)
    return out


def chunks_of(path, data: bytes):
    """the blocks a search of this file alone sees: one chunk up to CHUNK_BYTES, else the plan of xsg_plan_chunks (host only)"""
    if len(data) <= CHUNK_BYTES:
        return [np.frombuffer(data, dtype=np.uint8)]
    plan = xsg.plan_chunks(str(path), CHUNK_BYTES)
    blocks = [np.frombuffer(data[int(c["original_offset"]):int(c["original_offset"]) + int(c["original_size"])], dtype=np.uint8) for c in plan]
    assert len(blocks) > 1 and sum(b.size for b in blocks) == len(data)
    return blocks


def want_file(oracle, kind, pat, pflags, flags, path, data):
    return file_results(oracle, kind, pat, pflags, flags, chunks_of(path, data))
