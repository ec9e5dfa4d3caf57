"""Shared helpers: load the committed golden fixtures and rebuild their inputs."""
import hashlib
import json
from pathlib import Path

import numpy as np

import corpus

GOLDEN = Path(__file__).resolve().parent / "golden"


def load(name):
    return json.loads((GOLDEN / name).read_text())


def make_input(spec) -> np.ndarray:
    kind = spec["kind"]
    if kind == "literal":
        return np.frombuffer(spec["text"].encode("latin-1"), dtype=np.uint8).copy()
    if kind == "small_alphabet":
        return corpus.small_alphabet(spec["seed"], spec["n"], spec["alphabet"].encode("latin-1"),
                                     spec.get("terminate", False))
    if kind == "text_block":
        a = corpus.text_block(spec["seed"], spec["index"], spec["n"],
                              needle=spec.get("needle", "Sherlock").encode("latin-1"),
                              needle_rate=spec.get("needle_rate", 2.76e-6))
        if spec.get("unterminated"):
            a = a[:-1].copy()
        for pos, s in spec.get("splice", []):
            b = s.encode("latin-1")
            p = pos if pos >= 0 else len(a) + pos
            a[p:p + len(b)] = np.frombuffer(b, dtype=np.uint8)
        return a
    raise ValueError(kind)


def generated_cases():
    """Yields (case_name, data, expect_entry) with the input's sha256 verified."""
    doc = load("ref_generated_vectors.json")
    for c in doc["cases"]:
        data = make_input(c["input"])
        assert data.size == c["len"], c["name"]
        assert hashlib.sha256(data.tobytes()).hexdigest() == c["sha256"], f"generator drift in {c['name']}"
        for e in c["expect"]:
            yield c["name"], data, e


def generated_icase_cases():
    """ignore_case vectors: expected values from the wrapper loops on the reference's simd::strcasestr
    (tests/golden/gen_golden.py: icase_cases)."""
    doc = load("ref_generated_vectors.json")
    for c in doc["icase_cases"]:
        data = make_input(c["input"])
        assert data.size == c["len"], c["name"]
        assert hashlib.sha256(data.tobytes()).hexdigest() == c["sha256"], f"generator drift in {c['name']}"
        for e in c["expect"]:
            yield c["name"], data, e


def ref_metafile(name: str, directory) -> Path:
    """Rebuilds the reference's test/files/<name> (one of its four .meta fixtures) byte for byte under `directory`
    from tests/golden/ref_metafiles.json + ref_metafile_mappings.xz (tests/golden/extract_ref_metafiles.py)."""
    import lzma
    doc = load("ref_metafiles.json")
    f = doc["files"][name]
    n = doc["n_mappings"]
    blob = lzma.decompress((GOLDEN / doc["mappings"]).read_bytes())
    assert len(blob) == 3 * n, "mapping table size"
    d = np.stack([np.frombuffer(blob[:2 * n], "<u2"), np.frombuffer(blob[2 * n:], "u1")], axis=1).astype(np.uint64)
    table = np.cumsum(d, axis=0, dtype=np.uint64).astype("<u8")
    parts, at = [np.array([f["compression_type"]], "<i4").tobytes()], 0
    for rec in f["records"]:
        parts += [np.array(rec, "<u8").tobytes(), table[at:at + rec[4]].tobytes()]
        at += rec[4]
    assert at == n, "the chunk records cover the mapping table"
    raw = b"".join(parts)
    assert len(raw) == f["file_bytes"] and hashlib.sha256(raw).hexdigest() == f["sha256"], f"{name} not rebuilt exactly"
    path = Path(directory) / name
    path.write_bytes(raw)
    return path


def digest(answers) -> str:
    """sha256 of a nest of lists / tuples of ints and bytes (numpy integers included): how tests/golden/ holds what the
    reference build answered on a test's seeded inputs without holding every answer"""
    def plain(x):
        if isinstance(x, (bytes, bytearray)):
            return {"b": bytes(x).hex()}
        if isinstance(x, np.integer):
            return int(x)
        if isinstance(x, np.ndarray):
            return x.tolist()
        raise TypeError(type(x))
    return hashlib.sha256(json.dumps(answers, default=plain, separators=(",", ":")).encode()).hexdigest()
