"""The committed call sequences of tests/call_sequences.py once more with the sketch built before the first eligible pass
of every binding (XSG_SKETCH=1, XSG_SKETCH_MIN_BYTES=0): whatever order the calls come in -- re-binds, rewritten bytes,
pattern changes, list passes, timing loops between the counts -- a gated pass must give what the model predicts."""
import os

import pytest

import call_sequences as cs
import test_gpu_call_sequences as replayer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", list(range(cs.N_SEQUENCES)))
def test_generated_sequence_with_the_sketch(seed, oracle):
    env = {"XSG_SKETCH": "1", "XSG_SKETCH_MIN_BYTES": "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        replayer.replay(oracle, cs.sequences()[seed], seed)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
