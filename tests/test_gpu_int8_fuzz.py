"""The fuzzer's int8 trial (tools/fuzz_parity.py int8_trial) on the device: one random cosine / dot table per trial
through the int8 first stage (SDB_TUNE_SKETCH = 4, 3) and the walks beside it (1, 0), held to the float64 model
(tests/int8_stage_model.py).  A random stream of its own: tests/test_gpu_fuzz.py's trials draw what they drew before.
tests/test_int8_fuzz_model.py runs the same draws without a GPU."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS = 6


def _fuzz():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_parity
    return fuzz_parity


@pytest.mark.parametrize("seed", [1, 20251002])
def test_int8_trials(oracle, seed):
    fz = _fuzz()
    for t in range(TRIALS):
        out = fz.int8_trial(np.random.default_rng([seed, t, 3]), spill_rng=fz.spill_generator(seed, t))
        for b in out["batches"]:
            assert b is None or b[0] <= b[1] <= b[2], (out["desc"], b)
