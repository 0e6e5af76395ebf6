"""The fuzzer's two-precision trial (tools/fuzz_parity.py two_precision_trial) without a GPU, on the draws of the short
soak (tests/test_gpu_fuzz.py: the same seeds, the same number of trials, the same random streams): every replay of the
two float64 models equals the oracle's walk (asserted inside the trial), lower <= upper everywhere, and the draws are
worth sending to the device -- of the batches whose routing has the stage at least three quarters prove something
(lower > 0), and summed over the soak lower >= 0.99 upper, for the plain and for the filtered walk.  The last two are
conditions on the draw distribution: a trial that passes on tables where nothing is provable says nothing about the
kernel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIALS = 12  # test_gpu_fuzz.py's default


def _fuzz():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_parity
    return fuzz_parity


@pytest.mark.parametrize("seed", [1, 20251002])
def test_two_precision_trial_draws(oracle, seed):
    fz = _fuzz()
    results = [fz.two_precision_trial(np.random.default_rng([seed, t, 2]), device=False) for t in range(TRIALS)]
    for r in results:
        for b in r["batches"]:
            for walk in ("plain", "filtered"):
                assert b[walk][0] <= b[walk][2], (r["desc"], b)
    sums = fz.two_precision_sums(results)
    print(seed, sums)
    for walk in ("plain", "filtered"):
        s = sums[walk]
        assert s["batches_with_stage"] >= 8, s
        assert 4 * s["with_lower_above_0"] >= 3 * s["batches_with_stage"], (walk, s)
        assert s["lower"] >= 0.99 * s["upper"], (walk, s)
