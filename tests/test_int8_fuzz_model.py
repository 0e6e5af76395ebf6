"""The fuzzer's int8 trial (tools/fuzz_parity.py int8_trial) without a GPU, on the draws of tests/test_gpu_int8_fuzz.py:
every replay equals the oracle's walk (asserted inside the trial), lower <= upper everywhere, and the draws are worth
sending to the device: most batches keep the int8 copy and prove something, and summed over them lower >= 0.98 upper."""
import numpy as np
import pytest

from tests.test_gpu_int8_fuzz import TRIALS, _fuzz

pytestmark = []  # (not the GPU module's mark)


@pytest.mark.parametrize("seed", [1, 20251002])
def test_int8_trial_draws(oracle, seed):
    fz = _fuzz()
    recs = []
    for t in range(TRIALS):
        out = fz.int8_trial(np.random.default_rng([seed, t, 3]), device=False)
        recs += out["batches"]
    kept = [b for b in recs if b is not None]
    print(seed, len(recs), len(kept), sum(b[0] for b in kept), sum(b[2] for b in kept))
    assert all(b[0] <= b[2] for b in kept)
    assert 2 * len(kept) >= len(recs) and sum(1 for b in kept if b[0] > 0) * 4 >= 3 * len(kept)
    assert sum(b[0] for b in kept) >= 0.98 * sum(b[2] for b in kept)
