"""Randomised differential trials (tools/fuzz_parity.py: device through the C ABI vs the oracle over random shapes,
metrics, parameters, data with ties and duplicates, build schedules, write sequences in rounds or one by one, a
quantizer attached mid-way; graphs edge for edge, plain / filtered / exact-scan searches and K1 bit for bit; plus
random product-quantizer fits / codecs and shard merges; plus one table per trial through the two-precision walks, plain
and filtered, held to the float64 models -- two_precision_trial; tests/test_two_precision_fuzz_model.py runs the same
draws without a GPU and asserts that the models prove something on them).

The soak's first runs exposed two defects, each now pinned by a deterministic test of its own:
  * a delete leaving more stragglers than the start node's 64-entry row holds (the reference's start node has no
    bound, prune.go:131-151) -> tests/test_gpu_delete.py::test_start_node_overflow_list;
  * a store switched to the product quantizer kept per-row cached distances made with the old distance function
    -> tests/test_gpu_pq.py::test_quantizer_attached_to_a_device_built_graph.
A short fresh soak runs here on every `pytest -m gpu` (SDB_SOAK_TRIALS trials per seed, 12 by default: the suite has a
time budget; the long soaks are run with tools/fuzz_parity.py and tallied in DESIGN.md)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fuzz():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_parity
    return fuzz_parity


@pytest.mark.parametrize("seed", [1, 20251002])
def test_fuzz_short_soak(oracle, monkeypatch, seed):
    fz = _fuzz()
    for t in range(int(os.environ.get("SDB_SOAK_TRIALS", 12))):
        rng = np.random.default_rng([seed, t])
        fz.merge_trial(rng)
        fz.pq_trial(rng)
        fz.flat_trial(rng)
        fz.trial(rng, t, fz.spill_generator(seed, t))
        # (streams of their own: the four trials above draw what they drew before this one, and the repeats under a
        # lowered hash_limit, existed)
        fz.two_precision_trial(np.random.default_rng([seed, t, 2]), spill_rng=fz.spill_generator(seed, t))
