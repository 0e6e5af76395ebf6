"""CPU: the conditions under which parity with tests/rerank_model.py on the device (tests/test_gpu_rerank.py) means
something, asserted on exactly the tables and queries that test uses, and the ABI's two new entry points.

  * on a store without a quantizer the model is the plain search (ids and distance bits, every query);
  * on every quantized fixture re-ranking 25 and 50 candidates changes the top 10 of at least 16 of the 32 queries;
  * mean recall@10 against the exact top 10 does not fall from rerank 10 to 25 to 50."""
import os
import re

import numpy as np
import pytest

from tests import rerank_model as rm
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CHANGED = 16  # of rm.NQ = 32 queries


def test_header_and_signature_table_have_both_entry_points():
    from semadb_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "semadb_amd.h")).read(), flags=re.S)
    for name, n_args in (("sdb_index_search_batch_rerank", 14), ("sdb_index_search_batch_bitmap_rerank", 15)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/semadb_amd.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args and args[5] == "uint32_t rerank", args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+SDB_ABI_VERSION\s+2\b", text)


@pytest.mark.parametrize("metric", rm.METRICS)
@pytest.mark.parametrize("d", [100, 384])
def test_model_on_a_plain_store_is_the_plain_search(oracle, metric, d):
    fx = rm.plain_fixture(metric, d)
    for k in range(fx.q.shape[0]):
        want = fx.o.search(fx.q[k], rm.LIMIT, rm.L)
        for r in rm.RERANKS:
            ids, e, _ = rm.rerank(oracle, fx.o, fx.ids, fx.vecs, fx.metric, fx.q[k], rm.LIMIT, rm.L, r)
            assert np.array_equal(ids, want[0]) and np.array_equal(bits(e), bits(want[1])), (k, r)


def _conditions(oracle, fx, what):
    got = rm.recall_and_changes(oracle, fx)
    print(what, {r: (round(v[0], 3), v[1]) for r, v in got.items()})
    for k in range(rm.NQ):  # rerank == limit only reorders: the same ten ids
        assert sorted(rm.rerank(oracle, fx.o, fx.ids, fx.vecs, fx.metric, fx.q[k], rm.LIMIT, rm.L, 10)[0]) == \
            sorted(fx.o.search(fx.q[k], rm.LIMIT, rm.L)[0]), k
    assert got[25][1] >= MIN_CHANGED and got[50][1] >= MIN_CHANGED, (what, got)
    assert got[10][0] <= got[25][0] <= got[50][0], (what, got)
    return got


@pytest.mark.parametrize("metric", rm.METRICS)
@pytest.mark.parametrize("d,M,K,n", rm.PQ_SHAPES)
def test_product_quantizer_fixtures_change_under_reranking(oracle, metric, d, M, K, n):
    got = _conditions(oracle, rm.pq_fixture(metric, d, M, K, n), ("pq", metric, d, M, K))
    if (d, M, K, n) in rm.PQ_TABLE:  # the oracle alone: every query's top 10 changes on the parity test's own tables
        assert got[25][1] == rm.NQ and got[50][1] == rm.NQ, got


@pytest.mark.parametrize("kind,d", rm.BQ_CASES)
def test_binary_quantizer_fixtures_change_under_reranking(oracle, kind, d):
    _conditions(oracle, rm.bq_fixture(kind, d), (kind, d))
