"""The staged hop's load schedule, read from the built library's disassembly (tools/kernel_table.py --memory-ops).

DESIGN.md section 4: a hop of a walk that asks for its copy rows ahead requests the rows of all 64 edges when the
adjacency row arrives and runs the visited-set test while they are in flight.  Two things in the compiled code decide
whether that happens, and neither shows in an answer:

* an argument read through cold_args() must be a scalar load and a pointer read through it a global one -- read as
  generic pointers they became flat loads, which count on both wait counters and can only be waited for with a full
  drain (`s_waitcnt vmcnt(0) lgkmcnt(0)`);
* from the first copy-row load of the hop to the visited-set test's first `ds_cmpst_rtn_b32` nothing may wait on
  vmcnt: a wait there puts the rows' flight in front of the test instead of under it.

No GPU: the code objects are taken out of semadb_amd/libsemadb_amd.so with the ROCm LLVM tools."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_table", os.path.join(ROOT, "tools", "kernel_table.py"))
kt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kt)

# every kernel of the two-precision hop that asks for its rows ahead: the int8 walks, and the float16 walks of rows of
# up to 384 floats -- cosine / dot and euclidean, plain and filtered
AHEAD_KERNELS = (["sdb::k_greedy_search<sdb::Int8Dist<%d>, 2, false, 8192u>" % ng for ng in (1, 2, 3)] +
                 ["sdb::k_greedy_search<sdb::PlainDist<%d, %s, true, 4, (sdb::Stage)1>, 2, %s, 8192u>" % (ng, l2, filt)
                  for ng in (1, 2, 3) for l2 in ("false", "true") for filt in ("false", "true")])


@pytest.fixture(scope="module")
def walk_kernels():
    if not os.path.exists(kt.SO):
        pytest.fail("semadb_amd/libsemadb_amd.so is not built")
    return kt.disassembly(kt.SO)


def test_the_library_has_every_walk_kernel_the_schedule_is_stated_for(walk_kernels):
    assert len(walk_kernels) > 100, "the walk kernels were not found in the disassembly"
    missing = [k for k in AHEAD_KERNELS if k not in walk_kernels]
    assert not missing, missing
    assert all(kt.AHEAD.match(k) for k in AHEAD_KERNELS)
    assert sorted(k for k in walk_kernels if kt.AHEAD.match(k)) == sorted(AHEAD_KERNELS)


def test_no_walk_kernel_has_a_flat_instruction(walk_kernels):
    bad = {}
    for name, ins in walk_kernels.items():
        flat = sorted({mn for mn, _ in ins if mn.startswith("flat_")})
        if flat:
            bad[name] = flat
    assert not bad, "flat instructions in %d walk kernels: %s" % (len(bad), sorted(bad.items())[:4])


@pytest.mark.parametrize("kernel", AHEAD_KERNELS)
def test_nothing_waits_on_vmcnt_between_the_copy_row_loads_and_the_visited_set_test(walk_kernels, kernel):
    ins = walk_kernels[kernel]
    want = kt.copy_row_loads(kernel)
    sp = kt.stage_span(ins, want)
    assert sp is not None, "no straight-line run of %d copy-row loads with a ds_cmpst_rtn_b32 behind it" % want
    # the stretch is the hop's: nothing but the run, and in front of it the adjacency row's load (the euclidean walks
    # test the copy's pointer first: their branch ends the stretch that holds that load)
    assert sp["loads"] in (want, want + 1), "%d vector loads in the hop's stretch, %d copy-row loads (and the adjacency row) expected" % (
        sp["loads"], want)
    print("%s: %d loads, %d instructions from the first to the ds_cmpst_rtn_b32" % (kernel, want, sp["cmpst"] - sp["first"]))
    assert not sp["vm_waits"], "s_waitcnt on vmcnt between the copy-row loads and the visited-set test: %s" % sp["vm_waits"]
    assert not sp["other_vmem"], "vector-memory instructions between the copy-row loads and the visited-set test: %s" % sp["other_vmem"]
