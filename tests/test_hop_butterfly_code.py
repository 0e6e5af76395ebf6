"""The int8 walk's hop, read from the built library's disassembly (tools/kernel_table.py): two forms that no answer shows.

* The transposing butterfly (walk_stage.h edge_sums) exchanges through v_permlane16_swap and DPP adds: the kernel holds
  no ds_swizzle_b32 (31 before, one per exchange, each a trip through the LDS pipe behind two selects).
* The copy rows' slots reach their lanes by ds_bpermute (FirstStage::begin): between the arrival of the adjacency row and
  the first copy-row load there is no v_readlane (64 before, with 64 moves and 32 selects), and the 32 source lanes are
  the instruction's offset field, not 32 registers.

No GPU: the code objects are taken out of semadb_amd/libsemadb_amd.so with the ROCm LLVM tools."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_table", os.path.join(ROOT, "tools", "kernel_table.py"))
kt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kt)

INT8_KERNELS = ["sdb::k_greedy_search<sdb::Int8Dist<%d>, 2, false, 8192u>" % ng for ng in (1, 2, 3)]


@pytest.fixture(scope="module")
def walk_kernels():
    if not os.path.exists(kt.SO):
        pytest.fail("semadb_amd/libsemadb_amd.so is not built")
    return kt.disassembly(kt.SO)


@pytest.mark.parametrize("kernel", INT8_KERNELS)
def test_the_butterfly_does_not_go_through_the_lds_pipe(walk_kernels, kernel):
    ins = walk_kernels[kernel]
    assert sum(mn == "ds_swizzle_b32" for mn, _ in ins) == 0
    assert sum(mn.startswith("v_permlane16_swap") for mn, _ in ins) >= 16, "the stride-16 exchanges are not there"


@pytest.mark.parametrize("kernel", INT8_KERNELS)
def test_the_copy_row_slots_come_by_bpermute(walk_kernels, kernel):
    ins = walk_kernels[kernel]
    sp = kt.stage_span(ins, 32)
    assert sp is not None
    first = sp["first"]
    # the adjacency row: the last vector load in front of the run, and the first wait on vmcnt behind it
    adj = max(j for j in range(first) if kt.is_vmem_load(ins[j][0]))
    assert ins[adj][0] == "global_load_dword", ins[adj]
    arrived = next(j for j in range(adj + 1, first) if ins[j][0] == "s_waitcnt" and "vmcnt" in ins[j][1])
    between = [mn for mn, _ in ins[arrived:first]]
    print("%s: %d instructions from the adjacency row's arrival to the first copy-row load" % (kernel, len(between)))
    assert not [mn for mn in between if mn.startswith("v_readlane")]
    # (the scheduler may put later pairs' permutes behind the first pairs' loads: counted up to the run's last load)
    perm = [ops for mn, ops in ins[arrived:sp["last"]] if mn == "ds_bpermute_b32"]
    assert len(perm) == 32, len(perm)
    assert sum("offset:" in ops for ops in perm) == 31, "the source lanes are not in the offset field"
