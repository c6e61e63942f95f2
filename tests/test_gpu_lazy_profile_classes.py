"""What profileBegin / profileEnd report for ONE lazy-entries call (lists, one set, per-segment sets; each on its MFMA path and
on the list kernels): which launches are bracketed as which kind.  The hidden layers run before the bracket, so only the
call's own scopes are counted: every path scores under one "output_gemm" scope -- the union path's build and score kernels
share it, the sets path's launches share it, the expand and rows kernels stand outside -- and finishes under one
"normalize" scope.  The numbers are those of the code before the calls got one driver (fdnn_lazy_entries.cpp).

Empty lists are left out on purpose: the list path opens an output scope for them and the union path does not."""
import numpy as np
import pytest

from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu
ROWS = 40  # one full 32-row frame tile and a partial one
WANT = {"l0": 0, "fix": 0, "hidden_gemm": 0, "output_gemm": 1, "normalize": 1}


@pytest.fixture(scope="module")
def setup(mid_model_path):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)  # (this module's own model: the union switch is a model's property)
    x = F.synth_features(ROWS, dnn.inputDimension(), seed=3)
    row_ptr, nodes = F.masks_to_lists(F.generate_masks(ROWS, dnn.outputDimension(), seed=11))
    assert np.diff(row_ptr).min() >= 1
    ctx = dnn.getNewLazyContext(ROWS)
    ctx.calculateUntilOutput(x)
    yield dnn, ctx, row_ptr, nodes
    ctx.delete()
    dnn.delete()


def lists_call(ctx, row_ptr, nodes):
    ctx.calculateForOutputNodesLists(row_ptr, nodes)


def set_call(ctx, row_ptr, nodes):
    ctx.calculateForOutputNodeSet(nodes[row_ptr[5]:row_ptr[6]])


def sets_call(ctx, row_ptr, nodes):
    a, b = nodes[row_ptr[5]:row_ptr[6]], nodes[row_ptr[7]:row_ptr[8]]
    ctx.calculateForOutputNodeSets([0, 32, ROWS], [0, a.size, a.size + b.size], np.concatenate((a, b)))


@pytest.mark.parametrize("name,call,set_kernel,union", [
    ("lists", lists_call, 0, 0),
    ("lists over unions", lists_call, 0, 1),
    ("set, MFMA kernel", set_call, 1, 0),
    ("set, list kernels", set_call, 2, 0),
    ("sets, MFMA kernel", sets_call, 0, 0),
    ("sets, list kernels", sets_call, 2, 0),
], ids=["lists", "lists_union", "set_mfma", "set_lists", "sets", "sets_lists"])
def test_profile_kinds_of_one_lazy_call(setup, name, call, set_kernel, union):
    dnn, ctx, row_ptr, nodes = setup
    try:
        api.set_kernel(set_kernel)
        dnn.setListsUnion(union)
        dnn.profileBegin()
        try:
            call(ctx, row_ptr, nodes)
        finally:
            prof = dnn.profileEnd()
    finally:
        api.set_kernel(0)
        dnn.setListsUnion(0)
    got = {k: prof[k]["launches"] for k in dnn.PROF_KINDS}
    print(f"\n[profile classes] {name}: {got}", flush=True)
    assert got == WANT
