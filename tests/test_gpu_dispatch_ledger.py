"""Every case of the dispatch ledger (tests/dispatch_ledger.py) on the GPU with the launch recorder on: the set of kernel
instances the case launches equals its expected set -- in both directions: a selection rule that drifts to another kernel
fails as loudly as a kernel that is never reached -- and what it computes is the oracle's (u8 activations and int32
accumulators bit-exact, soft-max <= 2e-6, NaN pattern, masked-out entries one value per row).  Every case's span also runs
under the scratch audit: each context the case used left its self-rewinding counters at zero, at least
one context was looked at, and the model's fault counters did not move; every case records how many contexts were audited
and what the audits themselves cost (record_property; the module prints the totals, visible with -s)."""
import pytest

import dispatch_ledger as L
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def recorder():
    yield
    api.launch_record(False)
    L.release_models()
    t = L.AUDIT_TOTAL
    print(f"\n[dispatch ledger] scratch audit: {t['contexts']} contexts over {t['cases']} cases, {t['seconds']:.3f} s spent auditing")


@pytest.mark.parametrize("case", L.CASES, ids=[c.id for c in L.CASES])
def test_case_launches_its_instances_and_matches_the_oracle(case, record_property):
    got = L.run_case_in_child(case) if case.env else L.run_case(case)
    want = L.EXPECT[case.id]
    assert got == want, f"launched but not expected: {sorted(got - want)}; expected but not launched: {sorted(want - got)}"
    assert L.LAST_AUDIT.get("contexts", 0) > 0, f"{case.id}: no context was audited"
    record_property("audited_contexts", L.LAST_AUDIT["contexts"])
    record_property("audit_seconds", L.LAST_AUDIT.get("seconds", 0.0))
