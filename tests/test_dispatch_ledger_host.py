"""The dispatch ledger against the library's table of launch names -- no GPU needed: every name the library can launch
is either in the expected set of a ledger case or on the ledger's exclusion list with its reason.  A new launch branch
without a covering case fails here, on any machine."""
import dispatch_ledger as L
from fast_dnn_amd import api


def test_every_launch_name_is_covered_or_excluded_with_a_reason():
    table = api.launch_names()
    assert len(table) > 100 and "splice" in table and "gemm.out.ft320.fused_masked" in table
    covered = set().union(*L.EXPECT.values())
    ablation = {n for n, flags in table.items() if flags & api.LAUNCH_ABLATION}
    unknown = (covered | set(L.EXCLUDED)) - set(table)
    assert not unknown, f"the ledger names instances the library does not have: {sorted(unknown)}"
    assert not covered & set(L.EXCLUDED), f"excluded although a case launches them: {sorted(covered & set(L.EXCLUDED))}"
    assert not covered & ablation, f"a case expects an ablation-only instance: {sorted(covered & ablation)}"
    assert not ablation & set(L.EXCLUDED), "ablation-only names are excluded by their flag, not by the list"
    missing = set(table) - covered - set(L.EXCLUDED) - ablation
    assert not missing, f"launch branches without a ledger case: {sorted(missing)}"
    for name, why in L.EXCLUDED.items():
        assert ".hip" in why or ".cpp" in why, f"{name}: an exclusion names the code that makes it unreachable"


def test_the_ledger_is_well_formed():
    ids = [c.id for c in L.CASES]
    assert len(ids) == len(set(ids))
    assert set(L.EXPECT) == set(ids), sorted(set(L.EXPECT) ^ set(ids))
    for c in L.CASES:
        assert set(c.must) <= L.EXPECT[c.id], f"{c.id}: exists for {sorted(set(c.must) - L.EXPECT[c.id])}, which its expected set lacks"
        assert c.entry in L._ENTRIES or c.entry in ("load", "blob")
    # load-time kernels are expected by the load cases and by no other
    load_time = {n for n, flags in api.launch_names().items() if flags & api.LAUNCH_LOAD_TIME}
    for c in L.CASES:
        if c.entry not in ("load", "blob"):
            assert not L.EXPECT[c.id] & load_time, c.id


def test_row_sample_of_the_big_net_cases():
    for n, tile in ((10241, 320), (9728, 256), (513, 320), (20480, 320)):
        idx = L.sample_rows(n, tile, seed=n)
        assert idx[0] == 0 and idx[-1] == n - 1 and len(idx) >= min(n, 70) and len(set(idx)) == len(idx)
        for target in (n / 2, n):
            m = int(round(target / tile)) * tile
            assert all(r in idx for r in (m - 1, m) if 0 <= r < n)
