"""The scratch audit can fail.  A context's self-rewinding counters -- scr_count, fuse_cnt, fuse_flag,
chain_ctl, chain_done -- are what tests/dispatch_ledger.py and tests/test_gpu_ctx_sequences.py hold to zero after every
launch; this file is the evidence that the count they rely on is not blind: on a context that has run one pass, one word is
poked into each of the five buffers in turn, at the first word, one in the middle and the LAST word of the whole buffer (not
of the extent some launch happens to touch), and the audit reports exactly that buffer with exactly one word; the zero is
written back and the audit is clean again.  Nothing is ever launched on a poked context: it is deleted once the restore
has been confirmed."""
import numpy as np
import pytest

from fast_dnn_amd import api, formats as F

NAMES = ("scr_count", "fuse_cnt", "fuse_flag", "chain_ctl", "chain_done")


def test_scratch_names_are_the_five_self_rewinding_buffers():
    assert api.scratch_names() == NAMES


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1500], ids=["n300", "n1500"])  # one and several tiles of every counter array
def test_audit_reports_a_poked_word_of_every_buffer(mid_model_path, n):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path, device=0)
    ctx = dnn.getNewLazyContext(n)
    try:
        ctx.calculateUntilOutput(F.synth_features(n, 432, seed=3))
        clean = dict.fromkeys(NAMES, 0)
        assert ctx.scratchState() == clean, "a context that ran one pass is not clean: nothing can be shown on it"
        words = ctx.scratchWords()
        assert set(words) == set(NAMES) and all(w > 0 for w in words.values()), words
        # the layout's sizes for this net (fdnn_ctx_layout.hpp: ctx_layout), so that "the last word" is the buffer's
        cap = -(-n // 64) * 64
        xt_ld = -(-cap // 128) * 128
        npt = cap + 320
        assert words == {"scr_count": xt_ld // 64 * 2, "fuse_cnt": 8 * (npt // 128 + 2), "fuse_flag": (npt // 128 + 2) * 4, "chain_ctl": 16,
                         "chain_done": (npt // 256 + 2) * 8}, words
        for name in NAMES:
            for where, index in (("first", 0), ("middle", words[name] // 2), ("last", words[name] - 1)):
                for value in (1, 0x80000000):
                    ctx.scratchPoke(name, index, value)
                    got = ctx.scratchState()
                    ctx.scratchPoke(name, index, 0)  # (restored before anything is judged: a failure leaves no dirty context behind)
                    assert ctx.scratchState() == clean, f"{name}[{index}] ({where} word): the zero written back is not seen"
                    assert got == {**clean, name: 1}, f"{name}[{index}] ({where} word) = {value:#x}: the audit reports {got}"
        with pytest.raises(api.FdnnError):
            ctx.scratchPoke("chain_ctl", words["chain_ctl"], 1)  # one past the end: refused, nothing written
        with pytest.raises(api.FdnnError):
            ctx.scratchPoke("scr_count", -1, 1)
        assert ctx.scratchState() == clean
    finally:
        ctx.delete()  # (never used again: no launch sees what this test wrote)
        dnn.delete()


@pytest.mark.gpu
def test_process_wide_audit_adds_up_and_resets(mid_model_path):
    """The switch: off, nothing is counted; on, a released pooled context, a deleted explicit one and a debug entry point's own
    are counted, a poked (and never launched-on) context shows in the totals when it is destroyed, and reading resets them."""
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path, device=0)
    x = F.synth_features(200, 432, seed=4)
    zero = {**dict.fromkeys(NAMES, 0), "contexts": 0, "unreadable": 0}

    def totals():
        t = api.scratch_dirty()
        assert (t.pop("seconds") > 0) == (t["contexts"] > 0)  # (what the audits themselves cost: counted with them)
        return t

    try:
        api.scratch_audit(False)
        api.scratch_dirty()
        dnn.calculate(x)
        assert totals() == zero, "the audit counted with the switch off"
        api.scratch_audit(True)
        dnn.calculate(x)  # the pooled context goes back to the pool: one
        assert totals() == {**zero, "contexts": 1}
        assert totals() == zero, "reading did not reset the totals"
        ctx = dnn.getNewLazyContext(200)
        ctx.calculateUntilOutput(x)
        ctx.delete()  # an explicit context, destroyed: one
        dnn.layer0(x)  # the debug entry point's own context: two
        assert totals() == {**zero, "contexts": 2}
        ctx = dnn.getNewLazyContext(200)
        ctx.calculateUntilOutput(x)
        last = ctx.scratchWords()["fuse_flag"] - 1
        ctx.scratchPoke("fuse_flag", last, 7)
        ctx.scratchPoke("chain_done", 0, 1)
        ctx.delete()  # destroyed dirty, never launched on
        assert totals() == {**zero, "fuse_flag": 1, "chain_done": 1, "contexts": 1}
    finally:
        api.scratch_audit(False)
        api.scratch_dirty()
        dnn.delete()
