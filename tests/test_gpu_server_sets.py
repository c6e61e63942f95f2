"""Set submissions through the scoring loop (fdnn_server_submit_lazy_set / fdnn_server_submit_raw_set): each utterance with
its own node set, coalesced with the other callers' set submissions, the pieces scored as the segments of one sets call per
batch (fdnn_sets.hip) -- the dense output layer never runs.  Every result's bytes are those of fdnn_calculate_lazy_set on that
utterance alone, whatever the packer put together; a request split over two batches, raw frames, and set, dense and bit-mask
submissions sharing one loop."""
import threading

import numpy as np
import pytest

import lazy_set_cases as SC
from fast_dnn_amd import api, convert as CV, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
TIGHT = SC.TIGHT
O = 1000


@pytest.fixture(scope="module")
def dnn(mid_model_path):
    api.set_kernel(1)
    d = api.QuantizedDnn.loadFromFile(mid_model_path)
    yield d
    d.delete()
    api.set_kernel(0)


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def the_sets():
    """lens 0, 1, 65, 129: the sets of the lazy_set_cases fixtures"""
    return [SC.CASES[f"mid.len{L}"].build() for L in (0, 1, 65, 129)]


def run_threads(n, body):
    errors = []

    def guarded(k):
        try:
            body(k)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=guarded, args=(k,)) for k in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_set_submissions_are_coalesced_and_skip_the_output_layer(dnn, mid_model_path):
    lens = [100, 37, 20, 64, 100, 91, 33, 100, 58, 77]
    utts = [F.synth_features(n, 432, seed=900 + i) for i, n in enumerate(lens)]
    sets = the_sets()
    which = [i % 4 for i in range(len(utts))]
    alone = [dnn.calculateLazySet(x, sets[which[i]]) for i, x in enumerate(utts)]
    orc = Oracle(mid_model_path)
    for i in (0, 2, 3):  # ... which are the oracle's lazy rows
        masks = np.zeros((lens[i], O), np.int8)
        masks[:, sets[which[i]]] = 1
        rp = SC.uniform_row_ptr(lens[i], sets[which[i]].size)
        rows = F.lists_to_rows(rp, np.tile(sets[which[i]], lens[i]), alone[i][0].ravel(), alone[i][1], O)
        assert np.abs(rows - orc.lazy(utts[i], masks)).max() <= TIGHT
    srv = api.ScoringServer(dnn, max_frames=1024, depth=3, linger_us=200)
    results, lock = [], threading.Lock()
    api.launch_reset()
    api.launch_record(True)
    tb, sb = api.sets_launches(), api.set_launches()
    try:
        def worker(w):
            for j in range(len(utts)):
                i = (j + w) % len(utts)
                probs = np.full((lens[i], sets[which[i]].size), -7.0, dtype=np.float32)
                inactive = np.full(lens[i], -7.0, dtype=np.float32)
                t, _, _ = srv.submitLazySet(utts[i], sets[which[i]].copy(), probs, inactive)  # (the set is copied at submit)
                srv.wait(t)
                with lock:
                    results.append((i, probs, inactive))

        run_threads(8, worker)
        counts = api.launch_counts()
    finally:
        api.launch_record(False)
    ta, sa = api.sets_launches(), api.set_launches()
    assert len(results) == 8 * len(utts)
    for i, probs, inactive in results:
        assert same_bytes(probs, alone[i][0]) and same_bytes(inactive, alone[i][1]), i
    st = srv.stats()
    assert st["coalesced_requests"] > 0 and st["requests"] == 8 * len(utts) and st["frames"] == 8 * sum(lens)
    assert ta[1] > tb[1] and ta[1] - tb[1] <= st["batches"] and sa == sb  # one launch of the segmented kernel per batch at most
    assert counts and not [k for k in counts if k.startswith(("gemm.out", "small.out", "ppo.out"))], counts  # no output-layer launch
    srv.close()


def test_a_request_split_over_two_batches(dnn):
    """max_frames = 96, 100-frame utterances: every request is split; the second piece continues at taken * len."""
    sets = the_sets()
    utts = [F.synth_features(100, 432, seed=930 + i) for i in range(4)]
    alone = [dnn.calculateLazySet(x, sets[i]) for i, x in enumerate(utts)]
    srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=200)
    got = [[] for _ in utts]

    def worker(k):
        for _ in range(3):
            t, probs, inactive = srv.submitLazySet(utts[k], sets[k])
            srv.wait(t)
            got[k].append((probs, inactive))

    run_threads(4, worker)
    for k, outs in enumerate(got):
        assert len(outs) == 3
        for probs, inactive in outs:
            assert same_bytes(probs, alone[k][0]) and same_bytes(inactive, alone[k][1]), k
    st = srv.stats()
    assert st["requests"] == 12 and st["frames"] == 1200 and st["batches"] >= 13
    srv.close()


def test_large_coalesced_set_batches(dnn):
    """Batches above the small-batch bound (4 000 frames here) take the loop's shared compute stream."""
    sets = the_sets()
    lens = [1300, 700, 900, 1100]
    utts = [F.synth_features(n, 432, seed=940 + i) for i, n in enumerate(lens)]
    alone = [dnn.calculateLazySet(x, sets[i]) for i, x in enumerate(utts)]
    srv = api.ScoringServer(dnn, max_frames=4000, depth=2, linger_us=2000)
    got = [[] for _ in utts]
    barrier = threading.Barrier(4)

    def worker(k):
        for _ in range(3):
            barrier.wait()
            t, probs, inactive = srv.submitLazySet(utts[k], sets[k])
            srv.wait(t)
            got[k].append((probs, inactive))

    run_threads(4, worker)
    for k, outs in enumerate(got):
        for probs, inactive in outs:
            assert same_bytes(probs, alone[k][0]) and same_bytes(inactive, alone[k][1]), k
    assert srv.stats()["coalesced_requests"] > 0
    srv.close()


def test_a_set_batch_of_two_chunks(tiny_model_path):
    """max_frames one above the chunk: a 20 481-frame request is ONE batch that the loop scores as two chunks on its main
    stream, the cut inside its only segment (the second chunk's block continues at cut * len of the batch's probs, its
    inactive values at cut) -- the bytes of the same rows as two calls."""
    n = 20480 + 1
    assert len(api.frame_chunks(n)) == 2 and len(api.frame_chunks(n - 1)) == 1
    cut = api.frame_chunks(n)[1][0]
    tiny = api.QuantizedDnn.loadFromFile(tiny_model_path)
    nodes = np.arange(3, 100, 3, dtype=np.int32)  # 33 of the tiny net's 100 nodes
    x = F.synth_features(n, 432, seed=950)
    a, b = tiny.calculateLazySet(x[:cut], nodes), tiny.calculateLazySet(x[cut:], nodes)
    srv = api.ScoringServer(tiny, max_frames=n, depth=1)
    t, probs, inactive = srv.submitLazySet(x, nodes)
    srv.wait(t)
    assert same_bytes(probs, np.concatenate([a[0], b[0]])) and same_bytes(inactive, np.concatenate([a[1], b[1]]))
    assert srv.stats()["batches"] == 1
    srv.close()
    tiny.delete()


def test_raw_frames_with_a_set(mid_model_path):
    """submitRawSet on the toy splice spec: the bytes of submitLazySet on host-spliced rows."""
    api.set_kernel(1)
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)
    try:
        offsets = list(range(-5, 6))
        dnn.setSplice(offsets, 39)
        sets = the_sets()
        raws = [np.random.default_rng(950 + i).standard_normal((n, 39)).astype(np.float32) * 3 for i, n in enumerate((70, 100, 31))]

        def spliced(raw):
            return CV.splice_frames(raw, offsets, 432)

        srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=200)
        want = []
        for i, raw in enumerate(raws):
            t, probs, inactive = srv.submitLazySet(spliced(raw), sets[i + 1])
            srv.wait(t)
            want.append((probs, inactive))
        got = [None] * len(raws)

        def worker(k):
            t, probs, inactive = srv.submitRawSet(raws[k], sets[k + 1])
            srv.wait(t)
            got[k] = (probs, inactive)

        run_threads(len(raws), worker)
        for k in range(len(raws)):
            assert same_bytes(got[k][0], want[k][0]) and same_bytes(got[k][1], want[k][1]), k
        srv.close()
    finally:
        dnn.delete()
        api.set_kernel(0)


def test_set_dense_and_bit_mask_submissions_share_one_loop(dnn):
    """Kinds never share a batch; each result equals the direct call's, and closing the loop does not hang."""
    sets = the_sets()
    xs = [F.synth_features(n, 432, seed=960 + i) for i, n in enumerate((100, 50, 130, 77))]
    bits = F.pack_mask_bits(F.generate_masks(130, O, 0.4, 0.03, seed=34))
    want_set = [dnn.calculateLazySet(xs[0], sets[3]), dnn.calculateLazySet(xs[3], sets[0])]
    want_dense = dnn.calculate(xs[1])
    want_bits = dnn.calculateLazy(xs[2], bits=bits)
    srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=2000)
    barrier = threading.Barrier(4)
    bad = []

    def caller(k):
        barrier.wait()
        for _ in range(3):
            if k == 0:
                t, p, i = srv.submitLazySet(xs[0], sets[3])
                srv.wait(t)
                ok = same_bytes(p, want_set[0][0]) and same_bytes(i, want_set[0][1])
            elif k == 1:
                t, out = srv.submit(xs[1])
                srv.wait(t)
                ok = np.array_equal(out, want_dense)
            elif k == 2:
                t, out = srv.submitLazy(xs[2], bits)
                srv.wait(t)
                ok = np.array_equal(out, want_bits)
            else:
                t, p, i = srv.submitLazySet(xs[3], sets[0])  # the empty set: 1 / O per row, no probs
                srv.wait(t)
                ok = p.shape == (77, 0) and same_bytes(i, want_set[1][1]) and (i == np.float32(1.0) / np.float32(O)).all()
            if not ok:
                bad.append(k)

    run_threads(4, caller)
    assert not bad, bad
    assert srv.stats()["requests"] == 12
    srv.close()


def test_set_submission_errors(dnn):
    srv = api.ScoringServer(dnn, max_frames=96, depth=2)
    x = F.synth_features(8, 432, seed=970)
    for wrong in ([2, 1], [1, 1], [-1, 3], [3, O]):
        with pytest.raises(api.FdnnError) as e:
            srv.submitLazySet(x, wrong)
        assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        srv.submitRawSet(np.zeros((8, 39), np.float32), [1, 2])  # no splice spec on this model
    assert e.value.code in (api.FDNN_E_STATE, api.FDNN_E_ARG)
    t, p, i = srv.submitLazySet(x, [1, 2])  # the loop still serves
    srv.wait(t)
    want = dnn.calculateLazySet(x, [1, 2])
    assert same_bytes(p, want[0]) and same_bytes(i, want[1])
    srv.close()
