"""Top-k submissions through the scoring loop (fdnn_server_submit_topk / fdnn_server_submit_raw_topk): eight callers'
utterances of 7 to 130 frames, each with its own k, coalesced into dense batches whose rows never leave the device -- one
selection launch with the batch's largest k, one transfer, each caller the first k columns of its rows.  Every result's bytes
are fdnn_calculate_topk's on that utterance alone, requests split by max_frames included, and the dense and bit-mask
submissions interleaved with them get what they get today."""
import threading

import numpy as np
import pytest

from fast_dnn_amd import api, convert as CV, formats as F

pytestmark = pytest.mark.gpu
O = 1000
KS = (1, 5, 32, 256)


@pytest.fixture(scope="module")
def dnn(mid_model_path):
    d = api.QuantizedDnn.loadFromFile(mid_model_path)
    yield d
    d.delete()


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))


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


def test_topk_submissions_are_coalesced_split_and_byte_equal(dnn):
    rng = np.random.default_rng(41)
    lens = [7, 130, 100, 64, 33, 97, 128, 20, 111, 75]
    ks = [KS[int(rng.integers(0, 4))] for _ in lens]
    ks[1], ks[2] = 256, 1  # (the longest utterance with the largest k: max_frames = 96 splits it)
    utts = [F.synth_features(n, 432, seed=1400 + i) for i, n in enumerate(lens)]
    alone = [dnn.calculateTopK(x, ks[i]) for i, x in enumerate(utts)]
    dense_x = F.synth_features(50, 432, seed=1450)
    want_dense = dnn.calculate(dense_x)
    bits = F.pack_mask_bits(F.generate_masks(40, O, 0.4, 0.03, seed=35))
    lazy_x = F.synth_features(40, 432, seed=1451)
    want_lazy = dnn.calculateLazy(lazy_x, bits=bits)
    srv = api.ScoringServer(dnn, max_frames=96, depth=3, linger_us=300)
    results, lock, bad = [], threading.Lock(), []
    before = api.topk_launches()

    def worker(w):
        for j in range(len(utts)):
            i = (j + w) % len(utts)
            nodes = np.full((lens[i], ks[i]), -7, dtype=np.int32)
            probs = np.full((lens[i], ks[i]), -7.0, dtype=np.float32)
            t, _, _ = srv.submitTopK(utts[i], ks[i], nodes, probs)
            if j % 4 == w % 4:  # a few dense and lazy-bits submissions in between
                if w % 2:
                    t2, out = srv.submit(dense_x)
                    srv.wait(t2)
                    if not np.array_equal(out.view(np.uint32), want_dense.view(np.uint32)):
                        bad.append(("dense", w, j))
                else:
                    t2, out = srv.submitLazy(lazy_x, bits)
                    srv.wait(t2)
                    if not np.array_equal(out.view(np.uint32), want_lazy.view(np.uint32)):
                        bad.append(("lazy", w, j))
            srv.wait(t)
            with lock:
                results.append((i, nodes, probs))

    run_threads(8, worker)
    after = api.topk_launches()
    assert not bad, bad
    assert len(results) == 8 * len(utts)
    for i, nodes, probs in results:
        assert same((nodes, probs), alone[i]), (i, ks[i])
    st = srv.stats()
    extra = st["requests"] - 8 * len(utts)
    assert extra > 0 and st["coalesced_requests"] > 0 and st["frames"] >= 8 * sum(lens)
    launches = (after[0] - before[0]) + (after[1] - before[1])
    assert 0 < launches <= st["batches"]  # one selection launch per top-k batch
    assert st["batches"] > 8 * sum(lens) // 96  # (max_frames = 96 splits requests)
    srv.close()


def test_a_split_request_continues_at_taken_times_k(dnn):
    """max_frames = 48, one caller, 130 frames, k = 256: three pieces of one request."""
    x = F.synth_features(130, 432, seed=1460)
    want = dnn.calculateTopK(x, 256)
    srv = api.ScoringServer(dnn, max_frames=48, depth=2)
    t, nodes, probs = srv.submitTopK(x, 256)
    srv.wait(t)
    assert same((nodes, probs), want)
    assert srv.stats()["batches"] == 3
    srv.close()


def test_a_batch_of_two_chunks(tiny_model_path):
    """max_frames one above the chunk: a 20 481-frame request is ONE batch that the loop scores as two chunks on its main
    stream, with one selection launch over all rows behind them -- the bytes of the same rows as two calls."""
    n, k = 20480 + 1, 32
    assert len(api.frame_chunks(n)) == 2 and len(api.frame_chunks(n - 1)) == 1
    cut = api.frame_chunks(n)[1][0]
    tiny = api.QuantizedDnn.loadFromFile(tiny_model_path)
    x = F.synth_features(n, 432, seed=1470)
    a, b = tiny.calculateTopK(x[:cut], k), tiny.calculateTopK(x[cut:], k)
    srv = api.ScoringServer(tiny, max_frames=n, depth=1)
    t, nodes, probs = srv.submitTopK(x, k)
    srv.wait(t)
    assert same((nodes, probs), (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])))
    assert srv.stats()["batches"] == 1
    srv.close()
    tiny.delete()


def test_raw_topk_submissions(mid_model_path):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)
    try:
        offsets = list(range(-5, 6))
        dnn.setSplice(offsets, 39)
        raws = [(np.random.default_rng(1470 + i).standard_normal((n, 39)) * 3).astype(np.float32) for i, n in enumerate((70, 130, 31, 7))]
        ks = (32, 5, 256, 1)
        want = [dnn.calculateTopKRaw(r, ks[i]) for i, r in enumerate(raws)]
        assert same(want[0], dnn.calculateTopK(CV.splice_frames(raws[0], offsets, 432), ks[0]))
        srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=300)
        got = [[] for _ in raws]

        def worker(w):
            for j in range(len(raws)):
                i = (j + w) % len(raws)
                t, nodes, probs = srv.submitRawTopK(raws[i], ks[i])
                srv.wait(t)
                got[i].append((nodes, probs))

        run_threads(8, worker)
        for i, outs in enumerate(got):
            assert len(outs) == 8
            for res in outs:
                assert same(res, want[i]), i
        assert srv.stats()["coalesced_requests"] > 0
        srv.close()
    finally:
        dnn.delete()


def test_topk_submission_errors(dnn):
    srv = api.ScoringServer(dnn, max_frames=96, depth=2)
    x = F.synth_features(8, 432, seed=1480)
    for k in (0, 257, O + 1):
        with pytest.raises(api.FdnnError) as e:
            srv.submitTopK(x, k)
        assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        srv.submitRawTopK(np.zeros((8, 39), np.float32), 5)  # no splice spec on this model
    assert e.value.code in (api.FDNN_E_STATE, api.FDNN_E_ARG)
    t, nodes, probs = srv.submitTopK(x, 5)  # the loop still serves
    srv.wait(t)
    assert same((nodes, probs), dnn.calculateTopK(x, 5))
    srv.close()
