"""Pool submissions through the scoring loop (fdnn_server_submit_pool / fdnn_server_submit_raw_pool): eight callers'
utterances of 7 to 130 frames under TWO different class maps in flight at once, coalesced into dense batches whose rows never
leave the device -- requests of one handle share a batch, requests of different handles never do; one pooling launch, one
transfer, each caller its rows.  Every result's bytes are fdnn_calculate_pool's on that utterance alone, requests split by
max_frames included, and the dense, bit-mask and top-k submissions interleaved with them get what they get today."""
import threading

import numpy as np
import pytest

import pool_cases as PC
from fast_dnn_amd import api, convert as CV, formats as F

pytestmark = pytest.mark.gpu
O = 1000


@pytest.fixture(scope="module")
def dnn(mid_model_path):
    d = api.QuantizedDnn.loadFromFile(mid_model_path)
    yield d
    d.delete()


@pytest.fixture(scope="module")
def pools():
    ps = [api.ClassPool(*PC.map_of("interleaved", O)), api.ClassPool(*PC.map_of("sizes", O))]
    assert ps[0].classes() != ps[1].classes()
    yield ps
    for p in ps:
        p.delete()


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


def test_pool_submissions_are_coalesced_split_and_byte_equal(dnn, pools):
    lens = [7, 130, 100, 64, 33, 97, 128, 20, 111, 75]  # (max_frames = 96 splits the long ones)
    which = [i % 2 for i in range(len(lens))]
    utts = [F.synth_features(n, 432, seed=1700 + i) for i, n in enumerate(lens)]
    alone = [dnn.calculatePool(x, pools[which[i]]) for i, x in enumerate(utts)]
    assert all(PC.same_bytes(alone[i], api.pool_ref(dnn.calculate(utts[i]), pools[which[i]].class_of, pools[which[i]].classes())) for i in (0, 1))
    dense_x = F.synth_features(50, 432, seed=1750)
    want_dense = dnn.calculate(dense_x)
    bits = F.pack_mask_bits(F.generate_masks(40, O, 0.4, 0.03, seed=36))
    lazy_x = F.synth_features(40, 432, seed=1751)
    want_lazy = dnn.calculateLazy(lazy_x, bits=bits)
    want_topk = dnn.calculateTopK(dense_x, 32)
    srv = api.ScoringServer(dnn, max_frames=96, depth=3, linger_us=300)
    results, lock, bad = [], threading.Lock(), []
    before = api.pool_launches()

    def worker(w):
        for j in range(len(utts)):
            i = (j + w) % len(utts)
            out = np.full((lens[i], pools[which[i]].classes()), -7.0, dtype=np.float32)
            t, _ = srv.submitPool(utts[i], pools[which[i]], out)
            if j % 4 == w % 4:  # dense, lazy-bits and top-k submissions in between
                if w % 3 == 0:
                    t2, o2 = srv.submit(dense_x)
                    srv.wait(t2)
                    ok = np.array_equal(o2.view(np.uint32), want_dense.view(np.uint32))
                elif w % 3 == 1:
                    t2, o2 = srv.submitLazy(lazy_x, bits)
                    srv.wait(t2)
                    ok = np.array_equal(o2.view(np.uint32), want_lazy.view(np.uint32))
                else:
                    t2, nd, pr = srv.submitTopK(dense_x, 32)
                    srv.wait(t2)
                    ok = np.array_equal(nd, want_topk[0]) and np.array_equal(pr.view(np.uint32), want_topk[1].view(np.uint32))
                if not ok:
                    bad.append((w, j))
            srv.wait(t)
            with lock:
                results.append((i, out))

    run_threads(8, worker)
    after = api.pool_launches()
    assert not bad, bad
    assert len(results) == 8 * len(utts)
    for i, out in results:
        assert PC.same_bytes(out, alone[i]), i
    st = srv.stats()
    extra = st["requests"] - 8 * len(utts)
    assert extra > 0 and st["coalesced_requests"] > 0 and st["frames"] >= 8 * sum(lens)
    launches = (after[0] - before[0]) + (after[1] - before[1])
    assert 0 < launches <= st["batches"]  # one pooling launch per pool batch
    assert st["batches"] > 8 * sum(lens) // 96  # (max_frames = 96 splits requests)
    srv.close()


def test_a_split_request_continues_at_taken_times_c(dnn, pools):
    """max_frames = 48, one caller, 130 frames: three pieces of one request."""
    x = F.synth_features(130, 432, seed=1760)
    want = dnn.calculatePool(x, pools[0])
    srv = api.ScoringServer(dnn, max_frames=48, depth=2)
    t, out = srv.submitPool(x, pools[0])
    srv.wait(t)
    assert PC.same_bytes(out, want)
    assert srv.stats()["batches"] == 3
    srv.close()


def test_requests_of_two_handles_never_share_a_batch(dnn, pools):
    """Two requests queued together under different maps: two batches, one pooling launch each."""
    x = F.synth_features(20, 432, seed=1761)
    same_map = api.ClassPool(pools[0].class_of, pools[0].classes())  # an equal map behind ANOTHER handle does not join either
    srv = api.ScoringServer(dnn, max_frames=512, depth=2, linger_us=300)
    before = api.pool_launches()
    subs = [srv.submitPool(x, p) for p in (pools[0], pools[1], same_map)]
    for t, _ in subs:
        srv.wait(t)
    after = api.pool_launches()
    for (t, out), p in zip(subs, (pools[0], pools[1], same_map)):
        assert PC.same_bytes(out, dnn.calculatePool(x, p))
    assert srv.stats()["batches"] == 3 and sum(after) - sum(before) == 3  # (`after` was read before the per-call forms ran)
    srv.close()
    same_map.delete()


def test_raw_pool_submissions(mid_model_path, pools):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)
    try:
        offsets = list(range(-5, 6))
        dnn.setSplice(offsets, 39)
        raws = [(np.random.default_rng(1770 + i).standard_normal((n, 39)) * 3).astype(np.float32) for i, n in enumerate((70, 130, 31, 7))]
        want = [dnn.calculatePoolRaw(r, pools[i % 2]) for i, r in enumerate(raws)]
        assert PC.same_bytes(want[0], dnn.calculatePool(CV.splice_frames(raws[0], offsets, 432), pools[0]))
        srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=300)
        got = [[] for _ in raws]

        def worker(w):
            for j in range(len(raws)):
                i = (j + w) % len(raws)
                t, out = srv.submitRawPool(raws[i], pools[i % 2])
                srv.wait(t)
                got[i].append(out)

        run_threads(8, worker)
        for i, outs in enumerate(got):
            assert len(outs) == 8
            for res in outs:
                assert PC.same_bytes(res, want[i]), i
        assert srv.stats()["coalesced_requests"] > 0
        srv.close()
    finally:
        dnn.delete()


def test_pool_submission_errors(dnn, pools):
    srv = api.ScoringServer(dnn, max_frames=96, depth=2)
    x = F.synth_features(8, 432, seed=1780)
    narrow = api.ClassPool(np.zeros(O - 1, np.int32), 1)
    with pytest.raises(api.FdnnError) as e:
        srv.submitPool(x, narrow)  # width mismatch
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        srv.submitRawPool(np.zeros((8, 39), np.float32), pools[0])  # no splice spec on this model
    assert e.value.code in (api.FDNN_E_STATE, api.FDNN_E_ARG)
    t, out = srv.submitPool(x, pools[0])  # the loop still serves
    srv.wait(t)
    assert PC.same_bytes(out, dnn.calculatePool(x, pools[0]))
    srv.close()
    narrow.delete()
