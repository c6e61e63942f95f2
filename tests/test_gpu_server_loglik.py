"""Loglik submissions through the scoring loop (fdnn_server_submit_loglik / _raw_loglik, fdnn_server_live_push_loglik): eight
callers' utterances of 7 to 130 frames under an fp32 AND an fp16 score handle in flight at once, coalesced into dense batches
whose rows never leave the device -- requests of one handle share a batch, requests of different handles never do; one score
launch, one transfer of [rows][O] scores (half the dense batch's bytes for fp16), each caller its rows.  Every result's bytes
are fdnn_calculate_loglik's on that utterance alone, requests split by max_frames included, and the dense, top-k and pool
submissions interleaved with them get what they get today."""
import threading

import numpy as np
import pytest

import loglik_cases as LL
import pool_cases as PC
from fast_dnn_amd import api, convert as CV, formats as F

pytestmark = pytest.mark.gpu
O = 1000
KALDI = (list(range(-5, 6)), 39)


@pytest.fixture(scope="module")
def dnn(mid_model_path):
    d = api.QuantizedDnn.loadFromFile(mid_model_path)
    yield d
    d.delete()


@pytest.fixture(scope="module")
def handles():
    lp = LL.priors(O)
    hs = [api.Loglik(lp, -np.inf, api.LOGLIK_F32), api.Loglik(lp, -20.0, api.LOGLIK_F16)]
    yield hs
    for h in hs:
        h.delete()


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


def test_loglik_submissions_are_coalesced_split_and_byte_equal(dnn, handles):
    lens = [7, 130, 100, 64, 33, 97, 128, 20, 111, 75]  # (max_frames = 96 splits the long ones)
    which = [i % 2 for i in range(len(lens))]
    utts = [F.synth_features(n, 432, seed=2000 + i) for i, n in enumerate(lens)]
    alone = [dnn.calculateLoglik(x, handles[which[i]]) for i, x in enumerate(utts)]
    for i in (0, 1):
        h = handles[which[i]]
        assert LL.same_bytes(alone[i], api.loglik_ref(dnn.calculate(utts[i]), h.log_prior, h.floor, h.type()))
    dense_x = F.synth_features(50, 432, seed=2050)
    want_dense = dnn.calculate(dense_x)
    want_topk = dnn.calculateTopK(dense_x, 32)
    pool = api.ClassPool(*PC.map_of("interleaved", O))
    want_pool = dnn.calculatePool(dense_x, pool)
    srv = api.ScoringServer(dnn, max_frames=96, depth=3, linger_us=300)
    results, lock, bad = [], threading.Lock(), []
    before = api.loglik_launches()

    def worker(w):
        for j in range(len(utts)):
            i = (j + w) % len(utts)
            h = handles[which[i]]
            out = np.full((lens[i], O), -7.0, dtype=h.dtype)
            t, _ = srv.submitLoglik(utts[i], h, out)
            if j % 4 == w % 4:  # dense, top-k and pool submissions in between
                if w % 3 == 0:
                    t2, o2 = srv.submit(dense_x)
                    srv.wait(t2)
                    ok = np.array_equal(o2.view(np.uint32), want_dense.view(np.uint32))
                elif w % 3 == 1:
                    t2, nd, pr = srv.submitTopK(dense_x, 32)
                    srv.wait(t2)
                    ok = np.array_equal(nd, want_topk[0]) and np.array_equal(pr.view(np.uint32), want_topk[1].view(np.uint32))
                else:
                    t2, o2 = srv.submitPool(dense_x, pool)
                    srv.wait(t2)
                    ok = PC.same_bytes(o2, want_pool)
                if not ok:
                    bad.append((w, j))
            srv.wait(t)
            with lock:
                results.append((i, out))

    run_threads(8, worker)
    after = api.loglik_launches()
    assert not bad, bad
    assert len(results) == 8 * len(utts)
    for i, out in results:
        assert LL.same_bytes(out, alone[i]), i
    st = srv.stats()
    extra = st["requests"] - 8 * len(utts)
    assert extra > 0 and st["coalesced_requests"] > 0 and st["frames"] >= 8 * sum(lens)
    launches = sum(after[:2]) - sum(before[:2])
    assert 0 < launches <= st["batches"] and after[2] == before[2]  # one score launch per loglik batch
    assert st["batches"] > 8 * sum(lens) // 96  # (max_frames = 96 splits requests)
    srv.close()
    pool.delete()


@pytest.mark.parametrize("which", [0, 1])
def test_a_split_request_continues_at_taken_times_o(dnn, handles, which):
    """max_frames = 48, one caller, 130 frames: three pieces of one request, each at its byte offset of the caller's array."""
    x = F.synth_features(130, 432, seed=2060)
    want = dnn.calculateLoglik(x, handles[which])
    srv = api.ScoringServer(dnn, max_frames=48, depth=2)
    t, out = srv.submitLoglik(x, handles[which])
    srv.wait(t)
    assert out.dtype == handles[which].dtype and LL.same_bytes(out, want)
    assert srv.stats()["batches"] == 3
    srv.close()


def test_an_f32_and_an_f16_handle_never_share_a_batch(dnn, handles):
    """Three requests queued together under an fp32 handle, an fp16 handle and an equal fp16 handle behind ANOTHER address:
    three batches, one score launch each."""
    x = F.synth_features(20, 432, seed=2061)
    twin = api.Loglik(handles[1].log_prior, handles[1].floor, api.LOGLIK_F16)
    srv = api.ScoringServer(dnn, max_frames=512, depth=2, linger_us=300)
    before = api.loglik_launches()
    hs = (handles[0], handles[1], twin)
    subs = [srv.submitLoglik(x, h) for h in hs]
    for t, _ in subs:
        srv.wait(t)
    after = api.loglik_launches()
    for (t, out), h in zip(subs, hs):
        assert LL.same_bytes(out, dnn.calculateLoglik(x, h))
    assert LL.same_bytes(subs[1][1], subs[2][1])
    assert srv.stats()["batches"] == 3 and sum(after) - sum(before) == 3  # (`after` was read before the per-call forms ran)
    srv.close()
    twin.delete()


def test_raw_submissions_and_a_live_push(mid_model_path, handles):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)
    try:
        dnn.setSplice(*KALDI)
        raws = [(np.random.default_rng(2070 + i).standard_normal((n, 39)) * 3).astype(np.float32) for i, n in enumerate((70, 130, 31, 7))]
        want = [dnn.calculateLoglikRaw(r, handles[i % 2]) for i, r in enumerate(raws)]
        assert LL.same_bytes(want[0], dnn.calculateLoglik(CV.splice_frames(raws[0], KALDI[0], 432), handles[0]))
        srv = api.ScoringServer(dnn, max_frames=96, depth=2, linger_us=300)
        got = [[] for _ in raws]

        def worker(w):
            for j in range(len(raws)):
                i = (j + w) % len(raws)
                t, out = srv.submitRawLoglik(raws[i], handles[i % 2])
                srv.wait(t)
                got[i].append(out)

        run_threads(8, worker)
        for i, outs in enumerate(got):
            assert len(outs) == 8
            for res in outs:
                assert LL.same_bytes(res, want[i]), i
        assert srv.stats()["coalesced_requests"] > 0
        # a live utterance pushed chunk by chunk equals the stream push of the same chunks (and the whole utterance)
        raw, h = raws[1], handles[1]
        live = srv.openLive(16)
        stream = dnn.newStream(16)
        pieces, from_stream = [], []
        for i in range(0, len(raw), 16):
            end = i + 16 >= len(raw)
            t, out = live.pushLoglik(raw[i:i + 16], h, end=end)
            if t is not None:
                srv.wait(t)
            pieces.append(out.copy())
            ctx = stream.pushHidden(raw[i:i + 16], end=end)
            from_stream.append(ctx.calculateOutputLoglik(h) if ctx.inputVectorCount else np.empty((0, O), h.dtype))
        live.close()
        stream.close()
        assert [p.shape for p in pieces] == [s.shape for s in from_stream]
        for p, s in zip(pieces, from_stream):
            assert LL.same_bytes(p, s)
        assert LL.same_bytes(np.concatenate(pieces), want[1])
        srv.close()
    finally:
        dnn.delete()


def test_loglik_submission_errors(dnn, handles):
    srv = api.ScoringServer(dnn, max_frames=96, depth=2)
    x = F.synth_features(8, 432, seed=2080)
    narrow = api.Loglik(np.zeros(O - 1, np.float32))
    with pytest.raises(api.FdnnError) as e:
        srv.submitLoglik(x, narrow)  # width mismatch
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        srv.submitRawLoglik(np.zeros((8, 39), np.float32), handles[0])  # no splice spec on this model
    assert e.value.code in (api.FDNN_E_STATE, api.FDNN_E_ARG)
    with pytest.raises(ValueError):
        srv.submitLoglik(x, handles[1], np.empty((8, O), np.float32))  # an fp32 array for an fp16 handle
    t, out = srv.submitLoglik(x, handles[1])  # the loop still serves
    srv.wait(t)
    assert LL.same_bytes(out, dnn.calculateLoglik(x, handles[1]))
    srv.close()
    narrow.delete()
