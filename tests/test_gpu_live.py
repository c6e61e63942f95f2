"""Live utterances through the scoring loop (fdnn_server_live_*): raw frames pushed chunk by chunk, many handles per batch.
Over an utterance's pushes the rows a handle hands back are the bytes of calculateRaw / calculateTopKRaw / calculatePoolRaw
on the whole utterance, and for sets of calculateLazySet on the host-spliced rows -- whatever the chunking and whatever else
shared the batches.  Every comparison is np.array_equal."""
import ctypes as C
import threading

import numpy as np
import pytest

import pool_cases as PC
from fast_dnn_amd import api, convert as CV

pytestmark = pytest.mark.gpu

KALDI = (list(range(-5, 6)), 39)
THREE = ([-2, 0, 3], 144)
IDENTITY = ([0], 432)
LEFT_ONLY = (list(range(-10, 1)), 39)
DUPLICATES = ([2, -1, 2, 0, -1, 5], 64)


def raw_frames(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32) * 3


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def mid(mid_model_path):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path, device=0)
    yield dnn
    dnn.delete()


@pytest.fixture(scope="module")
def tiny(tiny_model_path):
    dnn = api.QuantizedDnn.loadFromFile(tiny_model_path, device=0)
    yield dnn
    dnn.delete()


class Feed:
    """One utterance pushed through a live handle from a buffer of the caller's that is overwritten right after every push;
    checks the position and the row count of every push, keeps (ticket, arrays)."""

    def __init__(self, live, raw, right, push=None):
        self.live, self.raw, self.right = live, raw, right
        self.push_fn = push or live.push
        self.fed = self.rows = 0
        self.parts = []
        self.ring = np.empty((live.maxChunk, raw.shape[1]), dtype=np.float32)

    def push(self, c, end=False):
        self.ring[:c] = self.raw[self.fed:self.fed + c]
        ticket, *arrays = self.push_fn(self.ring[:c], end=end)
        self.ring[:] = -7.0  # the ring buffer moves on: the push has copied its frames
        self.fed += c
        upto = self.fed if end else max(self.rows, self.fed - self.right)
        assert all(len(a) == upto - self.rows for a in arrays), "n_out is the number of rows that arrive"
        assert (ticket is None) == (upto == self.rows), "a push that completes no rows has nothing to wait for"
        self.rows = upto
        assert self.live.position() == (self.fed, self.rows)
        if ticket is not None:
            self.parts.append((ticket, arrays))

    def push_rest(self, chunks):
        """The chunks in order, then a flush-only end."""
        for c in chunks:
            self.push(c)
        self.push(0, end=True)

    def result(self, srv):
        for t, _ in self.parts:
            srv.wait(t)
        return [np.concatenate([a[i] for _, a in self.parts]) for i in range(len(self.parts[0][1]))]


def chunks_of(n, most, rng, least=0):
    out = []
    while n > 0:
        out.append(min(n, int(rng.integers(least, most + 1))))
        n -= out[-1]
    return out


@pytest.mark.parametrize("spec", [KALDI, LEFT_ONLY, IDENTITY, DUPLICATES], ids=["kaldi11", "left_only", "identity", "duplicates"])
def test_one_handle_random_chunks_equal_the_whole_utterance(mid, spec):
    mid.setSplice(*spec)
    right = max(0, max(spec[0]))
    rng = np.random.default_rng(len(spec[0]))
    srv = api.ScoringServer(mid, 512, 2)
    live = srv.openLive(64)
    try:
        raw = raw_frames(300, spec[1], 11)
        want = mid.calculateRaw(raw)
        feed = Feed(live, raw, right)
        feed.push_rest(chunks_of(300, 64, rng))
        assert live.position() == (300, 300)
        assert same(feed.result(srv)[0], want)
        with pytest.raises(api.FdnnError) as e:  # the utterance has ended
            live.push(raw[:3])
        assert e.value.code == api.FDNN_E_STATE and live.position() == (300, 300)
        live.reset()
        assert live.position() == (0, 0)
        raw2 = raw_frames(50, spec[1], 12)
        feed2 = Feed(live, raw2, right)
        feed2.push(50, end=True)  # one push, ended by itself
        assert same(feed2.result(srv)[0], mid.calculateRaw(raw2))
    finally:
        live.close()
        srv.close()


def test_the_wants_equal_their_whole_utterance_entry_points(mid):
    mid.setSplice(*KALDI)
    raw = raw_frames(120, 39, 21)
    pool = api.ClassPool(*PC.map_of("interleaved", mid.outputDimension()))
    nodes = np.array([3, 17, 18, 400, 999], dtype=np.int32)
    srv = api.ScoringServer(mid, 512, 2)
    lives = [srv.openLive(16) for _ in range(3)]
    try:
        feeds = [Feed(lives[0], raw, 5, lambda r, end: lives[0].pushTopK(r, 5, end=end)),
                 Feed(lives[1], raw, 5, lambda r, end: lives[1].pushPool(r, pool, end=end)),
                 Feed(lives[2], raw, 5, lambda r, end: lives[2].pushSet(r, nodes, end=end))]
        for i in range(0, 120, 16):  # 7 x 16 + 8, the last push ends the utterance
            for f in feeds:
                f.push(min(16, 120 - i), end=i + 16 >= 120)
        tk_nodes, tk_probs = feeds[0].result(srv)
        want_nodes, want_probs = mid.calculateTopKRaw(raw, 5)
        assert same(tk_nodes, want_nodes) and same(tk_probs, want_probs)
        assert same(feeds[1].result(srv)[0], mid.calculatePoolRaw(raw, pool))
        probs, inactive = feeds[2].result(srv)
        want_p, want_i = mid.calculateLazySet(CV.splice_frames(raw, KALDI[0], 432), nodes)
        assert same(probs, want_p) and same(inactive, want_i)
    finally:
        for live in lives:
            live.close()
        srv.close()
        pool.delete()


def test_many_handles_share_batches_through_the_table_kernel(tiny):
    """300 handles, utterances of 3 - 12 frames in chunks of 1 - 3.  The first two pushes of every handle queue up under a hold and
    go out as one batch with one segment per push that completed rows; the rest comes from 8 threads.  The spec is
    [-2, 0, 3] x 144 (R = 3): two pushes of 1 - 3 frames complete rows for about two handles in three, where Kaldi's R = 5
    would let almost none through before the release -- and the batch under the hold is what must exceed 96 segments."""
    tiny.setSplice(*THREE)
    rng = np.random.default_rng(300)
    api.scratch_audit(True)
    api.scratch_dirty()
    srv = api.ScoringServer(tiny, 4096, 2, linger_us=300)
    lives = [srv.openLive(3) for _ in range(300)]
    try:
        utts = [raw_frames(int(rng.integers(3, 13)), 144, 1000 + i) for i in range(300)]
        want = [tiny.calculateRaw(u) for u in utts]
        plans = [chunks_of(len(u), 3, rng, least=1) for u in utts]
        feeds = [Feed(live, u, 3) for live, u in zip(lives, utts)]
        before = api.live_launches()
        srv.hold(True)
        for f, plan in zip(feeds, plans):
            for c in plan[:2]:
                f.push(c)
        held = sum(len(f.parts) for f in feeds)
        assert held > 96, "the held batch must have more segments than the by-value kernel takes"
        srv.hold(False)
        errors = []

        def rest(k):
            try:
                for f, plan in list(zip(feeds, plans))[k::8]:
                    f.push_rest(plan[2:])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=rest, args=(k,)) for k in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for f, w in zip(feeds, want):
            assert same(f.result(srv)[0], w)
        after = api.live_launches()
        assert after["max_segs"] > 96 and after["max_segs"] >= held and after["launches"] > before["launches"]
        assert srv.stats()["coalesced_requests"] > 0
    finally:
        for live in lives:
            live.close()
        srv.close()
        dirty = api.scratch_dirty()
        api.scratch_audit(False)
    dirty.pop("seconds")
    assert dirty.pop("contexts") > 0 and not any(dirty.values()), dirty


def test_live_pushes_share_a_batch_with_whole_utterances_of_their_spec(mid):
    mid.setSplice(*KALDI)
    utts = [raw_frames(40, 39, 31 + i) for i in range(4)]
    want = [mid.calculateRaw(u) for u in utts]
    srv = api.ScoringServer(mid, 512, 2)
    lives = [srv.openLive(20) for _ in range(3)]
    try:
        feeds = [Feed(live, u, 5) for live, u in zip(lives, utts)]
        batches = srv.stats()["batches"]
        srv.hold(True)
        feeds[0].push(20)
        ticket, out = srv.submitRaw(utts[3])
        feeds[1].push(20)
        feeds[2].push(20)
        srv.hold(False)
        srv.wait(ticket)
        for f in feeds:
            srv.wait(f.parts[0][0])
        assert srv.stats()["batches"] == batches + 1, "one raw utterance and three live pushes of one spec: one batch"
        assert same(out, want[3])
        for f, w in zip(feeds, want):
            assert same(f.parts[0][1][0], w[:15])
            f.push(20, end=True)
            assert same(f.result(srv)[0], w)
    finally:
        for live in lives:
            live.close()
        srv.close()


def test_a_handle_keeps_the_spec_it_was_opened_with(mid):
    mid.setSplice(*KALDI)
    raw_old, raw_new = raw_frames(30, 39, 41), raw_frames(30, 39, 42)
    want_old = mid.calculateRaw(raw_old)
    srv = api.ScoringServer(mid, 512, 2)
    live = srv.openLive(30)
    try:
        mid.setSplice(*LEFT_ONLY)
        want_new = mid.calculateRaw(raw_new)
        batches = srv.stats()["batches"]
        srv.hold(True)
        feed = Feed(live, raw_old, 5)
        feed.push(30, end=True)
        ticket, out = srv.submitRaw(raw_new)
        srv.hold(False)
        srv.wait(ticket)
        assert same(feed.result(srv)[0], want_old) and same(out, want_new)
        assert srv.stats()["batches"] == batches + 2, "two spec objects never share a batch"
    finally:
        live.close()
        srv.close()


def test_close_and_reset_with_tickets_outstanding(mid):
    mid.setSplice(*KALDI)
    a, b = raw_frames(25, 39, 51), raw_frames(12, 39, 52)
    want_a, want_b = mid.calculateRaw(a), mid.calculateRaw(b)
    srv = api.ScoringServer(mid, 512, 2)
    live = srv.openLive(25)
    try:
        srv.hold(True)
        first = Feed(live, a, 5)
        first.push(25)  # rows 0 .. 19 of a, queued
        live.reset()    # a is abandoned: its queued rows still arrive
        second = Feed(live, b, 5)
        second.push(12, end=True)
        live.close()    # never waits; the tickets stay valid
        srv.hold(False)
        assert same(first.result(srv)[0], want_a[:20])
        assert same(second.result(srv)[0], want_b)
    finally:
        live.close()
        srv.close()


def test_errors(tiny, tiny_model_path):
    L = api.lib()
    bare = api.QuantizedDnn.loadFromFile(tiny_model_path, device=0)  # no spec
    srv0 = api.ScoringServer(bare, 64, 1)
    with pytest.raises(api.FdnnError) as e:
        srv0.openLive(4)
    assert e.value.code == api.FDNN_E_STATE
    srv0.close()
    bare.delete()

    tiny.setSplice(*KALDI)
    O = tiny.outputDimension()
    srv = api.ScoringServer(tiny, 64, 1)
    with pytest.raises(api.FdnnError) as e:
        srv.openLive(0)
    assert e.value.code == api.FDNN_E_ARG
    live = srv.openLive(8)
    raw = raw_frames(9, 39, 61)
    narrow = api.ClassPool(np.zeros(O // 2, dtype=np.int32), 1)
    try:
        live.push(raw[:4])  # no rows yet (R = 5): nothing queued
        assert live.position() == (4, 0)
        for bad in (lambda: live.push(raw),                                   # n_raw > max_chunk
                    lambda: live.pushTopK(raw[:8], 0), lambda: live.pushTopK(raw[:8], O + 1),  # bad k
                    lambda: live.pushPool(raw[:8], narrow),                  # a pool of another width
                    lambda: live.pushSet(raw[:8], [5, 3]), lambda: live.pushSet(raw[:1], [5, 5]),  # a set out of order
                    lambda: live.pushSet(raw[:8], [O])):
            with pytest.raises(api.FdnnError) as e:
                bad()
            assert e.value.code == api.FDNN_E_ARG and live.position() == (4, 0), "a refused push leaves the handle where it was"
        # null buffers, on the C entry points themselves
        n, t = C.c_int(-1), C.c_uint64(9)
        r = raw[:8].ctypes.data_as(C.POINTER(C.c_float))
        buf = np.empty((13, O), dtype=np.float32)
        out = buf.ctypes.data_as(C.POINTER(C.c_float))
        nodes = np.array([1, 2], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        assert L.fdnn_server_live_push(live.handle, r, 8, 0, None, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert (n.value, t.value) == (0, 0)
        assert L.fdnn_server_live_push(live.handle, None, 8, 0, out, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push(live.handle, r, 8, 0, out, None, C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push(live.handle, r, 8, 0, out, C.byref(n), None) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push(None, r, 8, 0, out, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push_topk(live.handle, r, 8, 0, 2, None, out, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push_pool(live.handle, r, 8, 0, None, out, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_push_set(live.handle, r, 8, 0, nodes, 2, out, None, C.byref(n), C.byref(t)) == api.FDNN_E_ARG
        assert L.fdnn_server_live_reset(None) == api.FDNN_E_ARG and L.fdnn_server_live_position(None, None, None) == api.FDNN_E_ARG
        assert live.position() == (4, 0)
        with pytest.raises(api.FdnnError) as e:  # ticket 0 is nobody's
            srv.wait(0)
        assert e.value.code == api.FDNN_E_ARG
        # and the handle still works
        feed = Feed(live, raw, 5)
        feed.fed, feed.rows = 4, 0
        feed.push(5, end=True)
        assert same(feed.result(srv)[0], tiny.calculateRaw(raw))
    finally:
        live.close()
        srv.close()
        narrow.delete()
