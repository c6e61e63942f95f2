"""Raw feature frames spliced on the device (fdnn_splice.hip): whole utterances, streams, the lazy contract, the scoring
loop, device segment tables and groups.  Every result must be BIT-IDENTICAL to the existing entry point on the
host-spliced rows (convert.splice_frames): the spliced rows are copies, so the comparisons are np.array_equal."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, golden
from fast_dnn_amd import api
from fast_dnn_amd import convert as CV
from fast_dnn_amd import formats as F

pytestmark = pytest.mark.gpu

KALDI = (list(range(-5, 6)), 39)
SPECS = [KALDI, ([-2, 0, 3], 144), ([0], 432), (list(range(-10, 1)), 39), ([2, -1, 2, 0, -1, 5], 64)]


def spliced(raw, spec, width=432):
    return CV.splice_frames(raw, spec[0], width)


def raw_frames(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32) * 3


def bits_for(n, O, seed):
    return F.pack_mask_bits(F.generate_masks(n, O, seed=seed))


@pytest.fixture(scope="module")
def mid(mid_model_path):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path, device=0)
    yield dnn
    dnn.delete()


def test_reference_data_through_a_stream(tiny_model_path, tmp_path):
    """The reference's own 16 kHz utterance: 198 raw frames pushed in chunks of 1, 7 and 64 (no end) emit exactly the 193
    shipped rows' scores; the first 100 are the golden oracle's."""
    p = tmp_path / "16khz"
    p.write_bytes(golden("feat_files.npz")["16khz"].tobytes())
    (_, rows), = CV.load_feature_text(str(p))
    raw = np.ascontiguousarray(np.concatenate([rows[:, 195:234], rows[-1, 234:].reshape(5, 39)]))
    dnn = api.QuantizedDnn.loadFromFile(tiny_model_path, device=0)
    want = dnn.calculate(CV.align_features(rows, 4))
    dnn.setSplice(*KALDI)
    for chunk in (1, 7, 64):
        st = dnn.newStream(chunk)
        got = np.concatenate([st.push(raw[i:i + chunk]) for i in range(0, len(raw), chunk)])
        assert st.position() == (198, 193)
        st.close()
        assert got.shape == (193, 100) and np.array_equal(got, want)
    assert np.abs(want[:100] - golden("tiny.npz")["probs"]).max() <= 2e-6
    dnn.delete()


@pytest.mark.parametrize("spec", SPECS, ids=["kaldi11", "three144", "identity", "left_only", "duplicates"])
def test_whole_utterances_mid_net(mid, spec):
    mid.setSplice(*spec)
    for n in (1, 2, 7, 100, 1000, 10000, 20557):
        raw = raw_frames(n, spec[1], seed=n)
        assert np.array_equal(mid.calculateRaw(raw), mid.calculate(spliced(raw, spec))), (spec, n)
    mid.setSplice([], 0)


def test_whole_utterances_full_net(net_model_path):
    """10 000 and 20 557 frames on the 432 -> 7x2048 -> 8000 net: the chunked pass, the chained and role-split kernels."""
    dnn = api.QuantizedDnn.loadFromFile(net_model_path, device=0)
    dnn.setSplice(*KALDI)
    for n in (10000, 20557):
        raw = raw_frames(n, 39, seed=n + 1)
        assert np.array_equal(dnn.calculateRaw(raw), dnn.calculate(spliced(raw, KALDI))), n
    dnn.delete()


def test_stream_equals_whole_utterance(mid):
    mid.setSplice(*KALDI)
    rng = np.random.default_rng(5)
    raw = raw_frames(1000, 39, seed=77)
    want = mid.calculateRaw(raw)
    st = mid.newStream(64)
    got, i = [], 0
    while i < len(raw):
        k = int(rng.integers(0, 65))
        rows = st.push(raw[i:i + k])
        i += min(k, len(raw) - i)
        assert st.position() == (i, max(0, i - 5))
        assert len(rows) <= k + 5
        got.append(rows)
    got.append(st.push(raw[:0], end=True))  # a flush-only push
    assert st.position() == (1000, 1000)
    assert np.array_equal(np.concatenate(got), want)
    with pytest.raises(api.FdnnError) as e:  # the stream has ended
        st.push(raw[:3])
    assert e.value.code == api.FDNN_E_STATE
    # reset: a second utterance with edges of its own, ended by its last push
    st.reset()
    assert st.position() == (0, 0)
    raw2 = raw_frames(300, 39, seed=78)
    parts = [st.push(raw2[j:j + 64], end=j + 64 >= 300) for j in range(0, 300, 64)]
    assert np.array_equal(np.concatenate(parts), mid.calculateRaw(raw2))
    st.close()
    # left context only: every pushed frame is complete at once
    mid.setSplice(*SPECS[3])
    st = mid.newStream(16)
    raw3 = raw_frames(50, 39, seed=79)
    parts = []
    for j in range(0, 50, 16):
        parts.append(st.push(raw3[j:j + 16]))
        assert len(parts[-1]) == len(raw3[j:j + 16])
    assert np.array_equal(np.concatenate(parts), mid.calculateRaw(raw3))
    st.close()
    mid.setSplice([], 0)


def test_stream_keeps_the_spec_it_was_made_with(mid):
    """Changing or clearing the model's spec while a stream is open changes nothing for the stream (a wider D included:
    the stream's buffers hold frames of its own width)."""
    mid.setSplice(*KALDI)
    raw = raw_frames(200, 39, seed=81)
    want = mid.calculateRaw(raw)
    st = mid.newStream(72)
    parts = [st.push(raw[:64])]
    mid.setSplice([0], 432)
    parts.append(st.push(raw[64:128]))
    mid.setSplice([], 0)
    parts.append(st.push(raw[128:], end=True))
    assert np.array_equal(np.concatenate(parts), want)
    with pytest.raises(ValueError):  # frames of another width are refused, not reinterpreted
        st.reset()
        st.push(np.zeros((39, 40), np.float32))
    st.close()
    # a call in progress and a queued server submission keep theirs too: the same spec-change from the caller's thread
    mid.setSplice(*KALDI)
    srv = api.ScoringServer(mid, 256, 1)
    tickets = [srv.submitRaw(raw[:150]) for _ in range(4)]
    mid.setSplice(list(range(-10, 1)), 39)
    for t, out in tickets:
        srv.wait(t)
        assert np.array_equal(out, mid.calculate(spliced(raw[:150], KALDI)))
    srv.close()
    mid.setSplice([], 0)


def test_lazy_on_raw_frames(mid):
    mid.setSplice(*KALDI)
    O = mid.outputDimension()
    n = 700
    raw = raw_frames(n, 39, seed=91)
    x = spliced(raw, KALDI)
    bits = bits_for(n, O, seed=3)
    want = mid.calculateLazy(x, bits=bits)
    assert np.array_equal(mid.calculateLazyRaw(raw, bits), want)
    # LazyContext: calculateUntilOutputRaw == calculateUntilOutput on the spliced rows
    a, b = mid.getNewLazyContext(n), mid.getNewLazyContext(n)
    a.calculateUntilOutputRaw(raw)
    b.calculateUntilOutput(x)
    hid = b.hiddenActivations()
    assert np.array_equal(a.hiddenActivations(), hid)
    assert np.array_equal(a.calculateForOutputNodesBatchBits(bits), b.calculateForOutputNodesBatchBits(bits))
    a.delete()
    b.delete()
    # a stream's hidden-only pushes: the stream's context holds exactly the frames each push completed
    st = mid.newStream(128)
    first = 0
    for j in range(0, n, 128):
        view = st.pushHidden(raw[j:j + 128], end=j + 128 >= n)
        k = view.inputVectorCount
        assert np.array_equal(view.hiddenActivations(), hid[first:first + k])
        assert np.array_equal(view.calculateForOutputNodesBatchBits(bits[first:first + k]), want[first:first + k])
        view.delete()  # (a view: the stream keeps its context)
        first += k
    assert first == n
    st.close()
    mid.setSplice([], 0)


def test_scoring_loop_raw_submissions(mid):
    mid.setSplice(*KALDI)
    O = mid.outputDimension()
    lens = [1, 37, 100, 100, 250, 613, 5000, 80]
    raws = [raw_frames(n, 39, seed=300 + i) for i, n in enumerate(lens)]
    bits = [bits_for(n, O, seed=400 + i) for i, n in enumerate(lens)]
    dense_want = [mid.calculateRaw(r) for r in raws]
    lazy_want = [mid.calculateLazyRaw(r, b) for r, b in zip(raws, bits)]
    srv = api.ScoringServer(mid, 4096, 2, linger_us=2000)
    got = [[None, None] for _ in lens]
    barrier = threading.Barrier(len(lens))

    def caller(i):
        barrier.wait()
        for rep in range(3):
            t, out = srv.submitRaw(raws[i])
            srv.wait(t)
            got[i][0] = out
            t, out = srv.submitRaw(raws[i], bits=bits[i])
            srv.wait(t)
            got[i][1] = out

    threads = [threading.Thread(target=caller, args=(i,)) for i in range(len(lens))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for i in range(len(lens)):
        assert np.array_equal(got[i][0], dense_want[i]), i
        assert np.array_equal(got[i][1], lazy_want[i]), i
    st = srv.stats()
    assert st["coalesced_requests"] > 0 and st["requests"] == 2 * 3 * len(lens)
    srv.close()
    mid.setSplice([], 0)


def test_device_segment_table(mid):
    import torch

    mid.setSplice(*KALDI)
    lens = [3, 700, 1, 2400, 96]
    raws = [raw_frames(n, 39, seed=500 + i) for i, n in enumerate(lens)]
    want = np.concatenate([mid.calculateRaw(r) for r in raws])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    d_raw = torch.from_numpy(np.concatenate(raws)).cuda()
    d_out = torch.empty((sum(lens), mid.outputDimension()), dtype=torch.float32, device="cuda")
    mid.calculateRawDevice(d_raw.data_ptr(), sum(lens), d_out.data_ptr(), segStarts=starts, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want)
    # one utterance (no table) == the host call
    mid.calculateRawDevice(d_raw.data_ptr(), sum(lens), d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), mid.calculateRaw(np.concatenate(raws)))
    # more segments than one launch carries (96): the table goes as several launches
    rng = np.random.default_rng(9)
    lens2 = [int(v) for v in rng.integers(1, 6, size=230)]
    raws2 = [raw_frames(n, 39, seed=2000 + i) for i, n in enumerate(lens2)]
    want2 = np.concatenate([mid.calculate(spliced(r, KALDI)) for r in raws2])
    starts2 = np.concatenate([[0], np.cumsum(lens2)[:-1]]).tolist()
    d_raw2 = torch.from_numpy(np.concatenate(raws2)).cuda()
    d_out2 = torch.empty((sum(lens2), mid.outputDimension()), dtype=torch.float32, device="cuda")
    mid.calculateRawDevice(d_raw2.data_ptr(), sum(lens2), d_out2.data_ptr(), segStarts=starts2, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out2.cpu().numpy(), want2)
    # ... and as a server batch of many short utterances (one segment each)
    srv = api.ScoringServer(mid, 4096, 1, linger_us=20000)
    tickets = [srv.submitRaw(r) for r in raws2]
    for (t, out), r in zip(tickets, raws2):
        srv.wait(t)
        assert np.array_equal(out, mid.calculate(spliced(r, KALDI)))
    assert srv.stats()["batches"] < len(raws2)
    srv.close()
    with pytest.raises(api.FdnnError) as e:
        mid.calculateRawDevice(d_raw.data_ptr(), sum(lens), d_out.data_ptr(), segStarts=[0, 5, 5])
    assert e.value.code == api.FDNN_E_ARG
    mid.setSplice([], 0)


def test_device_raw_frames_in_two_chunks(tiny_model_path):
    """fdnn_calculate_raw_device at the smallest n that api.frame_chunks cuts in two, on the tiny net: the second chunk's rows
    are spliced from row `cut` on and land at d_out + cut * O -- the bytes of the same rows scored as two calls."""
    import torch

    n = 20480 + 1
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2 and len(api.frame_chunks(n - 1, chained)) == 1
    cut = api.frame_chunks(n, True)[1][0]
    tiny = api.QuantizedDnn.loadFromFile(tiny_model_path, device=0)
    tiny.setSplice(*KALDI)
    raw = raw_frames(n, 39, seed=600)
    rows = spliced(raw, KALDI)
    want = np.concatenate([tiny.calculate(rows[:cut]), tiny.calculate(rows[cut:])])
    d_raw = torch.from_numpy(raw).cuda()
    d_out = torch.full((n * tiny.outputDimension() + 4,), -7.0, dtype=torch.float32, device="cuda")
    tiny.calculateRawDevice(d_raw.data_ptr(), n, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n * tiny.outputDimension():] == -7.0).all()
    assert np.array_equal(got[:n * tiny.outputDimension()].reshape(n, -1).view(np.uint32), want.view(np.uint32))
    tiny.delete()


def test_group_and_batcher(mid, mid_model_path, monkeypatch, tmp_path):
    monkeypatch.setenv("FDNN_GROUP_SPLIT_MIN", "64")
    monkeypatch.setenv("FDNN_GROUP_SHARD_MIN", "16")
    mid.setSplice(*KALDI)
    raw = raw_frames(1001, 39, seed=600)
    want = mid.calculateRaw(raw)
    for before_attach in (True, False):  # the spec reaches every replica whether it was set before or after attaching
        grp = api.DeviceGroup(mid_model_path, [0, 0])
        lead = grp.model(0)
        if before_attach:
            lead.setSplice(*KALDI)
        api._check(api.lib().fdnn_group_attach(grp.handle))
        if not before_attach:
            lead.setSplice(*KALDI)
        assert grp.model(1).spliceSpec() == (KALDI[0], 39)
        assert np.array_equal(lead.calculateRaw(raw), want)  # sharded: each replica its shard + halo
        assert np.array_equal(lead.calculateRaw(raw[:40]), mid.calculateRaw(raw[:40]))  # small: whole on one replica
        grp.delete()
    # the batcher (FDNN_BATCHER at load) routes calculateRaw through the scoring loop: same bits
    # the batcher (FDNN_BATCHER at load) routes calculateRaw through the scoring loop: same bits -- on a plain model, and on
    # a group (FDNN_DEVICES) as fdnn_calculate routes: sharded first, each shard through its replica's loop
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
from fast_dnn_amd import api
raw = np.load({str(tmp_path / 'raw.npy')!r})
for name, dev in (("plain", 0), ("group", None)):
    dnn = api.QuantizedDnn.loadFromFile({mid_model_path!r}, device=dev)
    dnn.setSplice(list(range(-5, 6)), 39)
    np.save({str(tmp_path)!r} + "/got_" + name + ".npy", dnn.calculateRaw(raw))
    dnn.delete()
"""
    np.save(str(tmp_path / "raw.npy"), raw)
    env = dict(os.environ, FDNN_BATCHER="512:2", FDNN_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("plain", "group"):
        assert np.array_equal(np.load(str(tmp_path / f"got_{name}.npy")), want), name
    mid.setSplice([], 0)


def test_contract(mid):
    import torch

    mid.setSplice([], 0)
    raw = raw_frames(20, 39, seed=700)
    O = mid.outputDimension()
    bits = bits_for(20, O, seed=1)
    x = spliced(raw, KALDI)
    before = mid.calculate(x)

    def code_of(fn):
        with pytest.raises(api.FdnnError) as e:
            fn()
        return e.value.code

    # no spec: FDNN_E_STATE from every raw entry point
    assert mid.spliceSpec() is None
    assert code_of(lambda: mid.calculateRaw(raw)) == api.FDNN_E_STATE
    assert code_of(lambda: mid.calculateLazyRaw(raw, bits)) == api.FDNN_E_STATE
    assert code_of(lambda: mid.calculateRawDevice(0, 20, 0)) == api.FDNN_E_STATE
    assert code_of(lambda: mid.newStream(8)) == api.FDNN_E_STATE
    ctx = mid.getNewLazyContext(20)
    assert code_of(lambda: ctx.calculateUntilOutputRaw(raw)) == api.FDNN_E_STATE
    ctx.delete()
    srv = api.ScoringServer(mid, 256, 1)
    assert code_of(lambda: srv.submitRaw(raw)) == api.FDNN_E_STATE
    srv.close()
    # bad specs: C * D > input_dim, |o| > 64, C = 0, C > 64
    for offs, d in ((list(range(-5, 6)), 40), ([65], 4), ([-65], 4), ([], 39), ([0] * 65, 4)):
        assert code_of(lambda: mid.setSplice(offs, d)) == api.FDNN_E_ARG, (offs, d)
    assert mid.spliceSpec() is None
    mid.setSplice([64, -64] + [0] * 62, 6)  # the edges of the rule are accepted
    assert mid.spliceSpec() == ([64, -64] + [0] * 62, 6)
    # a wrong raw width
    mid.setSplice(*KALDI)
    assert code_of(lambda: mid.calculateRaw(raw_frames(20, 40, seed=1))) == api.FDNN_E_ARG
    assert code_of(lambda: mid.calculateLazyRaw(raw_frames(20, 38, seed=1), bits)) == api.FDNN_E_ARG
    # n = 0 is a no-op
    assert mid.calculateRaw(raw[:0]).shape == (0, O)
    mid.calculateRawDevice(0, 0, 0)
    # a spec changes no existing entry point
    assert np.array_equal(mid.calculate(x), before)
    assert np.array_equal(mid.calculateRaw(raw), before)
    d = torch.from_numpy(x).cuda()
    o = torch.empty((20, O), dtype=torch.float32, device="cuda")
    mid.calculate_device(d.data_ptr(), 20, o.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), before)
    mid.setSplice([], 0)
