"""
Stream records and held streams (include/pv_koala_batch.h: pv_koala_batch_export_state / import_state / process_chunk_hold) on a real
MI355X: the two kernels of koala_amd/csrc/kns_state.hip under every route of the dispatch table.  fp32 comparisons are ==; bf16
against the oracle within the suite's bar, bf16 between two runs of the same handle shape and call sequence ==.

The oracle's work is kept small (about 20 000 stream-frames in this file).  Streams are independent, so the large batches are filled
with copies of a few CLASSES of stream -- a class is a signal and, for the hold tests, a pattern of held calls -- scattered over the
slots at random: the oracle runs once per class and EVERY stream is compared with its class.
"""
import subprocess
import sys

import numpy as np
import pytest

import koala_amd
from conftest import ROOT, synth_streams
from koala_amd._errors import KoalaInvalidArgumentError, PicovoiceStatuses
from gpu_kit import (BF16_TOL, DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_SMALL, ROUTE_WAVE, batch, call, frames, lsb,
                     oracle_prec, route_of, tol)
from oracle import oracle
from stream_state_recipe import record_size, unpack_record

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. what a record holds

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_record_content(random_model, random5_model, precision):
    B, T = 40, 4
    hashes = []
    for model, taps in ((random_model, 1), (random5_model, 5)):
        kb = batch(model, B, T, precision)
        assert kb.state_size == record_size(taps) == 10240 + (taps - 1) * 257 * 4
        fresh = kb.export_state()
        assert fresh.shape == (B, kb.state_size) and fresh.dtype == np.uint8
        assert all(np.array_equal(fresh[b], fresh[0]) for b in range(B))
        f0 = unpack_record(fresh[0])
        assert f0['front_taps'] == taps and f0['precision'] == (1 if precision == 'bf16' else 0)
        assert not f0['hist'].any() and not f0['tail'].any() and not f0['h'].any()
        x = synth_streams(B, 3 * T, seed=11)
        for c in range(2):
            kb.process(frames(x, c * T, (c + 1) * T))
        kb.process(frames(x, 2 * T, 2 * T + 1))  # (a one-frame call: the in-place history, the graph's parity)
        hidden = kb.debug_read('hidden', 1)
        recs = kb.export_state()
        some = kb.export_state([7, 39, 0])
        assert np.array_equal(some, recs[[7, 39, 0]])
        for b in range(B):
            r = unpack_record(recs[b])
            assert r['model_hash'] == f0['model_hash']
            assert np.array_equal(r['h'], hidden[:, b]), b
            assert np.array_equal(r['hist'], x[b, 2 * T * 256:(2 * T + 1) * 256]), b
            assert r['tail'].any() and (taps == 1 or not np.array_equal(r['fctx'], f0['fctx']))
        # a masked reset leaves the record of a stream that was never used
        m = np.zeros(B, np.uint8)
        m[[3, 17]] = 1
        kb.reset(m)
        after = kb.export_state()
        assert np.array_equal(after[3], fresh[3]) and np.array_equal(after[17], fresh[17])
        assert np.array_equal(after[4], recs[4]) and np.array_equal(after[16], recs[16])
        hashes.append(f0['model_hash'])
        kb.delete()
    assert hashes[0] != hashes[1]


# ------------------------------------------------------------------------------------------------ 2. round trip in place

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', ['random', 'random5'])
def test_export_import_round_trip_in_place(random_model, random5_model, kind, precision):
    """Twin handles on the same input; one of them exports every stream and imports it back between the calls -- in place, and into
    permuted slots with the input rows permuted alike.  T alternates between 1 and more, so both parities of every ping-pong pair and
    the captured one-frame graphs are imported into."""
    model = random_model if kind == 'random' else random5_model
    B, Tmax = 48, 8
    seq = [1, 4, 1, 1, 8, 1, 3, 1, 1]
    x = synth_streams(B, sum(seq), seed=5)
    rng = np.random.default_rng(9)
    a, twin = batch(model, B, Tmax, precision), batch(model, B, Tmax, precision)
    pos = np.arange(B)  # slot of handle `a` in which stream i lives
    t0 = 0
    for n, T in enumerate(seq):
        xc = frames(x, t0, t0 + T)
        t0 += T
        want = twin.process(xc)
        xa = np.empty_like(xc)
        xa[pos] = xc
        got = a.process(xa)[pos]
        assert np.array_equal(got, want), (n, T)
        recs = a.export_state(pos)  # record i = stream i
        if n % 2:
            pos = rng.permutation(B)
        a.import_state(recs, pos)
    a.delete()
    twin.delete()


# ------------------------------------------------------------------------------------------------ 3. migration against the oracle

def migrate(model, precision, n, first, B2, T2, second, slots_seed=3, expect_routes=(), device=False):
    """`n` streams run `first` calls of 8 frames on a 64-stream handle (in slots of their own), move to random slots of a handle of B2
    streams x T2 frames, and finish there with the calls listed in `second`.  -> (engine output, oracle output, input) [n, frames]"""
    total = 8 * first + sum(second)
    x = synth_streams(n, total, seed=31)
    rng = np.random.default_rng(slots_seed)
    src = np.sort(rng.choice(64, n, replace=False))
    a = batch(model, 64, 8, precision, DEV_LIB)
    outs = []
    for c in range(first):
        xa = synth_streams(64, 8, seed=100 + c)  # (the other streams of the handle carry something else)
        xa[src] = frames(x, 8 * c, 8 * c + 8)
        outs.append(a.process(xa)[src])
    recs = a.export_state(src)
    a.delete()
    dst = rng.choice(B2, n, replace=False)
    b = batch(model, B2, T2, precision, DEV_LIB)
    warm = synth_streams(min(B2, 8), T2, seed=7)
    b.process(np.ascontiguousarray(np.tile(warm, (-(-B2 // warm.shape[0]), 1))[:B2]))  # the target slots have a past of their own
    b.import_state(recs, dst)
    routes, t0 = set(), 8 * first
    for T in second:
        xb = np.zeros((B2, T * 256), np.int16)
        xb[dst] = frames(x, t0, t0 + T)
        t0 += T
        outs.append(call(b, xb, 'device' if device else 'host', entry='classic')[dst])
        routes.add(route_of(b))
    b.delete()
    for r in expect_routes:
        assert r in routes, (routes, expect_routes)
    ref = oracle.Oracle(model, n, oracle_prec(precision)).process(x)
    return np.concatenate(outs, axis=1), ref, x


@pytest.mark.parametrize('precision,B2,T2,second,routes,device', [
    ('bf16', 1024, 32, [32, 1, 1], (ROUTE_PIPELINED, ROUTE_QUAD1), True),
    ('bf16', 4096, 8, [8, 1, 8, 1], (ROUTE_CHUNKED, ROUTE_QUAD1), True),  # the resident (chunked) kernels
    ('fp32', 4096, 8, [8, 1, 8], (ROUTE_WAVE, ROUTE_SMALL), True),
    ('fp32', 200, 5, [5, 1, 1, 5], (ROUTE_WAVE, ROUTE_SMALL), False),
    ('bf16', 24, 3, [1, 3, 1], (ROUTE_WAVE, ROUTE_SMALL), False),
])
def test_migration_matches_the_uninterrupted_oracle(random_model, precision, B2, T2, second, routes, device):
    if device:
        pytest.importorskip('torch')
    got, ref, _ = migrate(random_model, precision, 16, 2, B2, T2, second, expect_routes=routes, device=device)
    d = lsb(got, ref).max()
    print('migration %s -> %d x %d: max |engine - oracle| = %d LSB' % (precision, B2, T2, d))
    assert d <= tol(precision)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_migration_carries_the_feature_context(random5_model, precision):
    got, ref, _ = migrate(random5_model, precision, 12, 2, 96, 4, [4, 1, 1, 4, 1])
    d = lsb(got, ref).max()
    print('migration random5 %s: max |engine - oracle| = %d LSB' % (precision, d))
    assert d <= tol(precision)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_migration_keeps_the_adapted_noise_floor(gate_model, precision):
    """The default model carries its noise estimate in GRU state and needs seconds to adapt: 1.5 s on the first handle, the rest on the
    second.  The migrated streams equal the uninterrupted oracle -- and an oracle restarted at the move does not, so the comparison
    would see a reset."""
    n, first, second = 4, 12, [16, 1, 15]
    got, ref, x = migrate(gate_model, precision, n, first, 128, 16, second)
    d = lsb(got, ref).max()
    restarted = oracle.Oracle(gate_model, n, oracle_prec(precision)).process(frames(x, 8 * first, 8 * first + sum(second)))
    apart = lsb(restarted[:, 256:], ref[:, (8 * first + 1) * 256:]).max()
    print('migration gate %s: max |engine - oracle| = %d LSB; a restarted stream is %d LSB away' % (precision, d, apart))
    assert apart > BF16_TOL  # (else this comparison could not tell a reset from a move)
    assert d <= tol(precision)


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import koala_amd
model, blob_path, pcm_path, out_path = sys.argv[2:6]
raw = open(blob_path, 'rb').read()
x = np.load(pcm_path)
kb = koala_amd.create_batch('key', 32, 4, 'fp32', model_path=model)
n = len(raw) // kb.state_size
dst = [5 + 2 * i for i in range(n)]
kb.import_state([raw[i * kb.state_size:(i + 1) * kb.state_size] for i in range(n)], dst)
ys = []
for c in range(x.shape[1] // 1024):
    xb = np.zeros((32, 1024), np.int16)
    xb[dst] = x[:, c * 1024:(c + 1) * 1024]
    ys.append(kb.process(xb)[dst])
kb.delete()
np.save(out_path, np.concatenate(ys, axis=1))
'''


def test_records_travel_as_bytes_to_another_process(random_model, tmp_path):
    n = 6
    x = synth_streams(n, 24, seed=41)
    a = batch(random_model, 64, 8, 'fp32')
    xa = np.zeros((64, 16 * 256), np.int16)
    xa[10:10 + n] = frames(x, 0, 16)
    y0 = np.concatenate([a.process(frames(xa, 0, 8)), a.process(frames(xa, 8, 16))], axis=1)[10:10 + n]
    recs = a.export_state(np.arange(10, 10 + n))
    a.delete()
    blob = b''.join(bytes(recs[i]) for i in range(n))
    assert len(blob) == n * 10240
    (tmp_path / 'records.bin').write_bytes(blob)
    np.save(str(tmp_path / 'pcm.npy'), frames(x, 16, 24))
    child = subprocess.run([sys.executable, '-c', _CHILD, ROOT, random_model, str(tmp_path / 'records.bin'), str(tmp_path / 'pcm.npy'),
                            str(tmp_path / 'out.npy')], capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    got = np.concatenate([y0, np.load(str(tmp_path / 'out.npy'))], axis=1)
    assert np.array_equal(got, oracle.Oracle(random_model, n).process(x))


# ------------------------------------------------------------------------------------------------ 4. a fresh record is a reset

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', ['random', 'random5'])
def test_importing_a_fresh_record_is_a_masked_reset(random_model, random5_model, kind, precision):
    model = random_model if kind == 'random' else random5_model
    B, T = 40, 4
    x = synth_streams(B, 3 * T + 2, seed=13)
    a, twin = batch(model, B, T, precision), batch(model, B, T, precision)
    fresh = a.export_state([0])
    for c in range(2):
        assert np.array_equal(a.process(frames(x, c * T, (c + 1) * T)), twin.process(frames(x, c * T, (c + 1) * T)))
    idx = np.array([1, 2, 15, 16, 33, 39])
    m = np.zeros(B, np.uint8)
    m[idx] = 1
    a.import_state(np.repeat(fresh, idx.size, axis=0), idx)
    twin.reset(m)
    assert np.array_equal(a.export_state(), twin.export_state())
    for t0, t1 in ((2 * T, 2 * T + 1), (2 * T + 1, 3 * T + 1), (3 * T + 1, 3 * T + 2)):
        assert np.array_equal(a.process(frames(x, t0, t1)), twin.process(frames(x, t0, t1)))
    a.delete()
    twin.delete()


# ------------------------------------------------------------------------------------------------ 5. held streams

HOLD_CASES = [  # precision, B, Tmax, call lengths to draw from, calls, classes, routes that must have been taken, device pointers
    ('bf16', 32, 1, [1], 30, 8, (ROUTE_SMALL,), False),  # host one-frame calls on the handle's own stream: the captured graph
    ('fp32', 32, 1, [1], 30, 8, (ROUTE_SMALL,), False),
    ('bf16', 64, 8, [1, 8], 24, 6, (ROUTE_WAVE, ROUTE_SMALL), False),
    ('fp32', 64, 8, [1, 8], 24, 6, (ROUTE_WAVE, ROUTE_SMALL), False),
    ('bf16', 1024, 64, [1, 8, 64], 20, 3, (ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_CHUNKED), True),
    ('bf16', 4096, 64, [1, 8, 64], 20, 3, (ROUTE_CHUNKED, ROUTE_QUAD1), False),  # (64 frames from host memory: cut into sub-chunks)
    ('fp32', 4112, 8, [1, 8], 20, 3, (ROUTE_CHUNKED,), False),  # (257 m-tiles: past the fp32 wavefront and low-latency routes)
]


@pytest.mark.parametrize('precision,B,Tmax,lengths,calls,classes,routes,device', HOLD_CASES)
def test_held_streams_are_not_advanced(random_model, precision, B, Tmax, lengths, calls, classes, routes, device):
    if device:
        pytest.importorskip('torch')
    """Random hold masks over 20-30 calls.  Class 0 is held in EVERY call after the first; every stream's outputs of the calls it took
    part in equal the oracle on the inputs it was given in those calls."""
    rng = np.random.default_rng(B + Tmax + calls)
    cls = rng.integers(0, classes, B)
    cls[:classes] = np.arange(classes)
    kb = batch(random_model, B, Tmax, precision, DEV_LIB)
    refs = [oracle.Oracle(random_model, 1, oracle_prec(precision)) for _ in range(classes)]
    bar, worst, seen, before = tol(precision), 0, set(), None
    zero = np.flatnonzero(cls == 0)
    # (the required routes come round in the first calls, whatever the draw)
    plan = [lengths[-1]] + list(lengths) + [int(rng.choice(lengths)) for _ in range(calls - 1 - len(lengths))]
    for n, T in enumerate(plan):
        xc = synth_streams(classes, T, seed=1000 * n + B)
        held_c = np.zeros(classes, bool) if n == 0 else rng.random(classes) < 0.45
        held_c[0] = n > 0
        if n == 3:
            held_c[:] = True  # (a call in which nobody advances)
        hold = held_c[cls].astype(np.uint8)
        y = call(kb, np.ascontiguousarray(xc[cls]), 'device' if device else 'host', hold=hold, entry='classic')
        seen.add(route_of(kb))
        for c in np.flatnonzero(~held_c):
            want = refs[c].process(xc[c])
            rows = y[cls == c]
            worst = max(worst, int(lsb(rows, np.broadcast_to(want, rows.shape)).max()))
        if n == 0:
            before = kb.export_state(zero)
    print('hold %s %d x %d: routes %s, max |engine - oracle| = %d LSB' % (precision, B, Tmax, sorted(seen), worst))
    assert np.array_equal(kb.export_state(zero), before)
    kb.delete()
    for r in routes:
        assert r in seen, (sorted(seen), routes)
    assert worst <= bar


@pytest.mark.parametrize('precision,B,T', [('bf16', 4096, 64), ('bf16', 1024, 64), ('bf16', 1024, 1), ('fp32', 37, 5), ('bf16', 32, 1)])
def test_null_and_zero_hold_masks_are_the_plain_call(random_model, precision, B, T):
    torch = pytest.importorskip('torch')
    kb = batch(random_model, B, T, precision, DEV_LIB)
    x = torch.from_numpy(synth_streams(B, 2 * T, seed=3)).cuda()
    outs, routes, launches = [], [], []
    for form in ('plain', 'null', 'zero'):
        kb.reset()
        ys = []
        for c in range(2):
            xc = x[:, c * T * 256:(c + 1) * T * 256].contiguous()
            y = torch.zeros_like(xc)
            torch.cuda.synchronize()
            if form == 'plain':
                kb.process_device(T, xc.data_ptr(), y.data_ptr())
            else:
                kb.process_device_hold(T, xc.data_ptr(), y.data_ptr(), None if form == 'null' else np.zeros(B, np.uint8))
            kb.synchronize()
            ys.append(y.cpu().numpy())
        outs.append(np.concatenate(ys, axis=1))
        routes.append(kb.debug_read('route', T).tolist())
        # host calls: the same bits again, and under the profiler the same number of launches
        kb.reset()
        xh = x[:, :T * 256].cpu().numpy()
        yh = kb.process(xh) if form == 'plain' else kb.process_hold(xh, None if form == 'null' else np.zeros(B, np.uint8))
        assert np.array_equal(yh, outs[-1][:, :T * 256])
        kb.profile_enable(True)
        kb.process(xh) if form == 'plain' else kb.process_hold(xh, None if form == 'null' else np.zeros(B, np.uint8))
        launches.append([v['launches'] for v in kb.profile_read().values()])
        kb.profile_enable(False)
    kb.delete()
    assert routes[0] == routes[1] == routes[2], routes
    assert launches[0] == launches[1] == launches[2] and sum(launches[0]) > 0, launches
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 6. refusals leave the state alone

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_refused_calls_leave_the_state_alone(random_model, random5_model, precision):
    B, T = 20, 2
    x = synth_streams(B, 3 * T, seed=17)
    a, twin = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    other = 'fp32' if precision == 'bf16' else 'bf16'
    foreign = {}
    for name, model, prec in (('model', koala_amd.default_model_path(), precision), ('precision', random_model, other),
                              ('front_taps', random5_model, precision)):
        h = batch(model, 2, 1, prec)
        foreign[name] = h.export_state([0])
        h.delete()
    for c in range(2):
        assert np.array_equal(a.process(frames(x, c * T, (c + 1) * T)), twin.process(frames(x, c * T, (c + 1) * T)))
    good = a.export_state()
    state = good.copy()

    def refused(fn, *words):
        with pytest.raises(KoalaInvalidArgumentError) as e:
            fn()
        text = ' '.join(e.value.message_stack)
        for w in words:
            assert w in text, (w, text)

    mixed = good[:3].copy()
    mixed[2] = foreign['model'][0]
    refused(lambda: a.import_state(mixed, [4, 5, 6]), 'record 2', 'model hash')
    mixed[2] = good[2]
    mixed[1] = foreign['precision'][0]
    refused(lambda: a.import_state(mixed, [4, 5, 6]), 'record 1', 'precision')
    taps5 = np.zeros((1, a.state_size), np.uint8)
    taps5[0] = foreign['front_taps'][0, :a.state_size]  # (its header; the handle takes records of its own size)
    refused(lambda: a.import_state(taps5, [4]), 'record 0', 'front_taps')
    with pytest.raises(KoalaInvalidArgumentError):
        a.import_state(foreign['front_taps'], [4])  # the wrong record size: refused by the binding
    bad = good[:2].copy()
    bad[1, 0] ^= 0xff
    refused(lambda: a.import_state(bad, [0, 1]), 'record 1', 'magic')
    bad = good[:2].copy()
    bad[0, 4] = 2
    refused(lambda: a.import_state(bad, [0, 1]), 'record 0', 'version')
    refused(lambda: a.import_state(good[:2], [0, B]), 'streams[1]')
    refused(lambda: a.import_state(good[:2], [-1, 0]), 'streams[0]')
    refused(lambda: a.import_state(good[:3], [3, 7, 3]), 'twice')
    refused(lambda: a.export_state([0, B]), 'streams[1]')
    refused(lambda: a.export_state(np.arange(B + 1) % B), 'count')
    refused(lambda: a.import_state(np.repeat(good, 2, axis=0)[:B + 1], np.arange(B + 1) % B), 'count')
    with pytest.raises(KoalaInvalidArgumentError):
        a.export_state([])  # a count of 0
    with pytest.raises(KoalaInvalidArgumentError):
        a.import_state(good[:0], [])
    # ... through the C ABI too
    from ctypes import c_void_p
    lib = a._lib
    assert lib.pv_koala_batch_export_state(a._handle, 0, None, c_void_p(state.ctypes.data)) == PicovoiceStatuses.INVALID_ARGUMENT
    assert lib.pv_koala_batch_import_state(a._handle, B + 1, None, c_void_p(state.ctypes.data)) == PicovoiceStatuses.INVALID_ARGUMENT
    with pytest.raises(KoalaInvalidArgumentError):
        a.process_hold(frames(x, 0, T), np.zeros(B + 1, np.uint8))
    assert np.array_equal(a.export_state(), state)
    assert np.array_equal(a.process(frames(x, 2 * T, 3 * T)), twin.process(frames(x, 2 * T, 3 * T)))
    a.delete()
    twin.delete()


# ------------------------------------------------------------------------------------------------ 7. ordering

def test_export_waits_for_asynchronous_calls_in_flight(random_model):
    B, T = 256, 16
    x = synth_streams(16, 3 * T, seed=23)
    x = np.ascontiguousarray(np.tile(x, (B // 16, 1)))
    a, twin = batch(random_model, B, T, 'bf16'), batch(random_model, B, T, 'bf16')
    bufs = [(a.alloc_host(T), a.alloc_host(T)) for _ in range(3)]
    for c in range(3):
        bufs[c][0][:] = frames(x, c * T, (c + 1) * T)
        a.process_async(bufs[c][0], bufs[c][1])
    recs = a.export_state()  # (no wait in between)
    ys = [twin.process(frames(x, c * T, (c + 1) * T)) for c in range(3)]
    twin.synchronize()
    assert np.array_equal(recs, twin.export_state())
    for c in range(3):
        assert np.array_equal(bufs[c][1], ys[c])
    a.delete()
    twin.delete()


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_export_and_import_are_ordered_on_a_callers_stream(random_model, precision):
    torch = pytest.importorskip('torch')
    B, T = 80, 4
    x = synth_streams(B, 3 * T, seed=29)
    a, twin = batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    s = torch.cuda.Stream()
    a.set_stream(s.cuda_stream)
    xd = torch.from_numpy(x).cuda()
    perm = np.random.default_rng(1).permutation(B)
    parts = [xd[:, c * T * 256:(c + 1) * T * 256].contiguous() for c in range(3)]
    outs = [torch.zeros_like(p) for p in parts]
    xperm = torch.from_numpy(np.ascontiguousarray(frames(x, 2 * T, 3 * T)[np.argsort(perm)])).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a.process_device(T, parts[0].data_ptr(), outs[0].data_ptr())
        a.process_device(T, parts[1].data_ptr(), outs[1].data_ptr())
        recs = a.export_state()               # behind the two calls enqueued on the caller's stream
        a.import_state(recs, perm)            # record i -> slot perm[i]
        a.process_device(T, xperm.data_ptr(), outs[2].data_ptr())  # no host wait between the import and this call
    a.synchronize()
    s.synchronize()
    want = [twin.process(frames(x, c * T, (c + 1) * T)) for c in range(2)]
    assert np.array_equal(recs, twin.export_state())
    want.append(twin.process(frames(x, 2 * T, 3 * T)))
    assert np.array_equal(outs[0].cpu().numpy(), want[0]) and np.array_equal(outs[1].cpu().numpy(), want[1])
    assert np.array_equal(outs[2].cpu().numpy()[perm], want[2])
    a.set_stream(0)
    a.delete()
    twin.delete()

