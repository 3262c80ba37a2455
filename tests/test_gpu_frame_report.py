"""
Frame report (include/pv_koala_batch.h: pv_koala_batch_process_call, pv_koala_process_report) on a real MI355X:
the kReport forms of koala_amd/csrc/kns_stft.hip's synthesis kernel under every route of the dispatch table, through the product library
(the developer library only where the route is read back).

Expected rows come from tests/frame_report_recipe.py, the numpy float32 restatement of the spec.  fp32: e_in, e_out and mask_sum == the
recipe.  bf16: e_in == the recipe (the spectrum is the spec's in both configurations); e_out relative and mask_sum / 257 absolute within
BF16_E_OUT_REL and BF16_MEAN_GAIN_ABS of the recipe module.  The `want_*` functions build every test's expected rows, so that tools/frame_report_bars.py
can run the same inputs through the plain and the jittered bf16 oracle on the CPU: the bars are 4 x the largest distance it finds.
"""
import ctypes

import numpy as np
import pytest

import koala_amd
from conftest import load_wav, synth_streams
from frame_report_recipe import BF16_E_OUT_REL, BF16_MEAN_GAIN_ABS, ReportRecipe
from gpu_kit import DEV_LIB, ROUTE_RESETS, batch, call, classes, frames, route_of
from koala_amd import corpus
from koala_amd._batch import BatchCall
from koala_amd._koala import fetch_error_stack
from min_gain_recipe import GAINS, NCLS, SHAPES

pytestmark = pytest.mark.gpu

def check(got, want, precision, what):
    """got, want float32 [..., 4].  Prints the figures before it asserts."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not got[..., 3].any(), what  # the reserved word
    nz = want[..., 1] != 0
    rel = np.zeros(want.shape[:-1])
    rel[nz] = np.abs(got[..., 1].astype(np.float64)[nz] - want[..., 1][nz]) / want[..., 1][nz]
    mg = np.abs(got[..., 2].astype(np.float64) - want[..., 2]) / 257.0
    print('%s %s: e_in %d of %d rows differ, e_out max rel %.3g (%d rows differ), mask_sum / 257 max abs %.3g (%d rows differ)' %
          (what, precision, int((got[..., 0] != want[..., 0]).sum()), rel.size, rel.max(), int((got[..., 1] != want[..., 1]).sum()), mg.max(),
           int((got[..., 2] != want[..., 2]).sum())))
    assert np.array_equal(got[..., 0], want[..., 0]), what
    assert np.array_equal(got[..., 1][~nz], want[..., 1][~nz]), what
    if precision == 'bf16':
        assert rel.max() <= BF16_E_OUT_REL and mg.max() <= BF16_MEAN_GAIN_ABS, (what, float(rel.max()), float(mg.max()))
    else:
        assert np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 2], want[..., 2]), what


# ------------------------------------------------------------------------------------------------ expected rows (shared with the bars' probe)

def want_mixed(model, precision, calls, seed=41):
    """per call: rows [NCLS, T, 4]; the gains of call n are GAINS rotated by n"""
    xc = synth_streams(NCLS, sum(T for T, _ in calls), seed=seed)
    rec, rows, t0 = ReportRecipe(model, NCLS, precision), [], 0
    for n, (T, _) in enumerate(calls):
        rows.append(rec.process(frames(xc, t0, t0 + T), np.roll(GAINS, n)))
        t0 += T
    return xc, rows


def reset_masks(T):
    rng = np.random.default_rng(6)
    rc = [(rng.random((NCLS, T)) < 0.2).astype(np.uint8) for _ in range(2)]
    rc[0][2, 0] = rc[0][2, 1] = rc[1][3, T - 1] = 1  # frame 0, adjacent frames, the last frame
    r0 = np.zeros((NCLS, 1), np.uint8)
    r0[[1, 4]] = 1
    return rc + [r0]


def want_resets(model, precision, T=8):
    xc = synth_streams(NCLS, 2 * T + 1, seed=43)
    rec, rc = ReportRecipe(model, NCLS, precision), reset_masks(T)
    spans = [(0, T), (T, 2 * T), (2 * T, 2 * T + 1)]
    return xc, [rec.process_resets(frames(xc, a, b), GAINS, rc[i]) for i, (a, b) in enumerate(spans)]


def want_hold(model, precision, T=4):
    """three calls; the second is run twice: `full` advances every class, `skip` does not see it (the held streams)"""
    xc = synth_streams(NCLS, 3 * T, seed=47)
    full, skip = ReportRecipe(model, NCLS, precision), ReportRecipe(model, NCLS, precision)
    x = [frames(xc, n * T, (n + 1) * T) for n in range(3)]
    rows = [full.process(x[0], GAINS), full.process(x[1], GAINS), full.process(x[2], GAINS)]
    skip.process(x[0], GAINS)
    return xc, rows, skip.process(x[2], GAINS)


def want_single(model, precision, pcm, nframes=365):
    x = np.ascontiguousarray(pcm[:nframes * 256]).reshape(1, -1)
    return x, ReportRecipe(model, 1, precision).process(x, np.array([0.25], np.float32))[0]


def bf16_cases(random_model):
    """name -> thunk returning a flat list of row arrays: every bf16 input of this module (tools/frame_report_bars.py)"""
    cases = {}
    for s in SHAPES:
        if s[0] == 'bf16':
            cases['mixed %dx%d' % (s[1], s[2])] = lambda s=s: want_mixed(random_model, 'bf16', s[3])[1]
    cases['resets'] = lambda: want_resets(random_model, 'bf16')[1]
    cases['hold'] = lambda: (lambda r: r[1] + [r[2]])(want_hold(random_model, 'bf16'))
    cases['single'] = lambda: [want_single(random_model, 'bf16', load_wav('test.wav'))[1]]
    return cases


# ------------------------------------------------------------------------------------------------ every route, mixed gains

@pytest.mark.parametrize('precision,B,Tmax,calls,routes', SHAPES, ids=['%s-%dx%d' % (s[0], s[1], s[2]) for s in SHAPES])
def test_every_route_reports_the_recipe_and_changes_nothing_else(random_model, precision, B, Tmax, calls, routes):
    if any(m != 'host' and m != 'async' for _, m in calls):
        pytest.importorskip('torch')
    xc, want = want_mixed(random_model, precision, calls)
    cls = classes(B, B, NCLS)
    x = xc[cls]
    # kb asks for the report (product library), plain never does; dev repeats kb's calls on the developer library, where the route is read back
    kb, plain, dev = batch(random_model, B, Tmax, precision), batch(random_model, B, Tmax, precision), batch(random_model, B, Tmax, precision, DEV_LIB)
    taken, t0 = set(), 0
    for n, (T, mode) in enumerate(calls):
        gc = np.roll(GAINS, n)[cls]
        for h in (kb, plain, dev):
            h.set_min_gain(gc)
        xn = frames(x, t0, t0 + T)
        got, rep = call(kb, xn, mode, report=True)
        base = call(plain, xn, mode)
        again, rep_dev = call(dev, xn, mode, report=True)
        taken.add(route_of(dev))
        what = 'call %d (%d frames, %s)' % (n, T, mode)
        check(rep, want[n][cls], precision, what)
        assert np.array_equal(rep, rep_dev), what
        assert np.array_equal(got, base) and np.array_equal(again, base), what  # the samples do not know of the report
        one = gc == 1
        assert np.array_equal(rep[one][..., 0], rep[one][..., 1]), what  # g = 1: Y = X, bit for bit, in both precisions
        t0 += T
    assert np.array_equal(kb.export_state(), plain.export_state())  # nor does the state
    for h in (kb, plain, dev):
        h.delete()
    for r in routes:
        assert r in taken, (taken, routes)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_sub_chunked_host_call_into_page_locked_buffers(random_model, precision):
    """a host call of 16 MiB from page-locked memory: every sub-chunk's report rows are copied straight into the caller's array, beside its
    samples -- the rows and samples of the same call through pageable memory (the staging path, checked against the recipe above)"""
    B, T = 1024, 32
    x = synth_streams(NCLS, 2 * T, seed=53)[classes(B, 3, NCLS)]
    pin, page, plain = batch(random_model, B, T, precision), batch(random_model, B, T, precision), batch(random_model, B, T, precision)
    for h in (pin, page, plain):
        h.set_min_gain(np.resize(GAINS, B))
    for n in range(2):
        xn = frames(x, n * T, (n + 1) * T)
        y0, r0 = call(page, xn, 'host', report=True)
        y1, r1 = call(pin, xn, 'pinned', report=True)
        y2 = call(plain, xn, 'pinned')
        assert np.array_equal(r1, r0) and np.array_equal(y1, y0) and np.array_equal(y2, y0), n
        assert (r1[..., 0] > 0).all() and not r1[..., 3].any()
    for h in (pin, page, plain):
        h.delete()


# ------------------------------------------------------------------------------------------------ exact identities

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_unity_model_and_silence(unity_model, precision):
    pytest.importorskip('torch')
    for B, T, seq in ((21, 4, [(1, 'host'), (4, 'host'), (4, 'device')]), (1024, 32, [(32, 'host'), (1, 'host'), (32, 'device')])):
        x = synth_streams(B, sum(t for t, _ in seq), seed=51)
        x[3] = 0  # digital silence
        x[B - 1, :256 * 2] = 0
        kb = batch(unity_model, B, T, precision)
        kb.set_min_gain(np.resize(GAINS, B))
        t0 = 0
        for n, mode in seq:
            _, rep = call(kb, frames(x, t0, t0 + n), mode, report=True)
            assert (rep[..., 2] == np.float32(257.0)).all() and np.array_equal(rep[..., 0], rep[..., 1]) and not rep[..., 3].any(), (B, n, mode)
            assert not rep[3][..., :2].any() and (rep[[b for b in range(B) if b not in (3, B - 1)]][..., 0] > 0).all()
            if t0 == 0:
                assert not rep[B - 1, :min(n, 2), :2].any()  # (silence: zeros in, zeros out)
            t0 += n
        kb.delete()


# ------------------------------------------------------------------------------------------------ per-frame resets

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('mode', ['host', 'inplace', 'async'])
def test_per_frame_resets(random_model, precision, mode):
    if mode == 'inplace':
        pytest.importorskip('torch')
    B, T = 40, 8
    xc, want = want_resets(random_model, precision, T)
    cls = classes(B, 5, NCLS)
    rc = reset_masks(T)
    kb, plain, dev = batch(random_model, B, T, precision), batch(random_model, B, T, precision), batch(random_model, B, T, precision, DEV_LIB)
    for h in (kb, plain, dev):
        h.set_min_gain(GAINS[cls])
    for n in range(2):
        xn, r = frames(xc, n * T, (n + 1) * T)[cls], np.ascontiguousarray(rc[n][cls])
        got, rep = call(kb, xn, mode, reset=r, report=True)
        base = call(plain, xn, mode, reset=r)
        call(dev, xn, mode, reset=r, report=True)
        assert route_of(dev) == ROUTE_RESETS
        check(rep, want[n][cls], precision, 'resets, call %d (%s)' % (n, mode))  # a reset frame: the spectrum of [0 | frame]
        assert np.array_equal(got, base)
    # a one-frame call that restarts streams at frame 0: the reset kernel in front of the captured frame
    xn, r = frames(xc, 2 * T, 2 * T + 1)[cls], np.ascontiguousarray(rc[2][cls])
    got, rep = kb.process_call(xn, reset=r, report=True)
    check(rep, want[2][cls], precision, 'resets, one frame')
    assert np.array_equal(got, plain.process_resets(xn, r))
    assert np.array_equal(kb.export_state(), plain.export_state())
    for h in (kb, plain, dev):
        h.delete()


# ------------------------------------------------------------------------------------------------ held streams

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_held_streams(random_model, precision):
    B, T = 40, 4
    xc, want, want_skipped = want_hold(random_model, precision, T)
    cls = classes(B, 7, NCLS)
    hold = (np.random.default_rng(8).random(B) < 0.4).astype(np.uint8)
    hold[0], hold[1] = 1, 0
    free = hold == 0
    kb = batch(random_model, B, T, precision)
    kb.set_min_gain(GAINS[cls])
    x = [frames(xc, n * T, (n + 1) * T)[cls] for n in range(3)]
    _, rep = kb.process_call(x[0], report=True)
    check(rep, want[0][cls], precision, 'hold, call 0')
    before = kb.export_state()
    _, rep = kb.process_call(x[1], hold=hold, report=True)
    check(rep[free], want[1][cls][free], precision, 'hold, call 1 (streams not held)')
    assert np.array_equal(kb.export_state()[~free], before[~free])  # the held rows' state is what it was
    _, rep = kb.process_call(x[2], report=True)
    check(rep, np.where(free[:, None, None], want[2][cls], want_skipped[cls]), precision, 'hold, call 2')
    kb.delete()


# ------------------------------------------------------------------------------------------------ the single-stream ABI

@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_single_stream_handle(random_model, test_pcm, precision, monkeypatch):
    """one frame per call: the hipGraph path, with its second set of captures for calls that ask"""
    monkeypatch.setenv('KOALA_AMD_PRECISION', precision)
    x, want = want_single(random_model, precision, test_pcm)
    n = x.shape[1] // 256
    k, mixed, plain = (koala_amd.create('key', model_path=random_model) for _ in range(3))
    for h in (k, mixed, plain):
        h.set_min_gain(0.25)
    rows, same = [], True
    for t in range(n):
        fr = x[0, t * 256:(t + 1) * 256]
        y, row = k.process_with_report(fr)
        rows.append(row)
        base = plain.process(fr)
        ym = mixed.process_with_report(fr)[0] if (t // 3) % 2 else mixed.process(fr)  # asking and not asking, interleaved
        same = same and y == base and ym == base
    for h in (k, mixed, plain):
        h.delete()
    check(np.array(rows), want, precision, 'single stream, %d frames' % n)
    assert same  # the samples of a handle that never asked


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_leave_state_and_output_untouched(random_model):
    torch = pytest.importorskip('torch')
    B, T = 24, 4
    kb = batch(random_model, B, T, 'fp32')
    x = synth_streams(B, 2 * T, seed=61)
    kb.process(frames(x, 0, T))
    before = kb.export_state()
    xn = frames(x, T, 2 * T)
    out = np.full_like(xn, 12345)
    rep = np.full((B, T, 4), -7.0, np.float32)
    lib = kb._lib

    def raw(**kw):
        c = BatchCall(ctypes.sizeof(BatchCall), T, xn.ctypes.data, out.ctypes.data, None, None, rep.ctypes.data, 0)
        for k_, v in kw.items():
            setattr(c, k_, v)
        return lib.pv_koala_batch_process_call(kb._handle, ctypes.byref(c))

    reset = np.zeros((B, T), np.uint8)
    reset[1, 2] = 1
    hold = np.zeros(B, np.uint8)
    hold[2] = 1
    dev_rep = torch.zeros((B, T, 4), dtype=torch.float32, device='cuda')
    pin_in, pin_out = kb.alloc_host(T), kb.alloc_host(T)
    pin_in[:] = xn
    pin_out[:] = 12345
    refused = [
        ('struct_size', lambda: raw(struct_size=ctypes.sizeof(BatchCall) - 8), 'INVALID_ARGUMENT'),
        ('struct_size 0', lambda: raw(struct_size=0), 'INVALID_ARGUMENT'),
        ('device report, host audio', lambda: raw(report=dev_rep.data_ptr()), 'RUNTIME_ERROR'),
        ('pageable report, asynchronous', lambda: raw(pcm=pin_in.ctypes.data, enhanced=pin_out.ctypes.data, asynchronous=1), 'RUNTIME_ERROR'),
        ('hold with reset', lambda: raw(reset=reset.ctypes.data, hold=hold.ctypes.data), 'INVALID_ARGUMENT'),
        ('hold, asynchronous', lambda: raw(pcm=pin_in.ctypes.data, enhanced=pin_out.ctypes.data, hold=hold.ctypes.data, asynchronous=1, report=None),
         'INVALID_ARGUMENT'),
    ]
    for what, fn, status in refused:
        st = fn()
        assert st.name == status, (what, st)
        msgs = fetch_error_stack(lib)
        print(what, '->', st.name, msgs)
        assert len(msgs) >= 1
        kb.synchronize()
        assert (out == 12345).all() and (pin_out == 12345).all() and (rep == -7.0).all() and not dev_rep.any().item(), what
        assert np.array_equal(kb.export_state(), before), what
    # ... and the same call without the flaw goes through
    assert raw().name == 'SUCCESS' and (rep[..., 3] == 0).all() and (rep[..., 0] > 0).all()
    kb.delete()


# ------------------------------------------------------------------------------------------------ corpus

@pytest.mark.parametrize('mode', ['host', 'async', 'device'])
def test_corpus_reports_every_file_as_if_run_alone(random_model, mode):
    if mode == 'device':
        pytest.importorskip('torch')
    S, T, N = 8, 16, 40
    rng = np.random.default_rng(71)
    lengths = rng.integers(300, 30 * 256, N)
    pool = synth_streams(N, 31, seed=72)
    signals = [pool[u, :lengths[u]].copy() for u in range(N)]
    kb = batch(random_model, S, T, 'fp32')
    enhanced, reports = corpus.enhance_corpus(kb, signals, T, mode=mode, report=True)
    only = corpus.enhance_corpus(kb, signals, T, mode=mode)
    kb.delete()
    assert all(np.array_equal(a, b) for a, b in zip(enhanced, only))
    alone = batch(random_model, 1, T, 'fp32')
    for u, sig in enumerate(signals):
        nf = int(corpus.utterance_frames([len(sig)])[0])
        assert reports[u].shape == (nf, 4)  # its own frames and the flush frame
        pad = np.zeros((-(-nf // T)) * T * 256, np.int16)
        pad[:len(sig)] = sig
        alone.reset()
        rows = np.concatenate([alone.process_call(pad[None, c * T * 256:(c + 1) * T * 256], report=True)[1][0] for c in range(len(pad) // (T * 256))])
        assert np.array_equal(reports[u], rows[:nf]), u
    alone.delete()
