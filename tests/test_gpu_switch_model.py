"""
The network kernels (kns_gemm.hip, kns_gru.hip, kns_gruq.hip) against the integer reference of the switch model (tests/switch_recipe.py), on a
real MI355X, with == on every route of Engine::run_device's dispatch table, the route read back from the developer library after every call.

Every gate of the switch model saturates, so the bf16 network is a digital circuit: the hidden state is exactly {-1, 0, 1}, the mask
exactly {0, 1}, and the samples those of the mask.  bf16 is held to the integer reference: the `hidden` tap, the `mask`
tap where the call formed a mask outside the synthesis launch, the samples, and the `h` part of the product library's stream records.  fp32
saturates to 6e-39 instead of 0 (tests/test_switch_recipe.py), so its mask and samples are held to the fp32 oracle, as everywhere; its hidden
state is the reference's, which that module proves of the oracle.

The sixteen streams are tiled over the B slots (slot i holds stream i % 16): the first sixteen slots are compared with the reference, every
other slot -- the ragged last m-tile of 4100 included -- with its stream.  Shapes: tests/test_gpu_edge_inputs.py and
tests/test_gpu_high_band_routes.py.
"""
import collections

import numpy as np
import pytest

import koala_amd
import switch_recipe as sr
from gpu_kit import (DEV_LIB, ROUTE_CHUNKED, ROUTE_PIPELINED, ROUTE_QUAD1, ROUTE_RESETS, ROUTE_SMALL, ROUTE_SMALL_STEPS, ROUTE_WAVE, batch, call, cut,
                     oracle_prec, replicas, route_info, same, tiled)
from oracle import oracle

pytestmark = pytest.mark.gpu

R = sr.ROWS
H_OFFSET = 1568  # of float h[8][271] in a stream record ("Stream record")

# `flagged`: the reset flag is set on frame 2 of every call on every third stream.  `env`: a developer switch the handle is made under.
Case = collections.namedtuple('Case', 'precision name route B T calls mode flagged env seed taps', defaults=(False, None, 1, 1))
CASES = [
    Case('bf16', 'small', ROUTE_SMALL, 16, 1, 4, 'host', seed=1),
    Case('bf16', 'quad', ROUTE_QUAD1, 960, 1, 4, 'device', seed=2),
    Case('bf16', 'wavefront-49', ROUTE_WAVE, 784, 4, 2, 'device', seed=3),
    Case('bf16', 'pipelined', ROUTE_PIPELINED, 784, 32, 2, 'device', seed=1),
    Case('bf16', 'pipelined-chunk16', ROUTE_PIPELINED, 784, 32, 2, 'inplace', env='KOALA_AMD_PIPE_CHUNK=16', seed=2),
    Case('bf16', 'chunked-ragged', ROUTE_CHUNKED, 4100, 2, 2, 'inplace', seed=3),
    Case('bf16', 'chunked', ROUTE_CHUNKED, 4112, 2, 2, 'device', seed=1),
    Case('bf16', 'resets', ROUTE_RESETS, 64, 4, 2, 'device', True, seed=2),
    Case('fp32', 'small', ROUTE_SMALL, 16, 1, 4, 'host', seed=3),
    Case('fp32', 'small-steps', ROUTE_SMALL_STEPS, 64, 2, 2, 'device', env='KOALA_AMD_WAVE_MT=0', seed=1),
    Case('fp32', 'wavefront', ROUTE_WAVE, 64, 2, 2, 'device', seed=2),
    Case('fp32', 'chunked', ROUTE_CHUNKED, 4112, 2, 2, 'device', seed=3),
    Case('fp32', 'resets', ROUTE_RESETS, 64, 4, 2, 'device', True, seed=1),
    # the five-frame front-end: gemm_front5_t1_kernel on one-frame calls, gemm_front5_kernel on the others
    Case('bf16', 'front5-small', ROUTE_SMALL, 16, 1, 7, 'host', taps=5),
    Case('bf16', 'front5-wavefront', ROUTE_WAVE, 64, 4, 2, 'device', taps=5),
    Case('bf16', 'front5-chunked', ROUTE_CHUNKED, 1040, 2, 3, 'device', taps=5),
    Case('fp32', 'front5-small', ROUTE_SMALL, 16, 1, 7, 'host', taps=5),
]


def cid(c):
    return '%s-%s-%dx%dx%d' % (c.precision, c.name, c.B, c.T, c.calls)


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp('switch_models')
    return {(seed, taps): sr.model_path(d, seed, taps) for seed, taps in [(s, 1) for s in sr.SEEDS] + [(1, 5)]}


def reset_flags(c):
    f = np.zeros((R, c.T), np.uint8)
    if c.flagged:
        f[::3, 2] = 1
    return f


_want = {}


def want(models, c):
    """what the calls of a case must deliver, made once per (model, precision, cut): a list per call of dict(pcm, mask, hidden) -- hidden the
    integer reference's state behind the call's last frame; bf16: mask and pcm the reference's; fp32: the fp32 oracle's"""
    key = (c.seed, c.taps, c.precision, c.T, c.calls, c.flagged)
    if key not in _want:
        model = models[(c.seed, c.taps)]
        ref = sr.Reference(sr.Circuit(c.seed, c.taps), model, R, c.precision)
        o = oracle.Oracle(model, R, oracle_prec(c.precision)) if c.precision == 'fp32' else None
        out = []
        for xc in cut(sr.switch_streams(c.T * c.calls), 16000, [c.T] * c.calls):
            w = ref.process(xc, reset_flags(c) if c.flagged else None)
            one = {'hidden': w['hidden'][-1].astype(np.float32), 'mask': w['mask'], 'pcm': w['pcm']}
            if o is not None:
                if c.flagged:  # a reset right before frame 2 of the call
                    p0, m0 = o.process_with_mask(np.ascontiguousarray(xc[:, :512]))
                    o.reset(reset_flags(c)[:, 2])
                    p1, m1 = o.process_with_mask(np.ascontiguousarray(xc[:, 512:]))
                    one['pcm'], one['mask'] = np.concatenate([p0, p1], axis=1), np.concatenate([m0, m1])
                else:
                    one['pcm'], one['mask'] = o.process_with_mask(xc)
                assert np.array_equal(one['pcm'], w['pcm']) and np.array_equal(one['mask'] == 1, w['mask'] == 1)
            out.append(one)
        assert ref.min_pre >= sr.MARGIN and ref.max_gi < sr.FP16_MAX and ref.min_gap >= sr.MARGIN / 1024.0
        _want[key] = out
    return _want[key]


def check(kb, y, w, what, mask=True):
    """hidden tap, mask tap (where the call kept a mask) and samples of one call against `w`; every replica against its stream"""
    B = kb.num_streams
    hidden = kb.debug_read('hidden', 1)
    d = sr.first_difference(hidden[:, :R], w['hidden'], ('layer', 'stream', 'unit'))
    assert d is None, '%s: hidden state (frame: the call\'s last): %s' % (what, d)
    assert replicas(hidden.transpose(1, 0, 2).reshape(B, -1), R), '%s: hidden state of a replica' % what
    if mask and route_info(kb)[2] == 0:  # (a one-frame bf16 call forms its mask inside the synthesis launch: no tap)
        T = w['mask'].shape[0]
        m = kb.debug_read('mask', T)
        d = sr.first_difference(m[:, :R].view(np.uint32), w['mask'].view(np.uint32), ('frame', 'stream', 'bin'))
        assert d is None, '%s: mask (as bits): %s' % (what, d)
        assert replicas(m.transpose(1, 0, 2).reshape(B, -1), R), '%s: mask of a replica' % what
    d = sr.first_difference(y[:R], w['pcm'], ('stream', 'sample'))
    assert d is None, '%s: samples: %s' % (what, d)
    assert replicas(y, R), '%s: samples of a replica' % what


def run(models, c, monkeypatch, mode=None, lib=DEV_LIB):
    if c.env:
        monkeypatch.setenv(*c.env.split('='))
    kb = batch(models[(c.seed, c.taps)], c.B, c.T, c.precision, lib)
    flags = tiled(reset_flags(c), c.B) if c.flagged else None
    for n, (xc, w) in enumerate(zip(cut(sr.switch_streams(c.T * c.calls), 16000, [c.T] * c.calls), want(models, c))):
        y = call(kb, tiled(xc, c.B), mode or c.mode, reset=flags)
        if lib == DEV_LIB:
            assert int(route_info(kb)[0]) == c.route, (cid(c), n, route_info(kb).tolist())
            check(kb, y, w, '%s call %d' % (cid(c), n))
        else:  # the product library: samples, and the h part of every stream's record (state_export_kernel's unpacking of the layouts)
            assert sr.first_difference(y[:R], w['pcm'], ('stream', 'sample')) is None and replicas(y, R), (cid(c), n)
            rec = kb.export_state()
            h = np.ascontiguousarray(rec[:, H_OFFSET:H_OFFSET + 8 * sr.H * 4]).view(np.float32).reshape(c.B, 8, sr.H)
            d = sr.first_difference(h[:R].transpose(1, 0, 2), w['hidden'], ('layer', 'stream', 'unit'))
            assert d is None, '%s call %d: h of the stream records: %s' % (cid(c), n, d)
            assert replicas(h.reshape(c.B, -1), R), (cid(c), n)
    kb.delete()


# ---------------------------------------------------------------------------------------------------- every route

@pytest.mark.parametrize('c', CASES, ids=cid)
def test_every_route_equals_the_integer_reference(models, monkeypatch, c):
    run(models, c, monkeypatch)


@pytest.mark.parametrize('c', [c for c in CASES if c.env is None and c.name not in ('pipelined', 'chunked')], ids=cid)
def test_stream_records_of_the_product_library_hold_the_references_hidden_state(models, monkeypatch, c):
    run(models, c, monkeypatch, lib=None)


@pytest.mark.parametrize('mode', ['host', 'inplace', 'offset'])
@pytest.mark.parametrize('c', [CASES[2], CASES[10]], ids=cid)
def test_host_and_in_place_calls_equal_the_integer_reference(models, monkeypatch, c, mode):
    run(models, c, monkeypatch, mode=mode)


# ---------------------------------------------------------------------------------------------------- one call against many

@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
@pytest.mark.parametrize('B,route', [(16, ROUTE_SMALL), (960, ROUTE_QUAD1)])
def test_one_call_of_k_frames_equals_k_one_frame_calls(models, monkeypatch, precision, B, route):
    """the one-frame bf16 calls form their mask inside the synthesis launch (kMaskIn) and have no mask tap: their samples and hidden state
    are held to the reference's, and to the K-frame call's"""
    K = 4
    c1 = Case(precision, 'one-frame', route if precision == 'bf16' else ROUTE_SMALL, B, 1, K, 'device', seed=3)
    ck = Case(precision, 'k-frames', -1, B, K, 1, 'device', seed=3)
    x = tiled(sr.switch_streams(K), B)
    k1, kk = (batch(models[(3, 1)], B, K, precision, DEV_LIB) for _ in range(2))
    ys = []
    for t, (xc, w) in enumerate(zip(cut(x, 16000, [1] * K), want(models, c1))):
        ys.append(call(k1, xc, 'device'))
        info = route_info(k1)
        assert int(info[0]) == c1.route and bool(info[2]) == (precision == 'bf16'), (t, info.tolist())
        check(k1, ys[-1], w, '%s call %d' % (cid(c1), t))
    yk = call(kk, x, 'device')
    assert int(route_info(kk)[0]) not in (ROUTE_SMALL, ROUTE_QUAD1)
    check(kk, yk, want(models, ck)[0], cid(ck))
    assert same(np.concatenate(ys, axis=1), yk) and same(k1.debug_read('hidden', 1), kk.debug_read('hidden', 1))
    k1.delete(), kk.delete()


# ---------------------------------------------------------------------------------------------------- alternative kernels

# the developer switches tests/test_gpu_parity.py::test_alternative_kernels_give_identical_pcm walks
SWITCHES = ['KOALA_AMD_GRU_STREAM', 'KOALA_AMD_GEMM_GENERIC', 'KOALA_AMD_GEMM_NO_WSR', 'KOALA_AMD_NO_SMALL', 'KOALA_AMD_NO_GRAPH',
            'KOALA_AMD_STORE_SPECTRUM', 'KOALA_AMD_DEBUG_TAPS', 'KOALA_AMD_NO_QUAD', 'KOALA_AMD_NO_HEAD_FUSE', 'KOALA_AMD_NO_STFT_FUSE',
            'KOALA_AMD_WAVE_MT=0', 'KOALA_AMD_WAVE_MT=4096', 'KOALA_AMD_WAVE_GROUP=2', 'KOALA_AMD_NO_SPIN_WAIT', 'KOALA_AMD_PIPE_MT=0',
            'KOALA_AMD_PIPE_CHUNK=8', 'KOALA_AMD_PIPE_WHOLE_STFT', 'KOALA_AMD_NO_WEIGHT_CACHE']
SHAPES = [('bf16', 16, 1, 3, 1), ('bf16', 960, 1, 3, 2), ('bf16', 64, 4, 2, 3), ('bf16', 1040, 2, 2, 1), ('bf16', 784, 32, 1, 2), ('fp32', 64, 2, 2, 3),
          ('bf16', 16, 1, 6, 5)]


@pytest.mark.parametrize('switch', SWITCHES)
def test_alternative_kernels_equal_the_integer_reference(models, monkeypatch, switch):
    """whatever kernels a switch selects: the reference's hidden state, mask and samples (the route is printed, not asserted)"""
    monkeypatch.setenv(switch.split('=')[0], switch.split('=')[1] if '=' in switch else '1')
    for precision, B, T, calls, model in SHAPES:
        seed, taps = (1, 5) if model == 5 else (model, 1)
        c = Case(precision, switch, -1, B, T, calls, 'device', seed=seed, taps=taps)
        kb = batch(models[(seed, taps)], B, T, precision, DEV_LIB)
        for n, (xc, w) in enumerate(zip(cut(sr.switch_streams(T * calls), 16000, [T] * calls), want(models, c))):
            y = call(kb, tiled(xc, B), 'device')
            print(switch, cid(c), 'call', n, 'route', route_info(kb).tolist())
            check(kb, y, w, '%s call %d' % (cid(c), n))
        kb.delete()


# ---------------------------------------------------------------------------------------------------- the single-stream ABI

@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_single_stream_abi_equals_the_integer_reference(models, monkeypatch, precision):
    """pv_koala_process, one frame per call through the captured graph: four of the streams for 12 frames"""
    monkeypatch.setenv('KOALA_AMD_PRECISION', precision)
    frames, rows = 12, (0, 5, 10, 15)
    c = Case(precision, 'abi', -1, R, frames, 1, 'host', seed=2)
    w = want(models, c)[0]
    k = koala_amd.create('key', model_path=models[(2, 1)], device='gpu:0')
    for r in rows:
        k.reset()
        y = np.concatenate([np.array(k.process(sr.switch_streams(frames)[r, t * 256:(t + 1) * 256]), np.int16) for t in range(frames)])
        d = sr.first_difference(y, w['pcm'][r], ('sample',))
        assert d is None, (r, d)
    k.delete()
