"""
Calls with per-frame stream resets (include/pv_koala_batch.h, pv_koala_batch_process_chunk_resets*) on a real MI355X: the reset arms of the
chunked kernels (kns_stft.hip analysis / synthesis, kns_gru.hip gru_resident8_kernel / gru_kernel<PF32, 8>) against the oracle run as the
call cut at its reset frames with masked resets between the pieces -- fp32 the same samples, bf16 within the suite's bar.
"""
import numpy as np
import pytest

import koala_amd
from conftest import model_file, synth_streams
from gpu_kit import BF16_TOL, DEV_LIB, ROUTE_RESETS, lsb
from koala_amd import corpus
from koala_amd._errors import KoalaInvalidArgumentError
from oracle import oracle

pytestmark = pytest.mark.gpu


def random_mask(rng, B, T):
    """1-3 resets per stream, with frame 0, frame T - 1 and adjacent frames among them."""
    m = np.zeros((B, T), np.uint8)
    for b in range(B):
        k = rng.integers(1, 4)
        m[b, rng.choice(T, size=k, replace=False)] = 1
    m[0, 0] = m[1 % B, T - 1] = 1
    m[2 % B, T // 2] = m[2 % B, T // 2 + 1] = 1
    return m


@pytest.mark.parametrize('precision,B,T', [('bf16', 4096, 64), ('fp32', 4096, 64), ('bf16', 1024, 64), ('fp32', 37, 5)])
def test_null_and_zero_mask_are_the_plain_call(random_model, precision, B, T):
    torch = pytest.importorskip('torch')
    kb = koala_amd.create_batch('key', B, T, precision, model_path=random_model, library_path=DEV_LIB)
    x = torch.from_numpy(synth_streams(B, 2 * T, seed=3)).cuda()
    outs, routes = [], []
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
                kb.process_device_resets(T, xc.data_ptr(), y.data_ptr(), None if form == 'null' else np.zeros((B, T), np.uint8))
            kb.synchronize()
            ys.append(y.cpu().numpy())
        outs.append(np.concatenate(ys, axis=1))
        routes.append(kb.debug_read('route', T).tolist())
    kb.delete()
    assert routes[0] == routes[1] == routes[2], routes
    assert routes[0][0] != ROUTE_RESETS
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


CASES = [('random', 'fp32', 4096, 64, 2), ('random', 'bf16', 4096, 64, 2)] + \
        [(m, p, 40, 32, 3) for m in ('random', 'adaptive', 'unity') for p in ('fp32', 'bf16')]


@pytest.mark.parametrize('kind,precision,B,T,calls', CASES)
def test_random_masks_against_split_calls_on_the_oracle(kind, precision, B, T, calls):
    """Host calls (4096 x 64: 128 MiB, cut into sub-chunks -- the table is rebased to each); per frame, the frame right before every reset
    is checked on its own: in bf16 the narrow head of that frame rides in the recurrent launch of the reset step (kns_gru.hip, kYHead)."""
    model = model_file(kind)
    rng = np.random.default_rng(B + T + calls)
    x = synth_streams(B, T * calls, seed=21)
    kb = koala_amd.create_batch('key', B, T, precision, model_path=model, library_path=DEV_LIB)
    ref = oracle.Oracle(model, B, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
    for c in range(calls):
        xc = np.ascontiguousarray(x[:, c * T * 256:(c + 1) * T * 256])
        m = random_mask(rng, B, T)
        y = kb.process_resets(xc, m)
        assert int(kb.debug_read('route', T)[0]) == ROUTE_RESETS
        want = corpus.process_split(ref, xc, m)
        d = lsb(y, want).reshape(B, T, 256).max(axis=2)  # [stream, frame]
        if precision == 'fp32':
            assert d.max() == 0, (c, np.argwhere(d > 0)[:8].tolist())
        else:
            assert d.max() <= BF16_TOL, (c, int(d.max()), np.argwhere(d > BF16_TOL)[:8].tolist())
            before = [(b, t - 1) for b, t in zip(*np.nonzero(m)) if t > 0]
            assert max(int(d[b, t]) for b, t in before) <= BF16_TOL
    kb.delete()


def test_five_frame_front_end_refuses_resets_after_frame_0(random5_model):
    B, T = 8, 6
    x = synth_streams(B, 3 * T, seed=4)
    kb = koala_amd.create_batch('key', B, T, 'fp32', model_path=random5_model)
    ref = oracle.Oracle(random5_model, B)
    parts = [np.ascontiguousarray(x[:, c * T * 256:(c + 1) * T * 256]) for c in range(3)]
    m0 = np.zeros((B, T), np.uint8)
    m0[3, 0] = 1  # frame 0 only: allowed (the reset kernel in front of the call)
    assert np.array_equal(kb.process_resets(parts[0], m0), corpus.process_split(ref, parts[0], m0))
    bad = np.zeros((B, T), np.uint8)
    bad[2, 3] = 1
    with pytest.raises(KoalaInvalidArgumentError) as e:
        kb.process_resets(parts[1], bad)
    assert 'front-end' in str(e.value)
    # nothing was processed: the next plain call continues from the untouched state
    assert np.array_equal(kb.process(parts[1]), ref.process(parts[1]))
    kb.delete()


def test_async_caller_may_overwrite_its_mask(random_model):
    B, T, calls = 48, 16, 5
    rng = np.random.default_rng(9)
    x = synth_streams(B, T * calls, seed=8)
    masks = [random_mask(rng, B, T) for _ in range(calls)]
    parts = [np.ascontiguousarray(x[:, c * T * 256:(c + 1) * T * 256]) for c in range(calls)]
    kb = koala_amd.create_batch('key', B, T, 'fp32', model_path=random_model)
    want = [kb.process_resets(p, m) for p, m in zip(parts, masks)]
    kb.reset()
    pins = [(kb.alloc_host(T), kb.alloc_host(T)) for _ in range(3)]
    got = [None] * calls
    scratch = np.zeros((B, T), np.uint8)
    for c in range(calls):
        if c >= 3:
            kb.wait(2)
            got[c - 3] = pins[c % 3][1].copy()
        pins[c % 3][0][:] = parts[c]
        scratch[:] = masks[c]
        kb.process_async_resets(pins[c % 3][0], pins[c % 3][1], scratch)
        scratch[:] = rng.integers(0, 2, (B, T))  # overwritten while the call is in flight
    kb.wait(0)
    for c in range(max(0, calls - 3), calls):
        got[c] = pins[c % 3][1].copy()
    kb.delete()
    for c in range(calls):
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_device_calls_on_a_caller_stream_match_host_calls(random_model, precision):
    torch = pytest.importorskip('torch')
    B, T, calls = 300, 24, 3
    rng = np.random.default_rng(5)
    x = synth_streams(B, T * calls, seed=6)
    masks = [random_mask(rng, B, T) for _ in range(calls)]
    kb = koala_amd.create_batch('key', B, T, precision, model_path=random_model)
    want = [kb.process_resets(np.ascontiguousarray(x[:, c * T * 256:(c + 1) * T * 256]), masks[c]) for c in range(calls)]
    kb.reset()
    s = torch.cuda.Stream()
    kb.set_stream(s.cuda_stream)
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    ys = []
    with torch.cuda.stream(s):
        for c in range(calls):
            xc = xd[:, c * T * 256:(c + 1) * T * 256].contiguous()
            y = torch.empty_like(xc)
            kb.process_device_resets(T, xc.data_ptr(), y.data_ptr(), masks[c])
            ys.append(y)
    s.synchronize()
    kb.set_stream(0)
    kb.delete()
    for c in range(calls):
        assert np.array_equal(ys[c].cpu().numpy(), want[c]), c
