"""
What the GPU suite (tests/test_gpu_*.py, tests/sample_rate_cases.py) shares: the bars, the route numbers, handles, one driver for a frame
call in every pointer mode, and the small array helpers.  Not a test module: imported like the *_recipe.py modules.  Features keep their
own expected values (the recipes) and their own bars where those differ; those bars are built on the constants below.
"""
import numpy as np

import koala_amd
from conftest import synth_streams
from oracle import oracle

# ---------------------------------------------------------------------------------------------------- bars

# bf16 engine vs the oracle with the same rounding points: the two differ in the last bit of GEMM outputs (the bf16 MFMA truncates
# far-apart addends inside its sums of eight, profiles/r05_mfma_probe.txt) and of the gate / head / log transcendentals (hardware
# v_exp / v_rcp / v_log, <= 1 ulp from the correctly rounded functions the oracle uses), and such a bit now and then flips an fp16 /
# bf16 rounding downstream.  Largest difference ever measured in this suite: see DESIGN.md section 5.
# Bar 5 LSB (the same as __graft_entry__.smoke(), whose white-noise sample measures 4; this suite's own maximum is 3) plus the
# distribution checked wherever a histogram is taken.  Constants, not knobs: nothing in the environment can loosen them.
BF16_TOL = 5
# share of samples within 1 LSB: 99.99 % over the bench's 16.8 M samples of synthetic streams (bench.py --full fails its run below
# 99.9 %); on real speech through the random-weight model (test_gpu_parity.test_bf16_against_both_oracles, 102 400 samples) 99.1 % measured
BF16_WITHIN_1 = 0.99
# fp32 engine: the oracle's values, every one of them
FP32_TOL = 0


def tol(precision):
    return BF16_TOL if precision == 'bf16' else FP32_TOL


def lsb(a, b):
    """the distance of every sample, in LSB"""
    return np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))


def check_pcm(got, want, precision, what):
    """fp32: the expected samples; bf16: the suite's bars.  Prints the figures before it asserts."""
    d = lsb(got, want)
    print('%s %s: max |engine - recipe| = %d LSB, %.4f %% within 1, %d samples' % (what, precision, int(d.max()), 100.0 * (d <= 1).mean(), d.size))
    if precision == 'bf16':
        assert d.max() <= BF16_TOL and (d <= 1).mean() >= BF16_WITHIN_1, (what, int(d.max()), float((d <= 1).mean()))
    else:
        assert d.max() <= FP32_TOL, (what, int(d.max()))


def same(a, b):
    """element for element, bit for bit (float rows compared as their bits: no -0 == 0, no NaN != NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- routes

# the -DKNS_DEV build of the same sources: the only library that reads the KOALA_AMD_* developer switches and reports a call's route
DEV_LIB = koala_amd.developer_library_path()
# koala_amd/csrc/kns_engine.cpp, enum Route: tests/test_route_table.py holds every ROUTE_* of this module to the enum's text
ROUTE_CHUNKED, ROUTE_SMALL, ROUTE_SMALL_STEPS, ROUTE_QUAD1, ROUTE_WAVE, ROUTE_PIPELINED, ROUTE_RESETS = 0, 1, 2, 3, 4, 5, 6


def route_info(kb):
    """developer library: the last call's [route, ., the mask head rode in the synthesis launch, a spectrum was stored]"""
    return kb.debug_read('route', 1)


def route_of(kb):
    return int(route_info(kb)[0])


def segments_of(kb):
    """developer library: (frames per time segment of the last analysis launch, of the last synthesis launch, the last call's synthesis launches)"""
    return tuple(int(v) for v in kb.debug_read('segments', 1)[4:])


# ---------------------------------------------------------------------------------------------------- shapes and streams

def flen(rate):
    """frame_length of a handle at `rate`"""
    return rate * 256 // 16000


def frames(x, t0, t1, F=256):
    """frames t0 .. t1 - 1 of every row"""
    return np.ascontiguousarray(x[:, t0 * F:t1 * F])


def cut(x, rate, seq):
    """x in consecutive calls of seq[i] frames"""
    out, t0 = [], 0
    for T in seq:
        out.append(frames(x, t0, t0 + T, flen(rate)))
        t0 += T
    return out


def streams(B, n, seed=0):
    """[B, n] int16, every row its own signal"""
    return np.ascontiguousarray(synth_streams(B, -(-n // 256), seed)[:, :n])


def tiled(a, B):
    """the rows of `a` repeated over B slots"""
    return np.ascontiguousarray(np.concatenate([a] * -(-B // a.shape[0]))[:B])


def replicas(a, R):
    """every replica of the first R rows == the first"""
    return same(a, tiled(a[:R], a.shape[0]))


def delayed(x, n=256):
    """the input delayed by n samples (delay_sample of a 16 kHz frame handle: one frame)"""
    return np.concatenate([np.zeros((x.shape[0], n), x.dtype), x[:, :-n]], axis=1)


def oracle_prec(precision):
    return oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32


def classes(B, seed, ncls):
    """a class for every slot, scattered at random, every class somewhere"""
    cls = np.random.default_rng(seed).integers(0, ncls, B)
    cls[:ncls] = np.arange(ncls)
    return cls


# ---------------------------------------------------------------------------------------------------- handles

def batch(model, B, T, precision, lib=None, **kw):
    """kw: sample_rate, packet_samples, sample_format, channels, channel_link, high_band"""
    return koala_amd.create_batch('key', B, T, precision, model_path=model, library_path=lib, **kw)


# ---------------------------------------------------------------------------------------------------- one frame call

MARK = 0x5A5A  # what device `enhanced` is prefilled with around and behind what a call may write
GUARD = 64     # elements of MARK on either side of device `enhanced`


def _guarded(flat, inplace, offset):
    """device buffers of one call -> (pcm, enhanced, the whole buffer around enhanced): `enhanced` lies `offset` elements behind an aligned
    address between two guard zones of MARK; in place pcm is enhanced"""
    import torch
    n = flat.numel()
    big = torch.zeros(GUARD + offset + n + GUARD, dtype=flat.dtype, device='cuda')
    big.view(torch.uint8)[:] = MARK & 0xFF
    out = big[GUARD + offset:]
    if inplace:
        out[:n] = flat.cuda()
        return out, out, big
    src = torch.zeros(n + offset + 8, dtype=flat.dtype, device='cuda')
    src[offset:offset + n] = flat.cuda()
    return src[offset:], out, big


def _unguarded(big, n, offset, shape):
    """the samples between the guard zones, which must have come back untouched"""
    got = big.cpu().numpy()
    marks = np.concatenate([got[:GUARD + offset], got[GUARD + offset + n:]]).view(np.uint8)
    assert (marks == (MARK & 0xFF)).all(), 'the call wrote outside `enhanced`'
    return got[GUARD + offset:GUARD + offset + n].reshape(shape)


def call(kb, x, mode, *, report=False, reset=None, hold=None, entry='call'):
    """one frame call -> enhanced shaped like x, or (enhanced, report) when `report` is set.
    mode: 'host' (pageable), 'pinned' (page-locked, synchronous), 'async' (page-locked, asynchronous, waited for), 'device', 'inplace'
    (device, enhanced == pcm), 'offset' (device, both pointers one element behind an aligned address).  The device modes put `enhanced`
    between guard zones of MARK, asserted untouched, and prefill the report with -1.
    entry: 'call' is pv_koala_batch_process_call (process_call / process_device_call / process_async_call); 'classic' the older entry
    points, one exported function per combination (process, process_resets, process_hold, their _device and _async forms), which have no
    report."""
    assert entry in ('call', 'classic') and not (entry == 'classic' and (report or mode == 'pinned'))
    x = np.ascontiguousarray(x)
    T = x.size // (kb.num_streams * kb.frame_length)
    if mode == 'host':
        if entry == 'call':
            return kb.process_call(x, reset=reset, hold=hold, report=report)
        assert reset is None or hold is None
        return kb.process_hold(x, hold) if hold is not None else kb.process_resets(x, reset) if reset is not None else kb.process(x)
    if mode in ('pinned', 'async'):
        a, b = kb.alloc_host(T), kb.alloc_host(T)
        rep = kb.alloc_host_report(T) if report else None
        a[:] = x
        if mode == 'pinned':  # the copy engines write the caller's arrays directly
            kb._call(T, a.ctypes.data, b.ctypes.data, reset, hold, rep.ctypes.data if report else None, False)
        else:
            assert hold is None  # (no asynchronous entry takes held streams)
            if entry == 'call':
                kb.process_async_call(a, b, report=rep, reset=reset)
            elif reset is None:
                kb.process_async(a, b)
            else:
                kb.process_async_resets(a, b, reset)
            kb.synchronize()
        return (b.copy(), rep.copy()) if report else b.copy()
    assert mode in ('device', 'inplace', 'offset'), mode
    import torch
    flat = torch.from_numpy(x.reshape(-1))
    n, offset = flat.numel(), 1 if mode == 'offset' else 0
    xin, out, big = _guarded(flat, mode == 'inplace', offset)
    rd = torch.full((kb.num_streams, T, 4), -1.0, dtype=torch.float32, device='cuda') if report else None
    torch.cuda.synchronize()
    if entry == 'call':
        kb.process_device_call(T, xin.data_ptr(), out.data_ptr(), rd.data_ptr() if report else 0, reset=reset, hold=hold)
    elif hold is not None:
        assert reset is None
        kb.process_device_hold(T, xin.data_ptr(), out.data_ptr(), hold)
    elif reset is not None:
        kb.process_device_resets(T, xin.data_ptr(), out.data_ptr(), reset)
    else:
        kb.process_device(T, xin.data_ptr(), out.data_ptr())
    kb.synchronize()
    y = _unguarded(big, n, offset, x.shape)
    return (y, rd.cpu().numpy()) if report else y


# ---------------------------------------------------------------------------------------------------- one packet call

def packet_call(kb, pcm, counts, restart=None, mode='device', fill=MARK):
    """one packet call into an `enhanced` prefilled with `fill` -> (the whole matrix as it came back, frames per stream).  'host': the
    caller's pageable arrays; 'device': device pointers, `enhanced` between guard zones of MARK, asserted untouched"""
    pcm = np.ascontiguousarray(pcm)
    N = pcm.size // kb.num_streams
    if mode == 'host':
        out = np.full_like(pcm, fill)
        return out, kb._packets(N, counts, pcm.ctypes.data, out.ctypes.data, restart, None, 0)
    assert mode == 'device', mode
    import torch
    xin, out, big = _guarded(torch.from_numpy(pcm.reshape(-1)), False, 0)
    out[:pcm.size] = torch.from_numpy(np.full(pcm.size, fill, pcm.dtype)).cuda()
    torch.cuda.synchronize()
    done = kb.process_device_packets(N, counts, xin.data_ptr(), out.data_ptr(), restart)
    kb.synchronize()
    return _unguarded(big, pcm.size, 0, pcm.shape), done
