"""
Packet handles without a GPU (fourth extension): tests/packet_recipe.py, the numpy restatement, around the oracle and
around a pure delay, and koala_amd.packets, the pure-Python restatement of the engine's host-side plan.

Whatever the packet sizes, the packets' outputs concatenate to ([0] * (F - 1) ++ frames(x))[:N] -- exactly, in the oracle's fp32 and bf16 modes.

(The case "fill = F - 1, counts = max_frames * F": (F - 1 + max_frames F) // F is max_frames, not max_frames + 1 -- a call of at most
max_samples_per_call samples never completes more than ceil(max_samples_per_call / F) frames, so the inner engine's max_frames always
suffices.  The test pins that down; a stream reaches max_frames + 1 only with max_frames F + 1 samples, which is a larger handle.)
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import koala_amd
import packet_recipe as pr
from conftest import ROOT, model_file, synth_streams
from koala_amd import packets
from koala_amd._batch import BatchPackets


def signal(n, seed=5):
    return np.ascontiguousarray(synth_streams(1, n // 256 + 2, seed=seed)[0, :n])


def sizes_fixed(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def sizes_random(n, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < n:
        out.append(int(min(rng.integers(0, hi + 1) if rng.random() > 0.15 else 0, n - sum(out))))
    return out


def run(stream, x, sizes):
    got, t = [], 0
    for s in sizes:
        got.append(stream.push(x[t:t + s]))
        assert got[-1].size == s and stream.invariant()
        t += s
    assert t == x.size
    return np.concatenate(got)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('sizes', ['160', '320', 'random', 'ones'])
def test_oracle_in_packets_is_the_oracle_in_frames_behind_f_minus_1_zeros(precision, sizes):
    F, model = 256, model_file('random', 1234)
    n = 700 if sizes == 'ones' else 4000
    x = signal(n)
    cuts = {'160': sizes_fixed(n, 160), '320': sizes_fixed(n, 320), 'random': sizes_random(n, 700, 3), 'ones': [1] * n}[sizes]
    if sizes == 'random':
        assert 0 in cuts and max(cuts) > 2 * F
    got = run(pr.PacketStream(pr.oracle_stream(model, precision), F), x, cuts)
    want = pr.expected(pr.oracle_stream(model, precision), F, x)
    assert np.array_equal(got, want)
    assert not got[:F - 1].any() and want[F - 1:].any()


@pytest.mark.parametrize('F,size', [(128, 80), (768, 480), (768, 960), (512, 320), (256, 1)])
def test_delay_only_frames_at_every_rate(F, size):
    n = 6 * F + 37
    x = signal(n, seed=9)
    got = run(pr.PacketStream(pr.DelayStream(F), F), x, sizes_fixed(n, size))
    assert np.array_equal(got, pr.expected(pr.DelayStream(F), F, x))
    # a unity mask: the input delayed by D + F - 1 = 2 F - 1 samples, bit for bit
    assert np.array_equal(got[2 * F - 1:], x[:n - (2 * F - 1)]) and not got[:2 * F - 1].any()


def test_full_buffer_and_a_whole_call_of_frames():
    F, max_frames = 256, 3
    s = pr.PacketStream(pr.DelayStream(F), F)
    x = signal(F - 1 + max_frames * F + 10, seed=2)
    a = s.push(x[:F - 1])
    assert s.fill == F - 1 and s.last_frames == 0 and s.invariant()
    b = s.push(x[F - 1:F - 1 + max_frames * F])
    # (F - 1 + max_frames F) // F: the call completes max_frames frames and the buffer is full of pending input again
    assert s.last_frames == max_frames and s.fill == F - 1 and s.invariant()
    k, new_fill = packets.frames_due([F - 1], [max_frames * F], F)
    assert (int(k[0]), int(new_fill[0])) == (max_frames, F - 1)
    assert all(T <= max_frames for _, T, _ in packets.plan(k, max_frames))
    # one sample more is one frame more: the largest count a handle of max_frames * F + 1 samples takes
    k1, _ = packets.frames_due([F - 1], [max_frames * F + 1], F)
    assert int(k1[0]) == max_frames + 1 and -(-(max_frames * F + 1) // F) == max_frames + 1
    c = s.push(x[F - 1 + max_frames * F:])
    assert np.array_equal(np.concatenate([a, b, c]), pr.expected(pr.DelayStream(F), F, x))


def test_restart_is_a_fresh_stream():
    F = 256
    x, y = signal(1000, seed=1), signal(1500, seed=2)
    s = pr.PacketStream(pr.DelayStream(F), F)
    run(s, x, sizes_fixed(1000, 160))
    assert s.fill == 1000 % F
    s.fn = pr.DelayStream(F)  # every reset: the frame handle's state and the packetiser's
    s.reset()
    assert s.fill == 0 and not s.buf.any() and s.invariant()
    got = run(s, y, sizes_fixed(1500, 160))
    assert np.array_equal(got, run(pr.PacketStream(pr.DelayStream(F), F), y, sizes_fixed(1500, 160)))


@pytest.mark.parametrize('F', [128, 256, 768])
def test_a_record_taken_mid_frame_continues_identically(F):
    n, at = 5 * F + 11, 2 * F + 77
    x = signal(n, seed=4)
    sizes = sizes_random(n, F + 50, 8)
    whole = run(pr.PacketStream(pr.DelayStream(F), F), x, sizes)
    a = pr.PacketStream(pr.DelayStream(F), F)
    first = a.push(x[:at])
    assert a.fill == at % F != 0
    rec, inner = a.record(), a.fn.state()
    assert rec.size == pr.record_bytes(F) and rec.size % 16 == 0 and not rec[4 + 2 * (F - 1):].any()
    assert {128: 272, 256: 528, 768: 1552}[F] == rec.size
    b = pr.PacketStream(pr.DelayStream(F), F)
    b.fn.set_state(inner)
    b.set_record(rec)
    assert b.invariant()
    rest = run(b, x[at:], sizes_random(n - at, 300, 9))
    assert np.array_equal(np.concatenate([first, rest]), whole)


# ------------------------------------------------------------------------------------------------ koala_amd.packets: the host-side plan

def test_frames_due():
    k, f = packets.frames_due([0, 255, 100, 0, 255], [0, 1, 160, 512, 768], 256)
    assert k.tolist() == [0, 1, 1, 2, 3] and f.tolist() == [0, 0, 4, 0, 255]


@pytest.mark.parametrize('max_frames', [1, 2, 3, 8])
def test_plan_covers_every_streams_frames_once_and_in_order(max_frames):
    rng = np.random.default_rng(max_frames)
    for _ in range(200):
        k = rng.integers(0, 7, rng.integers(1, 12))
        subs = packets.plan(k, max_frames)
        done = np.zeros(k.size, int)
        for c0, T, hold in subs:
            assert 1 <= T <= max_frames
            run_ = np.ones(k.size, bool) if hold is None else hold == 0
            assert (done[run_] == c0).all()  # in order, nothing twice, nothing skipped
            assert hold is None or hold.any()
            done[run_] += T
        assert (done == k).all()
        assert sum(T for _, T, _ in subs) == k.max()


def test_plan_equal_k_is_one_plain_call_and_all_zero_is_none():
    assert packets.plan([0, 0, 0], 4) == []
    (c0, T, hold), = packets.plan([2, 2, 2], 4)
    assert (c0, T, hold) == (0, 2, None)
    subs = packets.plan([1, 0, 2], 4)
    assert [(c0, T) for c0, T, _ in subs] == [(0, 1), (1, 1)]
    assert subs[0][2].tolist() == [0, 1, 0] and subs[1][2].tolist() == [1, 1, 0]


def test_packet_clock():
    c = packets.PacketClock(3, 320)
    c.push(0, np.arange(160, dtype=np.int16))
    c.push(2, np.arange(500, dtype=np.int16))
    c.push(0, np.arange(160, 200, dtype=np.int16))
    counts, pcm = c.take()
    assert counts.tolist() == [200, 0, 320] and pcm.shape == (3, 320)
    assert np.array_equal(pcm[0, :200], np.arange(200)) and np.array_equal(pcm[2], np.arange(320))
    counts, pcm = c.take()
    assert counts.tolist() == [0, 0, 180] and np.array_equal(pcm[2, :180], np.arange(320, 500))


# ------------------------------------------------------------------------------------------------ the library: kernels and symbols

HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_packet_kernels_build_for_gfx950_without_scratch_or_spills_and_store_16_byte_words(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_scan
    out = tmp_path / 'kns_packet.s'
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    assert 'csrc/kns_packet.hip' in mk and 'obj/kns_packet.o' in mk
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + [f for f in cxx if f != '-fPIC'] +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_packet.hip'), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    assert isa_scan.scan(text) == []
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n'
                      r'(?:(?!\.name:).*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', text)
    facts = {name: (int(p), int(s), int(v)) for name, p, s, v in meta}
    for kernel in ('packet_in_kernel', 'packet_out_kernel', 'packet_reset_kernel', 'packet_state_kernel'):
        name, = [n for n in facts if kernel in n]
        print(name, '(scratch, sgpr spills, vgpr spills) =', facts[name])
        assert facts[name] == (0, 0, 0), (name, facts[name])
    for kernel in ('packet_in_kernel', 'packet_out_kernel'):  # the staged rows leave as aligned 16-byte words
        body = text.split('%sENS_10PacketArgsE:' % kernel)[1].split('s_endpgm')[0]
        assert 'global_store_dwordx4' in body and ('ds_read_b128' in body or 'ds_read2_b64' in body), kernel


def test_packet_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in ('pv_koala_batch_init_packets', 'pv_koala_batch_is_packet_handle', 'pv_koala_batch_process_packets'):
            assert hasattr(lib, sym), (path, sym)
            assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    # pv_koala_batch_call_t is what it was: eight members, `asynchronous` the last
    call = re.search(r'typedef struct \{([^}]*)\} pv_koala_batch_call_t;', header).group(1)
    assert len(re.findall(r';', call)) == 8 and call.strip().splitlines()[-1].strip().startswith('int32_t asynchronous;')
    assert ctypes.sizeof(BatchPackets) == 64


def test_python_checks_a_packet_handles_arguments_before_it_loads_anything(random_model):
    for bad in (-1, 2.5, '160'):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, library_path='/nonexistent.so', packet_samples=bad)
