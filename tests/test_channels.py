"""
Multi-channel batch handles without a GPU (seventh extension): koala_amd.channels against the index sentence of the
specification, the channel kernels' build for gfx950 (exactly six kernels, no scratch, no spills), the exported symbols, the config struct
that did not grow, and Python's argument checks.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import koala_amd
from conftest import ROOT
from koala_amd import channels
from koala_amd._batch import BatchConfig


@pytest.mark.parametrize('dtype', [np.uint8, np.int16, np.float32])
@pytest.mark.parametrize('C', [2, 3, 8])
def test_interleave_and_deinterleave_are_inverses_and_match_the_index_sentence(C, dtype):
    G, n = 3, 37
    rng = np.random.default_rng(C)
    x = rng.integers(0, 200, (G, n * C)).astype(dtype)
    p = channels.deinterleave(x, C)
    assert p.shape == (G * C, n) and p.dtype == x.dtype
    for g in range(G):
        for c in range(C):
            for i in range(n):  # sample i of stream g C + c is element [g][i C + c]
                assert p[g * C + c, i] == x[g, i * C + c]
    back = channels.interleave(p, C)
    assert back.shape == x.shape and back.dtype == x.dtype and np.array_equal(back, x)
    assert np.array_equal(channels.deinterleave(x.reshape(G, n, C), C), p)  # [G, n, C] is the same memory
    q = rng.integers(0, 200, (G * C, n)).astype(dtype)
    assert np.array_equal(channels.deinterleave(channels.interleave(q, C), C), q)
    with pytest.raises(ValueError):
        channels.deinterleave(x[:, :-1], C)
    with pytest.raises(ValueError):
        channels.interleave(q[:-1], C)
    for bad in (0, 9, '2', None, True):
        with pytest.raises(ValueError):
            channels.interleave(q, bad)


HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_channel_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    out = tmp_path / 'kns_channels.s'
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    assert 'csrc/kns_channels.hip' in mk and 'obj/kns_channels.o' in mk and 'csrc/pv_api_extensions.cpp' in mk and 'obj/pv_api_extensions.o' in mk
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + [f for f in cxx if f != '-fPIC'] +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_channels.hip'), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n'
                      r'(?:(?!\.name:).*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', text)
    facts = {name: (int(p), int(s), int(v)) for name, p, s, v in meta}
    assert len(facts) == 6, sorted(facts)  # nothing but: split and join, three element widths
    for kind in ('split', 'join'):
        for width in (1, 2, 4):
            name = [n for n in facts if 'channels_%s_kernelILi%dE' % (kind, width) in n]
            assert len(name) == 1, (kind, width, sorted(facts))
            print(name[0], '(scratch, sgpr spills, vgpr spills) =', facts[name[0]])
            assert facts[name[0]] == (0, 0, 0), (name[0], facts[name[0]])


def test_channel_symbols_are_exported_and_declared_and_the_config_did_not_grow(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in ('pv_koala_batch_init_channels', 'pv_koala_batch_channels'):
            assert hasattr(lib, sym), (path, sym)
            assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    config = re.search(r'typedef struct \{([^}]*)\} pv_koala_batch_config_t;', header).group(1)
    assert len(re.findall(r'int32_t \w+;', config)) == 7 and ctypes.sizeof(BatchConfig) == 28
    assert 'channels' not in config
    # the single-stream ABI stays the reference's: one channel
    assert 'channels' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read().lower()


def test_python_checks_channels_before_it_loads_anything(random_model):
    for bad in (0, 9, '2', None, True, 2.0):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='channels'):
            koala_amd.create_batch('key', 8, 1, 'fp32', model_path=random_model, library_path='/nonexistent.so', channels=bad)
    with pytest.raises(koala_amd.KoalaInvalidArgumentError, match='channels'):
        koala_amd.create_batch('key', 5, 1, 'fp32', model_path=random_model, library_path='/nonexistent.so', channels=2)
    # a handle that never reached a library: the shape checks are Python's alone
    kb = koala_amd.KoalaBatch.__new__(koala_amd.KoalaBatch)
    kb.num_streams, kb.frame_length, kb.packet_samples, kb.channels = 6, 256, 0, 2
    for wrong in (np.zeros((6, 256), np.int16), np.zeros((3, 511), np.int16), np.zeros((3, 256, 3), np.int16), np.zeros((2, 768), np.int16)):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.process(wrong)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.process_call(wrong)
    rows, shape = kb._rows(np.zeros((3, 256, 2), np.int16))
    assert rows.shape == (6, 256) and shape == (3, 256, 2)
    rows, shape = kb._rows(np.zeros((3, 512), np.int16))
    assert rows.shape == (6, 256) and shape == (3, 512)
    assert koala_amd.KoalaBatch.channels == 1  # what a handle is unless it was made with channels
