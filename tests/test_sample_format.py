"""
Sample formats without a GPU (fifth extension): tests/sample_format_recipe.py against the anchors of the specification
over all 256 bytes and all 65 536 samples, koala_amd.formats against the recipe everywhere, the float conversion at its edges, the format
kernels' build for gfx950 (no scratch, no spills), the exported symbols and Python's argument checks.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import koala_amd
import sample_format_recipe as sf
from conftest import ROOT
from koala_amd import formats
from koala_amd._batch import BatchConfig

ALL_BYTES = np.arange(256, dtype=np.uint8)
ALL_S16 = sf.ALL_SAMPLES.astype(np.int16)


def test_recipe_mu_law_anchors():
    dec, enc = sf.DEC[sf.ULAW], sf.ENC[sf.ULAW]
    assert np.unique(dec).size == 255 and dec.max() == 32124 and dec.min() == -32124
    assert dec[0xFF] == 0 and dec[0x7F] == 0
    back = enc[dec.astype(np.int32) + 32768]
    assert [b for b in range(256) if back[b] != b] == [0x7F] and back[0x7F] == 0xFF
    assert (sf.ulaw_enc(0), sf.ulaw_enc(-1), sf.ulaw_enc(32767), sf.ulaw_enc(-32768)) == (0xFF, 0x7F, 0x80, 0x00)


def test_recipe_a_law_anchors():
    dec, enc = sf.DEC[sf.ALAW], sf.ENC[sf.ALAW]
    assert np.unique(dec).size == 256 and dec.max() == 32256 and dec.min() == -32256
    assert np.array_equal(enc[dec.astype(np.int32) + 32768], ALL_BYTES)
    assert (sf.alaw_enc(0), sf.alaw_enc(-1), sf.alaw_enc(32767), sf.alaw_enc(-32768)) == (0xD5, 0x55, 0xAA, 0x2A)
    assert sf.alaw_dec(0xD5) == 8


@pytest.mark.parametrize('law', [sf.ULAW, sf.ALAW])
def test_recipe_decode_of_encode_is_idempotent_on_all_of_int16(law):
    once = sf.decode(law, sf.encode(law, ALL_S16))
    assert np.array_equal(sf.decode(law, sf.encode(law, once)), once)
    # the encoder truncates: the decoded level is the centre of the cell the sample fell into, never further away than the cell is wide
    assert np.abs(once.astype(np.int32) - ALL_S16).max() <= 1024


def test_recipe_f32_edges():
    assert np.array_equal(sf.decode(sf.F32, sf.F32_EDGES), sf.F32_EDGES_WANT)
    back = sf.encode(sf.F32, ALL_S16)
    assert back.dtype == np.float32 and np.array_equal(back.astype(np.float64) * 32768, ALL_S16.astype(np.float64))
    assert np.array_equal(sf.decode(sf.F32, back), ALL_S16)  # for inputs s / 32768 the format is the identity


@pytest.mark.parametrize('fmt', [sf.S16, sf.F32, sf.ULAW, sf.ALAW])
def test_koala_amd_formats_is_the_recipe_everywhere(fmt):
    name = sf.NAMES[fmt]
    assert formats.FORMATS[fmt] == name and formats.dtype(name) == sf.DTYPES[fmt] and formats.format_name(fmt) == name
    got = formats.encode(name, ALL_S16)
    assert got.dtype == sf.DTYPES[fmt] and np.array_equal(got, sf.encode(fmt, ALL_S16))
    if fmt in (sf.ULAW, sf.ALAW):
        x = ALL_BYTES
    elif fmt == sf.S16:
        x = ALL_S16
    else:
        rng = np.random.default_rng(3)
        x = np.concatenate([sf.F32_EDGES, got, (rng.standard_normal(20000) * 0.7).astype(np.float32),
                            ((rng.integers(-70000, 70000, 20000) + 0.5) / 32768).astype(np.float32),  # ties, in and out of range
                            rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)])  # any bit pattern
    back = formats.decode(name, x)
    assert back.dtype == np.int16 and np.array_equal(back, sf.decode(fmt, x))
    with pytest.raises(ValueError):
        formats.decode(name, np.zeros(4, np.float64))
    with pytest.raises(ValueError):
        formats.format_name('pcm')


# ------------------------------------------------------------------------------------------------ the library: kernels and symbols

HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_format_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    out = tmp_path / 'kns_format.s'
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    assert 'csrc/kns_format.hip' in mk and 'obj/kns_format.o' in mk and 'csrc/pv_api_extensions.cpp' in mk and 'obj/pv_api_extensions.o' in mk
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + [f for f in cxx if f != '-fPIC'] +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', 'kns_format.hip'), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = re.findall(r'\.name:\s+(\S+)\n(?:(?!\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:(?!\.name:).*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n'
                      r'(?:(?!\.name:).*\n)*?\s+\.vgpr_spill_count:\s+(\d+)', text)
    facts = {name: (int(p), int(s), int(v)) for name, p, s, v in meta}
    kernels = [n for n in facts if 'format_' in n]
    assert len(kernels) == 6, kernels  # in and out, three formats
    for name in kernels:
        print(name, '(scratch, sgpr spills, vgpr spills) =', facts[name])
        assert facts[name] == (0, 0, 0), (name, facts[name])


def test_format_symbols_are_exported_and_declared(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in ('pv_koala_batch_init_config', 'pv_koala_batch_sample_format'):
            assert hasattr(lib, sym), (path, sym)
            assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    config = re.search(r'typedef struct \{([^}]*)\} pv_koala_batch_config_t;', header).group(1)
    assert len(re.findall(r'int32_t \w+;', config)) == 7 and ctypes.sizeof(BatchConfig) == 28
    for name, value in (('S16', 0), ('F32', 1), ('ULAW', 2), ('ALAW', 3)):
        assert re.search(r'PV_KOALA_SAMPLE_%s = %d\b' % (name, value), header)
    # the single-stream ABI stays the reference's: int16 only
    single = open(os.path.join(ROOT, 'include', 'pv_koala.h')).read().lower()
    assert 'format' not in single and 'law' not in single


def test_python_checks_the_format_and_the_dtype_before_it_loads_anything(random_model):
    for bad in ('pcm', 'F32', 1, None):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            koala_amd.create_batch('key', 2, 1, 'fp32', model_path=random_model, library_path='/nonexistent.so', sample_format=bad)
    # a handle that never reached a library: the dtype checks are Python's alone
    kb = koala_amd.KoalaBatch.__new__(koala_amd.KoalaBatch)
    kb.sample_format, kb._dtype, kb._dtype_name, kb.num_streams, kb.frame_length, kb.packet_samples = 'ulaw', np.uint8, 'uint8', 2, 128, 0
    for wrong in (np.zeros((2, 128), np.int16), np.zeros((2, 128), np.float32), [[0] * 128] * 2):
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.process(wrong)
        with pytest.raises(koala_amd.KoalaInvalidArgumentError):
            kb.process_call(wrong)
    with pytest.raises(koala_amd.KoalaInvalidArgumentError):
        kb._audio(np.zeros((2, 128), np.int16))
    assert kb._audio(np.zeros((2, 256), np.uint8)) == 2
    kb.packet_samples = 80
    with pytest.raises(koala_amd.KoalaInvalidArgumentError):
        kb.process_packets(np.zeros((2, 80), np.int16), [80, 80])
