"""
Linked channels (include/pv_koala_batch.h: LINKED CHANNELS; DESIGN.md section 2, eighth extension) without a GPU: the recipe's identities,
the symbols, the config struct, the Python argument checks and the gfx950 build of the linked synthesis kernels.
tests/test_gpu_channel_link.py checks the samples on the GPU; tests/test_channel_link_abi.py the C entry points.
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
from channel_link_recipe import LinkRecipe
from conftest import ROOT, model_file, synth_streams
from koala_amd import KoalaInvalidArgumentError
from koala_amd._batch import BatchConfig, KoalaBatch
from koala_amd.channels import link_masks

sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SYMBOLS = ('pv_koala_batch_set_channel_link', 'pv_koala_batch_get_channel_link')


def test_link_masks_is_the_group_max_and_refuses_other_channel_counts():
    rng = np.random.default_rng(1)
    for C in (2, 4, 8):
        m = rng.random((3 * C, 2, 257)).astype(np.float32)
        out = link_masks(m, C)
        assert out.shape == m.shape and out.dtype == m.dtype
        for s in range(3 * C):
            g0 = s - s % C
            want = m[g0]
            for c in range(1, C):
                want = np.maximum(want, m[g0 + c])
            assert np.array_equal(out[s], want)
        h = m.astype(np.float16)  # (the bf16 configuration's masks: the max commutes with the exact widening)
        assert np.array_equal(link_masks(h, C).astype(np.float32), link_masks(h.astype(np.float32), C))
    for C in (1, 3, 5, 6, 7, 0, 9):
        with pytest.raises(ValueError):
            link_masks(np.zeros((max(C, 1) * 2, 257), np.float32), C)
    with pytest.raises(ValueError):
        link_masks(np.zeros((5, 257), np.float32), 2)


def test_recipe_identical_channels_give_the_unlinked_oracle_output_and_one_channel_is_refused():
    from oracle import oracle
    model, C, G, T = model_file('random'), 2, 2, 3
    one = synth_streams(G, T, 5)
    x = np.repeat(one, C, axis=0)  # every group: the same samples in both channels
    got, rep = LinkRecipe(model, G * C, C).process(x)
    assert np.array_equal(got, oracle.Oracle(model, G * C).process(x))
    plain, rep0 = LinkRecipe(model, G * C, C, link=False).process(x)
    assert np.array_equal(got, plain) and np.array_equal(rep.view(np.uint32), rep0.view(np.uint32))
    # different channels: the link changes samples and e_out, never e_in or mask_sum
    y = synth_streams(G * C, T, 6)
    a, ra = LinkRecipe(model, G * C, C).process(y)
    b, rb = LinkRecipe(model, G * C, C, link=False).process(y)
    assert not np.array_equal(a, b)
    assert np.array_equal(ra[..., [0, 2]].view(np.uint32), rb[..., [0, 2]].view(np.uint32)) and (ra[..., 1] >= rb[..., 1]).all()
    for C1 in (1, 3):
        with pytest.raises(ValueError):
            LinkRecipe(model, 6, C1)


def test_recipe_groups_are_independent_of_each_other():
    """the rule never looks outside a group: the recipe on G groups gives, group by group, what the recipe on that group alone gives --
    samples and report rows, with gains and per-frame resets that differ within the groups.  What the lone-group references of
    tests/test_gpu_channel_link_routes.py (packet handles whose groups are out of phase) rest on."""
    model, T = model_file('random'), 3
    for C, G in ((2, 4), (8, 2)):
        B = G * C
        x = [synth_streams(B, T, 7 + k) for k in range(2)]
        gains = np.resize(np.array([0.0, 0.5, 1.0, 0.25, 0.0], np.float32), B)
        rs = np.zeros((B, T), np.uint8)
        rs[1, 1] = rs[B - 1, 2] = rs[C, 0] = 1
        args = [(None, None), (gains, rs)]
        whole = LinkRecipe(model, B, C)
        got = [whole.process(x[k], *args[k]) for k in range(2)]
        for g in range(G):
            rows = slice(g * C, (g + 1) * C)
            alone = LinkRecipe(model, C, C)
            for k in range(2):
                gk, rk = args[k]
                y, rep = alone.process(x[k][rows], None if gk is None else gk[rows], None if rk is None else rk[rows])
                assert np.array_equal(got[k][0][rows], y), (C, g, k)
                assert np.array_equal(got[k][1][rows].view(np.uint32), rep.view(np.uint32)), (C, g, k)
        # (not vacuous: another group's samples would have changed these rows had they been linked across the boundary)
        other = LinkRecipe(model, B, 2 * C if C == 2 else 4).process(x[0])[0]
        assert not np.array_equal(other, got[0][0])


def test_symbols_are_exported_and_declared_and_the_config_struct_did_not_grow(native_library):
    header = open(os.path.join(ROOT, 'include', 'pv_koala_batch.h')).read()
    for path in (native_library, koala_amd.developer_library_path()):
        lib = ctypes.CDLL(path)
        for sym in SYMBOLS:
            assert hasattr(lib, sym), (path, sym)
    for sym in SYMBOLS:
        assert re.search(r'PV_API pv_status_t %s\(' % sym, header), sym
    assert re.search(r'typedef enum \{ PV_KOALA_CHANNEL_LINK_NONE = 0, PV_KOALA_CHANNEL_LINK_MAX = 1 \} pv_koala_channel_link_t;', header)
    assert 'channel_link' not in open(os.path.join(ROOT, 'include', 'pv_koala.h')).read()
    # pv_koala_batch_config_t: the seven int32 members it had, and the Python mirror agrees
    body = re.search(r'typedef struct \{([^}]*)\} pv_koala_batch_config_t;', header).group(1)
    assert len(re.findall(r'\bint32_t\s+\w+;', body)) + len(re.findall(r'pv_koala_\w+_t\s+\w+;', body)) == 7 and 'link' not in body
    assert ctypes.sizeof(BatchConfig) == 28
    lib = ctypes.CDLL(native_library)
    assert lib.pv_koala_batch_set_channel_link(None, 1) == 3 and lib.pv_koala_batch_get_channel_link(None, None) == 3


def test_python_argument_checks_mirror_the_c_refusals():
    # (the argument checks stand in front of the library: nothing is loaded, no handle is made)
    kw = dict(access_key='k', model_path=model_file('random'), device='best', library_path=os.path.join(ROOT, 'no-such-library.so'), max_frames_per_call=1)
    for C in (1, 3, 5, 6, 7):
        with pytest.raises(KoalaInvalidArgumentError, match='2, 4 or 8'):
            KoalaBatch(num_streams=C * 2, channels=C, channel_link='max', **kw)
    for bad in ('min', 'mean', 1, True, ''):
        with pytest.raises(KoalaInvalidArgumentError, match='channel_link'):
            KoalaBatch(num_streams=4, channels=2, channel_link=bad, **kw)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_every_linked_synthesis_form_builds_for_gfx950_without_scratch_at_three_waves(tmp_path):
    """synthesis_link_kernel<kReport, kRecompute, kMaskH, kMaskIn, kResets>: the 14 forms the engine can launch for a linked handle -- the
    nine report forms, and the five plain forms of the stored spectrum (the arm implies kMinGain; a recomputing call without a report runs
    the report form with an empty descriptor: DESIGN.md section 6).  None uses scratch; every multi-frame form stays inside the 168
    registers of three waves per SIMD; the one-frame form with the mask head inside is one workgroup of eight waves per CU by its launch
    bounds, as its plain counterpart.  The partner values come through plain vector loads and 17 v_max_i32."""
    import isa_scan
    src = 'kns_stft.hip'
    out = tmp_path / (src + '.s')
    mk = open(os.path.join(ROOT, 'koala_amd', 'Makefile')).read()
    cxx = re.search(r'^CXXFLAGS\s*=\s*(.*)$', mk, re.M).group(1).split()
    m = re.search(r'^FLAGS_%s\s*=\s*(.*)$' % src.split('.')[0], mk, re.M)
    flags = [f for f in cxx if f not in ('-fPIC',)] + (m.group(1).split() if m else [])
    subprocess.check_call([HIPCC, '--offload-arch=gfx950'] + flags +
                          ['-S', '--cuda-device-only', '-x', 'hip', os.path.join(ROOT, 'koala_amd', 'csrc', src), '-o', str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    assert isa_scan.scan(text) == []
    info = {}
    for name, body in re.findall(r'\.set (\S+)\.has_indirect_call, \d+\n[^\n]*\n; Kernel info:\n((?:;[^\n]*\n)*)', text):
        form = re.search(r'synthesis_link_kernelI((?:Lb[01]E)+)E', name)
        if form:
            bits = tuple(int(b) for b in re.findall(r'Lb([01])E', form.group(1)))
            info[bits] = {k: int(re.search(r'; %s: (\d+)' % k, body).group(1)) for k in ('ScratchSize', 'Occupancy', 'NumVgprs')}
    nine = [(1, 1, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1), (0, 1, 1, 0)]
    forms = [(1,) + f for f in nine] + [(0,) + f for f in nine if not f[0]]
    assert len(forms) == 14 and sorted(info) == sorted(forms), sorted(info)
    for f in forms:
        print(f, info[f])
        assert info[f]['ScratchSize'] == 0, (f, info[f])
        if f[3]:
            assert info[f]['Occupancy'] == 2, (f, info[f])
        else:
            assert info[f]['Occupancy'] >= 3 and info[f]['NumVgprs'] <= 168, (f, info[f])
    for name, body in re.findall(r'^(_Z\w*synthesis_link_kernel\w+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:', text, re.M | re.S):
        assert len(re.findall(r'\bv_max_i32', body)) == 17, name
