"""
The layer-B recurrent launches of stages 0 and 1 that carry the stage's narrow head (kns_gru.hip, gru_resident8_kernel<true>
and <true, true>) publish no hidden sequence: the head was that sequence's only reader.  Checked here on the resident route at a
small batch (developer library, KOALA_AMD_WAVE_MT=0): fused heads against KOALA_AMD_NO_HEAD_FUSE=1 -- the independent arm, the head
as its own GEMM over the published sequence -- and against KOALA_AMD_DEBUG_TAPS=1, which keeps every intermediate; all exactly.

32 streams (two m-tiles), T = 2, 5 and 8: an odd and an even count of LDS ping-pong swaps, the rewrite of frame 0's slot at t = 1 and
the head behind the loop.  Per shape: two consecutive calls (the carried state), a call with one per-frame reset in mid-call in the
first m-tile only (the reset form, with and without a reset in the m-tile), then the readers that follow a multi-frame call on the
same handle: a one-frame call (its layers read the hidden-sequence buffer) and an export / reset / import round trip.

debug_read has no tap for a hidden sequence (its codes: features, spectrum, mask, hidden state, embedding, stamps, route and the
count of head-carrying launches); what it returns of layer B is the hidden state (tap 'hidden': every layer's last hidden vector)
and, downstream of both narrow heads, the mask (tap 'mask'): both are compared in every arm, 'features' where they are kept.  The
developer build's tap 'head_launches' shows that the fused arm did launch the head-carrying form, and the other arms did not.

Each arm runs in a fresh child process: the engine reads its switches when a handle is created.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import koala_amd
from gpu_kit import ROUTE_CHUNKED, ROUTE_RESETS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (2, 5, 8)
B = 32

_ARM_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch  # noqa: F401  (first: see conftest)
import koala_amd
from koala_amd.workload import synth_streams
B, out = %(B)d, {}
for T in %(shapes)r:
    x = synth_streams(B, 3 * T + 2, seed=40 + T)
    part = lambda f0, n: np.ascontiguousarray(x[:, f0 * 256:(f0 + n) * 256])
    kb = koala_amd.create_batch('key', B, T, 'bf16', model_path=%(model)r, library_path=%(lib)r)
    for c in range(2):  # two consecutive calls: the second starts from the state the first left
        out['pcm_%%d_%%d' %% (T, c)] = kb.process(part(c * T, T))
        out['route_%%d_%%d' %% (T, c)] = kb.debug_read('route', T)
        out['heads_%%d_%%d' %% (T, c)] = kb.debug_read('head_launches', T)
        out['hidden_%%d_%%d' %% (T, c)] = kb.debug_read('hidden', T)
        out['mask_%%d_%%d' %% (T, c)] = kb.debug_read('mask', T)
    if %(features)r:
        out['features_%%d' %% T] = kb.debug_read('features', T)
    m = np.zeros((B, T), np.uint8)
    m[:16:3, T // 2] = 1  # one reset in mid-call, first m-tile only
    out['pcm_%%d_resets' %% T] = kb.process_resets(part(2 * T, T), m)
    out['route_%%d_resets' %% T] = kb.debug_read('route', T)
    out['heads_%%d_resets' %% T] = kb.debug_read('head_launches', T)
    out['hidden_%%d_resets' %% T] = kb.debug_read('hidden', T)
    out['pcm_%%d_one' %% T] = kb.process(part(3 * T, 1))  # a one-frame call behind the multi-frame ones
    blobs = kb.export_state()
    kb.reset()
    kb.import_state(blobs)
    out['pcm_%%d_imported' %% T] = kb.process(part(3 * T + 1, 1))
    kb.delete()
np.savez(%(npz)r, **out)
'''


@pytest.fixture(scope='module')
def arms(random_model, tmp_path_factory):
    d = tmp_path_factory.mktemp('head_launch')
    got = {}
    for arm, switches in (('fused', {}), ('no_head_fuse', {'KOALA_AMD_NO_HEAD_FUSE': '1'}), ('debug_taps', {'KOALA_AMD_DEBUG_TAPS': '1'})):
        npz = str(d / (arm + '.npz'))
        script = _ARM_SCRIPT % {'root': ROOT, 'B': B, 'shapes': SHAPES, 'model': random_model, 'lib': koala_amd.developer_library_path(),
                                'features': arm == 'debug_taps', 'npz': npz}
        env = dict(os.environ, KOALA_AMD_WAVE_MT='0', **switches)
        for k in ('KOALA_AMD_NO_HEAD_FUSE', 'KOALA_AMD_DEBUG_TAPS'):
            if k not in switches:
                env.pop(k, None)
        r = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (arm, r.stderr[-2000:])
        got[arm] = dict(np.load(npz))
    return got


def test_every_arm_took_the_resident_route(arms):
    """... and the fused arm launched the head-carrying form for stages 0 and 1, the other two arms never (the developer build counts
    the recurrent launches of a call that were handed their stage's head)."""
    for arm, a in arms.items():
        for T in SHAPES:
            want = 2 if arm == 'fused' else 0
            assert [int(a['heads_%d_%s' % (T, c)][0]) for c in ('0', '1', 'resets')] == [want] * 3, (arm, T)
            assert [int(a['route_%d_%d' % (T, c)][0]) for c in range(2)] == [ROUTE_CHUNKED] * 2, (arm, T)
            assert int(a['route_%d_resets' % T][0]) == ROUTE_RESETS, (arm, T)
            assert a['pcm_%d_0' % T].any() and a['pcm_%d_1' % T].any(), (arm, T)


@pytest.mark.parametrize('other', ['no_head_fuse', 'debug_taps'])
@pytest.mark.parametrize('T', SHAPES)
def test_fused_heads_give_the_pcm_of_the_published_sequence(arms, other, T):
    """... over two consecutive calls, a call with a per-frame reset, and the one-frame call and the state round trip that follow."""
    for what in ('0', '1', 'resets', 'one', 'imported'):
        k = 'pcm_%d_%s' % (T, what)
        assert np.array_equal(arms['fused'][k], arms[other][k]), (k, int(np.abs(arms['fused'][k].astype(int) - arms[other][k]).max()))


@pytest.mark.parametrize('T', SHAPES)
def test_debug_taps_still_return_what_layer_b_left(arms, T):
    """The publishing path where it is needed: with the taps on, the heads are GEMMs over the published sequences, and what debug_read
    returns behind them -- every layer's hidden vector, the mask -- is what the fused launches computed, bit for bit."""
    taps, fused, plain = arms['debug_taps'], arms['fused'], arms['no_head_fuse']
    for what in ('0', '1', 'resets'):
        k = 'hidden_%d_%s' % (T, what)
        assert taps[k].shape == (8, B, 271) and np.isfinite(taps[k]).all() and np.abs(taps[k][1::2]).max() > 0, k
        assert np.array_equal(taps[k], fused[k]) and np.array_equal(taps[k], plain[k]), k
    for c in range(2):
        k = 'mask_%d_%d' % (T, c)
        assert taps[k].shape == (T, B, 257) and np.abs(taps[k]).max() > 0, k
        assert np.array_equal(taps[k], fused[k]) and np.array_equal(taps[k], plain[k]), k
    assert taps['features_%d' % T].shape == (T, B, 257) and np.isfinite(taps['features_%d' % T]).all()
