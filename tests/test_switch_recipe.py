"""
The switch model on the CPU (tests/switch_recipe.py): the bf16 oracle, its jittered self and the fp32 oracle against the integer reference, the
margins the recipe's derivation promises, that the dynamics are alive, and that the recipe notices the defects it exists for.

Recorded, not asserted:
  * fp32 does not saturate to exactly 0: kns_sigmoid of a large negative argument is 1 / (1 + kns_exp(88)) = 6.05e-39 (kns_exp clamps at 88),
    so the fp32 oracle's mask is {6.05e-39, 1} where the reference's is {0, 1}.  Its hidden state and its samples ARE the reference's, and are
    asserted; the fp32 engine is held to its own oracle (tests/test_gpu_switch_model.py).
  * the jitter probe (kns_oracle_set_jitter) moves the last bit of every transcendental result that is neither 0 nor inf -- an exact 1.0
    included, which no reciprocal of exactly 1.0 can miss.  Under jitter r, z and q are therefore {0, 1 +- 2^-24 ...}: the mask (fp16), the
    fed-forward heads (bf16) and the samples stay bit for bit the plain oracle's, which is asserted; the float32 hidden state rounds to the
    plain one and drifts from it by at most 2^-21 per frame, which is asserted in that form.
  * the share of single sign flips the recipe notices: printed by test_share_of_single_sign_flips_that_are_noticed, figures in DESIGN.md
    section 5.
"""
import numpy as np
import pytest

import switch_recipe as sr
from koala_amd import params
from oracle import oracle

H, BINS = sr.H, sr.BINS
SHORT = 24  # frames of the runs that are repeated per mutation


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp('switch_models')
    return {(seed, taps): sr.model_path(d, seed, taps) for seed in sr.SEEDS for taps in (1,)} | {(sr.SEEDS[0], 5): sr.model_path(d, sr.SEEDS[0], 5)}


def oracle_run(model, x, precision):
    """every stream frame by frame through Oracle.process_tap -> pcm [R, n], mask [T, R, 257], hidden float32 [T, 8, R, 271]"""
    R, T = x.shape[0], x.shape[1] // 256
    o = oracle.Oracle(model, R, oracle.PREC_BF16 if precision == 'bf16' else oracle.PREC_FP32)
    pcm, mask, hidden = np.empty_like(x), np.empty((T, R, BINS), np.float32), np.empty((T, 8, R, H), np.float32)
    for b in range(R):
        for t in range(T):
            pcm[b, t * 256:(t + 1) * 256], tap = o.process_tap(x[b, t * 256:(t + 1) * 256], b)
            mask[t, b], hidden[t, :, b] = tap['mask'], tap['hidden']
    return pcm, mask, hidden


_ref, _plain = {}, {}


def reference(models, seed, taps, precision):
    key = (seed, taps, precision)
    if key not in _ref:
        r = sr.Reference(sr.Circuit(seed, taps), models[(seed, taps)], sr.ROWS, precision)
        _ref[key] = (r, r.process(sr.switch_streams()))
    return _ref[key]


def plain(models, seed, taps, precision):
    key = (seed, taps, precision)
    if key not in _plain:
        _plain[key] = oracle_run(models[(seed, taps)], sr.switch_streams(), precision)
    return _plain[key]


MODELS = [(seed, 1) for seed in sr.SEEDS] + [(sr.SEEDS[0], 5)]


# ---------------------------------------------------------------------------------------------------- 1, 3. the oracles == the reference

@pytest.mark.parametrize('seed,taps', MODELS)
def test_bf16_oracle_equals_the_integer_reference(models, seed, taps):
    want = reference(models, seed, taps, 'bf16')[1]
    pcm, mask, hidden = plain(models, seed, taps, 'bf16')
    assert sr.first_difference(hidden, want['hidden'].astype(np.float32), ('frame', 'layer', 'stream', 'unit')) is None
    assert sr.first_difference(mask.view(np.uint32), want['mask'].view(np.uint32), ('frame', 'stream', 'bin')) is None
    assert sr.first_difference(pcm, want['pcm'], ('stream', 'sample')) is None


@pytest.mark.parametrize('seed,taps', MODELS)
def test_fp32_oracle_has_the_references_hidden_state_and_samples(models, seed, taps):
    """... and a mask of {6e-39, 1}: the fp32 polynomials do not saturate to exactly 0 (module docstring)"""
    want = reference(models, seed, taps, 'fp32')[1]
    pcm, mask, hidden = plain(models, seed, taps, 'fp32')
    assert sr.first_difference(hidden, want['hidden'].astype(np.float32), ('frame', 'layer', 'stream', 'unit')) is None
    assert sr.first_difference(pcm, want['pcm'], ('stream', 'sample')) is None
    low = mask[want['mask'] == 0]
    print('fp32 mask where the reference has 0: %r .. %r; exactly 0: %s' % (low.min(), low.max(), bool((low == 0).all())))
    assert (mask[want['mask'] == 1] == 1).all() and (low >= 0).all() and (low < 1e-37).all()


# ---------------------------------------------------------------------------------------------------- 2. the jittered oracle

@pytest.mark.parametrize('seed', sr.SEEDS)
def test_jittered_bf16_oracle_equals_the_plain_one(models, seed):
    """two valid bf16 implementations cannot differ on this model: eight jitter seeds"""
    x = sr.switch_streams(SHORT)
    pcm, mask, hidden = (a[:SHORT] if a.ndim > 2 else a[:, :SHORT * 256] for a in plain(models, seed, 1, 'bf16'))
    try:
        for j in range(1, 9):
            oracle.set_jitter(j)
            jp, jm, jh = oracle_run(models[(seed, 1)], x, 'bf16')
            assert sr.first_difference(jm.view(np.uint32), mask.view(np.uint32), ('frame', 'stream', 'bin')) is None, j
            assert sr.first_difference(jp, pcm, ('stream', 'sample')) is None, j
            assert sr.first_difference(np.rint(jh), hidden, ('frame', 'layer', 'stream', 'unit')) is None, j
            # the probe moves an exact 1.0 (module docstring): z and q within 2^-23 of 1, |h - n| <= 2, so a frame adds at most 2^-21
            assert np.abs(jh - hidden).max() <= SHORT * 2.0 ** -21, j
    finally:
        oracle.set_jitter(0)


# ---------------------------------------------------------------------------------------------------- 4. margins

def test_scaled_weights_are_exact_bf16_values():
    """one float32 multiplication by the engine's constants, then bf16: 512 for every dense recurrent weight, 1024 for an input unit's"""
    rz, n = -sr.LOG2E, np.float32(2.88539008177792681)
    assert sr.round_bf16(sr.G * rz) == -512 and sr.round_bf16(np.float32(sr.G / 2) * n) == 512
    assert sr.round_bf16(sr.GF * rz) == -1024 and sr.round_bf16(np.float32(sr.GF / 2) * n) == 1024
    assert sr.round_bf16(sr.GH) == sr.GH
    t = sr.Circuit(1).tensors()
    for name, a in t.items():  # the file holds what the circuit says: integer multiples of U (GH / 2 in the heads), a single 1 per input unit
        if name[1].isdigit() and 'w_ih_a' not in name:
            q = a / (sr.GH / 2 if 'head' in name else sr.U)
            assert np.array_equal(q, np.rint(q)), name
    assert (t['w_in'].sum(0) <= 1).all() and t['w_in'].sum() == sr.F


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
@pytest.mark.parametrize('seed,taps', MODELS)
def test_margins(models, seed, taps, precision):
    r = reference(models, seed, taps, precision)[0]
    print('seed %d taps %d %s: min |pre| %.0f (saturation %.0f), max |gi| %.0f, min |f - theta| %.4f' % (seed, taps, precision, r.min_pre, sr.SATURATION,
                                                                                                       r.max_gi, r.min_gap))
    assert r.min_pre >= sr.MARGIN == 2 * sr.SATURATION
    assert r.max_gi < sr.FP16_MAX
    assert r.min_gap >= sr.MARGIN / 1024.0


def test_every_bin_of_every_frame_keeps_the_feature_gap(models):
    """all 257 bins, both precisions, not only the bins some model reads; and 1024 |f - theta| stays inside fp16"""
    x = sr.switch_streams()
    assert sr.feature_gap(x, models[(sr.SEEDS[0], 1)]) >= sr.FEATURE_GAP
    feat = sr.Analysis(models[(sr.SEEDS[0], 1)], sr.ROWS, 'fp32').process(x)[1]
    assert 1024.0 * max(np.abs(feat - sr.THETA).max(), np.abs(feat - sr.THETA_Z).max()) < sr.FP16_MAX
    assert 1024.0 * (feat - sr.THETA_Z).min() >= sr.MARGIN
    assert len({x[r].tobytes() for r in range(sr.ROWS)}) == sr.ROWS


# ---------------------------------------------------------------------------------------------------- 5. alive

@pytest.mark.parametrize('seed,taps', MODELS)
def test_dynamics_are_alive(models, seed, taps):
    r, want = reference(models, seed, taps, 'bf16')
    hid, mask = want['hidden'], want['mask']
    for l in range(8):
        both = ((hid[:, l] == 1).any(axis=(0, 1)) & (hid[:, l] == -1).any(axis=(0, 1)))
        assert both.mean() > 0.5, (l, float(both.mean()))  # (an input unit only ever takes the sign its n gate gives it)
    assert r.z_seen.all()
    assert not (mask == mask[0, 0]).all(axis=(0, 1)).any()  # no bin is constant
    runs = hid.transpose(2, 0, 1, 3).reshape(sr.ROWS, -1)
    assert len({row.tobytes() for row in runs}) == sr.ROWS  # every stream its own
    last = {row.tobytes() for row in hid[-1].transpose(1, 0, 2).reshape(sr.ROWS, -1)}
    print('seed %d taps %d: %d distinct states behind the last frame' % (seed, taps, len(last)))


# ---------------------------------------------------------------------------------------------------- 6. mutations

def weights(t):
    return [n for n in t if n.startswith('s') and '.w_' in n]


def result(tmp_path, t):
    path = str(tmp_path / 'mutant.kns')
    params.write_params(path, t)
    return oracle.Oracle(path, sr.ROWS, oracle.PREC_BF16).process_with_mask(sr.switch_streams(SHORT))


def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def swapped(a, axis, width):
    """the first two blocks of `width` along `axis` that differ, swapped (None: no such pair)"""
    a = np.moveaxis(a.copy(), axis, 0)
    nblk = a.shape[0] // width
    for i in range(nblk):
        for j in range(i + 1, nblk):
            bi, bj = a[i * width:(i + 1) * width].copy(), a[j * width:(j + 1) * width].copy()
            if not np.array_equal(bi, bj):
                a[i * width:(i + 1) * width], a[j * width:(j + 1) * width] = bj, bi
                return np.moveaxis(a, 0, axis)
    return None


@pytest.fixture(scope='module')
def base(models, tmp_path_factory):
    t = sr.Circuit(sr.SEEDS[0]).tensors()
    return t, result(tmp_path_factory.mktemp('base'), t)


@pytest.mark.parametrize('what', ['k-blocks', 'n-tiles'])
def test_swapped_blocks_are_noticed_in_every_matrix(base, tmp_path, what):
    t, want = base
    for name in ['w_in'] + weights(t):
        m = swapped(t[name], 0, 32) if what == 'k-blocks' else swapped(t[name], 1, 16)
        if m is None:
            assert what == 'n-tiles' and t[name].shape[1] < 32, name  # (heads of 1 and 5 columns have no second tile)
            continue
        assert differs(result(tmp_path, dict(t, **{name: m})), want), (what, name)


def test_a_zeroed_recurrent_bias_is_noticed(base, tmp_path):
    t, want = base
    for name, unit in (('s0.b_hh_a', 70), ('s1.b_hh_b', 5), ('s3.b_hh_b', 260)):
        b = t[name].copy()
        b[[unit, H + unit, 2 * H + unit]] = 0
        assert differs(result(tmp_path, dict(t, **{name: b})), want), name


def test_a_permuted_unit_of_tile_16_is_noticed(base, tmp_path):
    t, want = base
    for s in range(4):
        for layer in 'ab':
            name = 's%d.w_hh_%s' % (s, layer)
            w = t[name].copy()
            a, b = 256 + (3 * s + 7) % 15, 70 + s
            for g in range(3):
                w[:, [g * H + a, g * H + b]] = w[:, [g * H + b, g * H + a]]
            assert differs(result(tmp_path, dict(t, **{name: w})), want), name
    for s in range(4):  # ... and as a row of the head
        w = t['s%d.w_head' % s].copy()
        other = next(b for b in range(256) if not np.array_equal(w[b], w[256 + s]))
        w[[256 + s, other]] = w[[other, 256 + s]]
        assert differs(result(tmp_path, dict(t, **{'s%d.w_head' % s: w})), want), s


def test_a_moved_head_column_behind_the_features_is_noticed(base, tmp_path):
    """the y rows of stages 2 and 3 (1 and 5 values: the columns 257 ... of the feature block)"""
    t, want = base
    w = t['s1.w_ih_a'].copy()
    w[[0, 1]] = w[[1, 0]]  # the one y row <-> the first embedding row
    assert differs(result(tmp_path, dict(t, **{'s1.w_ih_a': w})), want)
    w = t['s2.w_ih_a'].copy()
    w[:5] = np.roll(w[:5], 1, axis=0)
    assert differs(result(tmp_path, dict(t, **{'s2.w_ih_a': w})), want)


# ---------------------------------------------------------------------------------------------------- 7. single sign flips

def test_share_of_single_sign_flips_that_are_noticed(base, tmp_path):
    """recorded, not asserted: one weight's sign flipped at six positions of every matrix -- two anywhere, two in a column of unit tile 16
    (units 256-270), two in the last rows (k >= 256) -- over 16 streams x 24 frames"""
    t, want = base
    rng = np.random.default_rng(5)
    tried, noticed, missed = 0, 0, []
    for name in weights(t):
        w = t[name]
        rows, cols = np.nonzero(w)
        tile16 = [i for i in range(len(rows)) if (cols[i] % H >= 256 if w.shape[1] == 3 * H else cols[i] >= 256)]
        last = [i for i in range(len(rows)) if rows[i] >= w.shape[0] - 15]
        picks = list(rng.choice(len(rows), 2)) + (list(rng.choice(tile16, 2)) if tile16 else []) + (list(rng.choice(last, 2)) if last else [])
        for i in picks:
            m = w.copy()
            m[rows[i], cols[i]] = -m[rows[i], cols[i]]
            hit = differs(result(tmp_path, dict(t, **{name: m})), want)
            tried, noticed = tried + 1, noticed + hit
            if not hit:
                missed.append((name, int(rows[i]), int(cols[i])))
    print('single sign flips noticed: %d of %d (%.1f %%); missed: %s' % (noticed, tried, 100.0 * noticed / tried, missed))
