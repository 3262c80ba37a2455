"""
What tests/test_gpu_edge_inputs.py rests on, checked without a GPU (tests/edge_recipe.py): that the (model, input) pairs the bf16 engine is
held to the suite's bars on are pairs where two valid bf16 implementations agree; that the fixed-mask models do drive the synthesis into the
rails with a mask that is not 1 everywhere, and that the oracle sits on the rail there; and that silence stays silence.
"""
import numpy as np
import pytest

from edge_recipe import (BF16_ASSERTED, FIXED, HORIZON, MODELS, NAMES, PASSBANDS, SILENCE, asserted_rows, beyond, edge_streams, jitter_figures,
                         model_path, unclamped)
from oracle import oracle


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp('edge_models')
    return {m: model_path(d, m) for m in MODELS}


def test_the_asserted_set_is_the_issues():
    """every input on the four constant-mask models (that part may never shrink), all but full-range noise on the default model, and the
    three quiet inputs on the random-weight models"""
    for m in FIXED:
        assert asserted_rows(m) == list(range(len(NAMES)))
    assert [NAMES[r] for r in range(len(NAMES)) if r not in asserted_rows('adaptive')] == ['noise']
    for m in ('random', 'random5'):
        assert [NAMES[r] for r in asserted_rows(m)] == ['impulse', 'dither', 'silence']
    assert len(BF16_ASSERTED) == 4 * 12 + 11 + 2 * 3


@pytest.mark.parametrize('model', MODELS)
def test_the_asserted_set_is_honest(models, model):
    """On every asserted pair the jittered bf16 oracle (seeds 1 .. 8: a second valid bf16 implementation) stays within 1 LSB of the plain one
    over the longest horizon the GPU module uses.  A condition for being listed, not a measurement: a pair that misses it leaves the list."""
    x, names = edge_streams(HORIZON)
    worst, within = jitter_figures(models[model], x)
    for r, name in enumerate(names):
        print('%-9s %-14s jitter: max %2d LSB, %.4f within 1%s' % (model, name, worst[r], within[r], '' if (model, name) in BF16_ASSERTED else '  (recorded only)'))
    rows = asserted_rows(model)
    assert worst[rows].max() <= 1, [(names[r], int(worst[r])) for r in rows if worst[r] > 1]
    if model in FIXED:  # a constant mask: nothing the jitter touches reaches a sample
        assert worst.max() == 0, worst.tolist()


@pytest.mark.parametrize('model,row', [('highpass8', 'noise'), ('lowpass64', 'square')])
def test_fixed_mask_models_reach_the_rails_with_a_real_mask(models, model, row):
    """The unrounded output of the brick-wall filter (float64 numpy, no code of the oracle's) leaves the int16 range on both sides, the fp32
    oracle sits on the matching rail at each such sample, and away from the rails the oracle is the numpy statement rounded (the fp32-vs-numpy
    bar of DESIGN.md section 5: within 1 LSB, >= 99 % identical)."""
    x, names = edge_streams(24)
    r = names.index(row)
    u = unclamped(x[r], PASSBANDS[model])[0]
    above, below = beyond(u)
    y = oracle.Oracle(models[model], 1).process(x[r:r + 1])[0]
    delayed_in = np.concatenate([np.zeros(256, np.int16), x[r, :-256]])
    print(model, row, 'beyond the rails: %d above, %d below; of those not on that rail in the delayed input: %d' %
          (above.sum(), below.sum(), (above & (delayed_in != 32767)).sum() + (below & (delayed_in != -32768)).sum()))
    assert above.sum() + below.sum() >= 32 and above.any() and below.any()
    assert (y[above] == 32767).all() and (y[below] == -32768).all()
    inside = np.abs(u) < 32000
    want = np.sign(u) * np.floor(np.abs(u) + 0.5)
    d = np.abs(y[inside] - want[inside])
    print(model, row, 'inside: max %d LSB, identical %.4f of %d' % (d.max(), (d == 0).mean(), d.size))
    assert inside.sum() > 1000 and d.max() <= 1 and (d == 0).mean() >= 0.99
    # the filter is not the identity here: the output differs from the delayed input
    assert (y != delayed_in).mean() > 0.5


@pytest.mark.parametrize('precision', [oracle.PREC_FP32, oracle.PREC_BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('model', MODELS)
def test_silence_is_silence(models, model, precision):
    """power 0 into the feature logarithm: finite features, and zeros out -- for every model of the suite, in both precisions"""
    x, _ = edge_streams(8)
    assert not x[SILENCE].any()
    assert not oracle.Oracle(models[model], 1, precision).process(x[SILENCE:SILENCE + 1]).any()
    o = oracle.Oracle(models[model], 1, precision)
    for t in range(3):
        y, tp = o.process_tap(x[SILENCE, t * 256:(t + 1) * 256])
        assert np.isfinite(tp['features']).all() and not y.any() and not tp['spectrum'].any(), t
