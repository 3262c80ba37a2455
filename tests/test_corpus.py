"""
The corpus planner and duration-balanced sharding (koala_amd/corpus.py, koala_amd/sharding.py) on the CPU, and the meaning of calls with
per-frame stream resets (include/pv_koala_batch.h, pv_koala_batch_process_chunk_resets) pinned on the oracle: a plan executed as calls
cut at their reset frames gives every file exactly what the file alone gives.
"""
import numpy as np
import pytest

from conftest import model_file, synth_streams
from koala_amd import corpus, sharding
from oracle import oracle


def check_plan(lengths, S, T, plan):
    nf = corpus.utterance_frames(lengths)
    src, reset = plan.src, plan.reset
    C = plan.num_calls
    assert src.shape == reset.shape == (C, S, T)
    timeline = src.transpose(1, 0, 2).reshape(S, C * T)  # per slot, frame by frame
    rtl = reset.transpose(1, 0, 2).reshape(S, C * T)
    F = int(nf.sum())
    assert plan.zero_frame == F
    seen = np.zeros(F + 1, np.int64)
    np.add.at(seen, timeline.reshape(-1), 1)
    assert (seen[:F] == 1).all()  # every frame of every utterance exactly once
    for u in range(len(lengths)):
        s, t0 = int(plan.slot[u]), int(plan.start[u])
        assert (timeline[s, t0:t0 + nf[u]] == plan.offsets[u] + np.arange(nf[u])).all()  # in order, in one slot
    starts = set(zip(plan.slot.tolist(), plan.start.tolist()))
    got = set(zip(*[a.tolist() for a in np.nonzero(rtl)]))
    assert got == starts  # the mask: exactly at each utterance's first frame
    # idle frames read the zero frame, and only after the slot's last utterance
    for s in range(S):
        idle = np.nonzero(timeline[s] == F)[0]
        if idle.size:
            assert (timeline[s, idle[0]:] == F).all()


@pytest.mark.parametrize('N,S,T,lo,hi,seed', [(40, 8, 16, 1, 9000, 0),      # more utterances than slots
                                              (25, 4, 32, 1, 700, 1),       # many utterances shorter than one call: several per slot per call
                                              (3, 8, 16, 0, 5000, 2),       # fewer utterances than slots, an empty one
                                              (200, 16, 64, 100, 60000, 3)])
def test_plan_invariants(N, S, T, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(lo, hi, N)
    plan = corpus.plan_corpus(lengths, S, T)
    check_plan(lengths, S, T, plan)
    if N > S:  # longest first: the utterances that start last are the shortest
        order = np.argsort(plan.start, kind='stable')
        nf = corpus.utterance_frames(lengths)
        assert nf[order[-1]] <= nf[order[0]]
    # several utterances in one slot inside one call
    if (lengths < 256 * T).sum() > S:
        assert (plan.reset.sum(axis=2) >= 2).any()


def test_plan_given_order_and_bad_args():
    plan = corpus.plan_corpus([256, 512, 10], 2, 4, order='given')
    check_plan([256, 512, 10], 2, 4, plan)
    assert plan.slot.tolist() == [0, 1, 0] and plan.start.tolist() == [0, 0, 2]
    with pytest.raises(ValueError):
        corpus.plan_corpus([1], 0, 4)
    with pytest.raises(ValueError):
        corpus.plan_corpus([1], 2, 4, order='random')


def test_process_split_cuts_at_reset_frames():
    calls = []

    class Rec:
        def reset(self, m):
            calls.append(('reset', m.tolist()))

        def process(self, x):
            calls.append(('process', x.shape[1] // 256))
            return x

    r = np.zeros((2, 6), np.uint8)
    r[0, 0] = r[1, 2] = r[0, 3] = r[1, 3] = 1
    x = np.arange(2 * 6 * 256, dtype=np.int16).reshape(2, -1)
    assert np.array_equal(corpus.process_split(Rec(), x, r), x)
    assert calls == [('reset', [1, 0]), ('process', 2), ('reset', [0, 1]), ('process', 1), ('reset', [1, 1]), ('process', 3)]


def run_plan_on_oracle(model, signals, S, T, precision=oracle.PREC_FP32):
    plan = corpus.plan_corpus([len(x) for x in signals], S, T)
    table = corpus.corpus_table(signals, plan)
    out = np.zeros_like(table)
    o = oracle.Oracle(model, S, precision)
    for c in range(plan.num_calls):
        y = corpus.process_split(o, table[plan.src[c]].reshape(S, T * 256), plan.reset[c])
        out[plan.src[c]] = y.reshape(S, T, 256)
    return corpus.trim(out, signals, plan, o.delay_sample), plan


@pytest.mark.parametrize('S,T', [(4, 8), (3, 5)])
def test_plan_on_oracle_equals_each_file_alone(S, T):
    model = model_file('random', 1234)
    rng = np.random.default_rng(7)
    lengths = np.concatenate([rng.integers(1, 2600, 7), rng.integers(1, 500, 6)])  # (the short ones: back to back inside one call)
    base = synth_streams(len(lengths), int(np.ceil(lengths.max() / 256)) + 1, seed=5)
    signals = [base[i, :n].copy() for i, n in enumerate(lengths)]
    got, plan = run_plan_on_oracle(model, signals, S, T)
    assert (plan.reset.sum(axis=2) >= 2).any()  # short utterances share a call inside one slot
    assert plan.reset[1:, :, 1:].any()  # resets inside calls, not only at their first frame
    # each file alone (the oracle is causal: one zero-padded batch of all files is each file alone)
    nmax = int(corpus.utterance_frames(lengths).max())
    pad = np.zeros((len(signals), nmax * 256), np.int16)
    for i, x in enumerate(signals):
        pad[i, :len(x)] = x
    ref = oracle.Oracle(model, len(signals)).process(pad)
    for i, x in enumerate(signals):
        assert np.array_equal(got[i], ref[i, 256:256 + len(x)]), i


def test_balanced_assignment_within_two_percent():
    rng = np.random.default_rng(11)
    d = np.clip(rng.lognormal(np.log(6.0), 0.8, 20000), 1.0, 60.0)
    for ws in (2, 8):
        ranks = sharding.balanced_assignment(d, ws)
        assert sorted(i for r in ranks for i in r) == list(range(d.size))
        loads = np.array([d[r].sum() for r in ranks])
        assert loads.max() <= 1.02 * loads.mean() and loads.min() >= 0.98 * loads.mean(), loads
        assert ranks == sharding.balanced_assignment(d.copy(), ws)  # deterministic


def test_balanced_assignment_edges():
    assert sharding.balanced_assignment([3.0, 1.0], 4) == [[0], [1], [], []]
    assert sharding.balanced_assignment([], 3) == [[], [], []]
    r = sharding.balanced_assignment([0.0, 0.0, 0.0, 5.0], 2)
    assert sorted(i for x in r for i in x) == [0, 1, 2, 3] and [3] in r
    with pytest.raises(ValueError):
        sharding.balanced_assignment([1.0], 0)
    with pytest.raises(ValueError):
        sharding.balanced_assignment([-1.0], 2)
