"""
The corpus runner (koala_amd/corpus.py) on a real MI355X: 300 utterances of 0.3-20 s through 64 slots of 32-frame calls with per-frame
stream resets, in the three modes; every file against the oracle run on that file alone.
"""
import numpy as np
import pytest

import koala_amd
from conftest import model_file, synth_streams
from gpu_kit import BF16_TOL
from koala_amd import corpus
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def utterances():
    rng = np.random.default_rng(2024)
    lengths = rng.integers(int(0.3 * 16000), 20 * 16000 + 1, 300)
    base = synth_streams(len(lengths), int(np.ceil(lengths.max() / 256)), seed=31)
    return [base[i, :n].copy() for i, n in enumerate(lengths)]


@pytest.fixture(scope='module')
def alone(utterances):
    """(the oracle is causal: one zero-padded batch of all 300 files is each file alone)"""
    model = model_file('random')
    nmax = int(corpus.utterance_frames([len(x) for x in utterances]).max())
    pad = np.zeros((len(utterances), nmax * 256), np.int16)
    for i, x in enumerate(utterances):
        pad[i, :len(x)] = x
    res = {}
    for precision, p in (('fp32', oracle.PREC_FP32), ('bf16', oracle.PREC_BF16)):
        y = oracle.Oracle(model, len(utterances), p).process(pad)
        res[precision] = [y[i, 256:256 + len(x)] for i, x in enumerate(utterances)]
    return res


@pytest.mark.parametrize('mode', ['host', 'async', 'device'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_corpus_equals_each_file_alone(utterances, alone, mode, precision):
    if mode == 'device':
        pytest.importorskip('torch')
    kb = koala_amd.create_batch('key', 64, 32, precision, model_path=model_file('random'))
    got = corpus.enhance_corpus(kb, utterances, 32, mode)
    kb.delete()
    assert len(got) == len(utterances)
    worst = 0
    for i, x in enumerate(utterances):
        assert got[i].shape == x.shape
        d = int(np.abs(got[i].astype(np.int64) - alone[precision][i].astype(np.int64)).max())
        if precision == 'fp32':
            assert d == 0, (i, d)
        worst = max(worst, d)
    assert worst <= BF16_TOL, worst


@pytest.mark.parametrize('asynchronous', [False, True])
def test_file_demo_refill_mode(tmp_path, asynchronous):
    """koala_amd.demo.koala_demo_file --refill: three files through two slots write what the default many-files mode writes."""
    import subprocess
    import sys
    import wave
    from conftest import GOLDEN, ROOT
    env = dict(__import__('os').environ, PYTHONPATH=ROOT)
    model = model_file('adaptive')
    files = [GOLDEN + '/test.wav', GOLDEN + '/noise.wav', GOLDEN + '/test.wav']
    (tmp_path / 'in').mkdir()
    names = []
    for i, f in enumerate(files):  # (distinct names: outputs are named after the inputs)
        p = tmp_path / 'in' / ('f%d.wav' % i)
        p.write_bytes(open(f, 'rb').read())
        names.append(str(p))
    outs = {}
    for mode, extra in (('plain', []), ('refill', ['--refill', '--num_slots', '2'] + (['--asynchronous'] if asynchronous else []))):
        d = tmp_path / mode
        r = subprocess.run([sys.executable, '-m', 'koala_amd.demo.koala_demo_file', '--input_path'] + names +
                           ['--output_dir', str(d), '--model_path', model, '--frames_per_call', '16'] + extra,
                           capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0 and 'Real time factor' in r.stdout, r.stderr
        outs[mode] = []
        for i in range(len(files)):
            with wave.open(str(d / ('f%d.wav' % i))) as w:
                outs[mode].append(np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16))
    for a, b in zip(outs['plain'], outs['refill']):
        assert len(a) == len(b) and np.array_equal(a, b)
