"""
CPU figures for profiles/r11_sample_rate.txt, from the numpy recipe (tests/sample_rate_recipe.py) and the oracle:

 (1) the default model's steady-state suppression of the tuning-set noises (tests/test_holdout.py: white / pink / rumble at 0.01 and 0.03 RMS)
     on a handle at 8 kHz -- the 16 kHz noise taken to 8 kHz by the spec's decimator, then through in-stage -> oracle -> out-stage -- beside
     the 16 kHz figure of the same noise.  A figure to quote, not a bar.
 (2) the share of samples by which the jittered bf16 oracle (oracle.set_jitter) misses the plain one by more than 1 LSB through the recipe
     on the inputs of tests/test_gpu_sample_rate.py (tests/sample_rate_cases.py) at 8, 32 and 48 kHz: a quarter of what that test allows
     the engine.

    python tools/sample_rate_figures.py        (prints; paste into sections 1 and 2 of the profile)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    import conftest
    import sample_rate_cases as g
    import sample_rate_recipe as srr
    import test_holdout as h
    from oracle import oracle
    model = conftest.model_file('adaptive')
    n = len(conftest.load_wav('test.wav')) // 256 * 256
    print('(1) default model, fp32 oracle, steady-state suppression in dB (from 0.5 s on)')
    for kind in ('white', 'pink', 'rumble'):
        for level in (0.01, 0.03):
            x = h.synth_noise(kind, n, np.random.default_rng(777))
            noise = np.clip(np.rint(x / np.std(x) * level * 32768), -32768, 32767).astype(np.int16).reshape(1, -1)
            y16 = oracle.Oracle(model, 1).process(noise)
            d16 = 20 * np.log10(h.rms(noise[0, 8000:]) / max(h.rms(y16[0, 8000 + 256:]), 1e-9))
            x8 = srr.Stage(1, 2, 1, 2).run(noise)  # (the out-stage of an 8 kHz handle: down 2)
            y8 = srr.Recipe(model, 1, 'fp32', 8000).process(x8)
            d8 = 20 * np.log10(h.rms(x8[0, 4000:]) / max(h.rms(y8[0, 4000 + srr.delay_sample(8000):]), 1e-9))
            print('    %-6s %.2f RMS   16 kHz %5.1f dB   8 kHz handle %5.1f dB' % (kind, level, d16, d8))
    print('(2) bf16, random model: share of samples the jittered oracle (seed 1) moves by more than 1 LSB through the recipe')
    for rate in (8000, 32000, 48000):
        want = np.concatenate(g.expected('random', 'bf16', rate)[1], axis=1).astype(np.int32)
        jit = np.concatenate(g.expected('random', 'bf16', rate, 1)[1], axis=1).astype(np.int32)
        d = np.abs(jit - want)
        print('    %5d Hz   share > 1 LSB %.3e   max %d LSB   (the engine may miss %.3e; its bound on the distance: %d LSB)' %
              (rate, float((d > 1).mean()), int(d.max()), 4 * float((d > 1).mean()), g.bf16_bound(rate)))


if __name__ == '__main__':
    main()
