"""
The bf16 bars of tests/test_gpu_frame_report.py, measured on the CPU: every bf16 input of that module (its bf16_cases()) goes through the
numpy recipe of the frame report twice -- on the plain bf16 oracle and on the jittered one (oracle.set_jitter: a second valid bf16
implementation) -- and the largest distance between the two is printed: e_out relative, mask_sum / 257 absolute.  The test's bars are 4 x
these values (profiles/r10_frame_report.txt).  e_in must not move at all: the spectrum does not depend on the mask network.

    python tools/frame_report_bars.py [--seeds 1 2 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
    a = ap.parse_args()
    import conftest
    import test_gpu_frame_report as t
    from oracle import oracle
    cases = t.bf16_cases(conftest.model_file('random', 1234))
    worst_e = worst_m = 0.0
    for name, thunk in cases.items():
        oracle.set_jitter(0)
        plain = thunk()
        for seed in a.seeds:
            oracle.set_jitter(seed)
            jit = thunk()
            oracle.set_jitter(0)
            e = m = 0.0
            for p, j in zip(plain, jit):
                assert np.array_equal(p[..., 0], j[..., 0]), name
                nz = p[..., 1] != 0
                assert np.array_equal(p[..., 1][~nz], j[..., 1][~nz]), name
                if nz.any():
                    e = max(e, float((np.abs(j[..., 1].astype(np.float64)[nz] - p[..., 1][nz]) / p[..., 1][nz]).max()))
                m = max(m, float(np.abs(j[..., 2].astype(np.float64) - p[..., 2]).max() / 257.0))
            print('%-16s jitter %d: e_out max rel %.3e   mask_sum / 257 max abs %.3e' % (name, seed, e, m))
            worst_e, worst_m = max(worst_e, e), max(worst_m, m)
    print('largest: e_out rel %.3e, mask_sum / 257 abs %.3e  ->  bars (4 x): %.3e, %.3e' % (worst_e, worst_m, 4 * worst_e, 4 * worst_m))


if __name__ == '__main__':
    main()
