"""
GPU: what packet handles at 44 100 and 22 050 Hz cost (koala_amd/csrc/kns_fractional.hip) next to the 48 kHz packet handle, bf16, one
MI355X, 4096 streams, 20 ms packets on device pointers, every stream delivering one FULL packet per timed call.  One ragged call in front
of the loop gives stream b its own first packet length, so the streams differ in N mod 441 and in the inner packetiser's fill; the timed
calls then keep those differences -- 882 = 2 * 441 and 441 return every stream to its own phase, every call yields exactly 320 inner
samples per stream, and a stream completes 1 or 2 inner frames in it according to its fill (sub-calls with holds).  "Mixed phases" means
that and no more: the timed counts are not ragged.  The times are HOST-INCLUSIVE wall times per call -- the call's host plan, its launches
and one synchronize -- not kernel times.  The three
handles are timed in ONE alternating loop (48 kHz, 44.1 kHz, 22.05 kHz, 48 kHz, ...), so that clock and thermal drift reach all of them
alike.  Per handle: wall milliseconds per call (median [10th .. 90th percentile]), microseconds per stream and 16 ms of audio, and the
ratio to the 48 kHz handle's.  There is no bar on speed; `bench.py` (a 16 kHz frame handle) must read as before.

Writes the section "== 3. measured" of profiles/r18_fractional_rate.txt (or --out); what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 3. measured (tools/fractional_rate_bench.py)'
RATES = (48000, 44100, 22050)


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=120)
    ap.add_argument('--warmup', type=int, default=16)
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_fractional_rate.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('fractional_rate_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, total = a.streams, a.calls + a.warmup
    say('20 ms packets, bf16, %s, %d streams, %d timed calls per handle after %d, one alternating loop' % (torch.cuda.get_device_name(0), B, a.calls, a.warmup))
    say('host-inclusive wall time per call (host plan, launches, one synchronize; not kernel time): median [10th .. 90th percentile]')
    say('every timed call: the full count for all streams; one ragged call in front leaves the streams at different N mod 441 and inner fill,')
    say('which full counts keep (882 = 2 * 441; 320 inner samples per stream and call, 1 or 2 inner frames by fill)')
    x = koala_amd.workload.synth_streams(B, 8, 7)
    lanes = {}
    for rate in RATES:
        P = rate // 50
        kb = koala_amd.create_batch('bench', B, precision='bf16', model_path=model, sample_rate=rate, packet_samples=P)
        xd = torch.from_numpy(np.ascontiguousarray(x[:, :P])).cuda()
        yd = torch.zeros_like(xd)
        torch.cuda.synchronize()
        kb.process_device_packets(P, ((np.arange(B) * 37) % (P + 1)).astype(np.int32), xd.data_ptr(), yd.data_ptr())  # mixed phases
        kb.synchronize()
        lanes[rate] = (kb, P, xd, yd, np.full(B, P, np.int32), [])
    for i in range(total):
        for rate in RATES:
            kb, P, xd, yd, counts, t = lanes[rate]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kb.process_device_packets(P, counts, xd.data_ptr(), yd.data_ptr())
            kb.synchronize()
            if i >= a.warmup:
                t.append(time.perf_counter() - t0)
    base = statistics.median(lanes[48000][5])
    for rate in RATES:
        kb, P, _, _, _, t = lanes[rate]
        m, lo, hi = med_spread([v * 1e3 for v in t])
        say('    %6d Hz  %4d samples  %8.4f ms per call [%.4f .. %.4f]   %7.4f us per stream and 16 ms of audio   %.3f x the 48 kHz handle' %
            (rate, P, m, lo, hi, m * 1e3 / B * 16.0 / 20.0, m / (base * 1e3)))
        kb.delete()

    head = ''
    if os.path.exists(a.out):
        head = open(a.out).read().split(MARK)[0]
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n' + '\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
