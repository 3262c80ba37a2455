"""
GPU: what the high-band carry costs (include/pv_koala_batch.h: HIGH-BAND CARRY; koala_amd/csrc/kns_highband.hip), bf16, one MI355X: a frame
handle at 48 kHz and at 32 kHz with `high_band='carry'` against the same handle without it, of the same build, 4096 streams x 64 frames each
on device pointers, the two ALTERNATING in one loop of the same process, in --runs runs (3) of --repeats timed repeats each.  A repeat is
--calls calls enqueued back to back and one synchronise, timed by HIP events on the handle's stream.  Every figure is the median of a run's
repeats after a warm-up; the ratio is taken to the plain handle of the same run.

The plain call runs the launches it always ran, so its figure is the parent commit's.  The prediction to hold the ratio against (DESIGN.md
section 6): one more out-stage-sized chain per output, x and the in-stage's rows read once more, E read and rewritten.  There is no bar on
the ratio.

Writes the section "== measured" of the file given by --out; what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== measured (tools/high_band_bench.py)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms of the plain handle)')
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rates', default='48000,32000')
    ap.add_argument('--out', required=True)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('high_band_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    stream = torch.cuda.Stream()
    for rate in [int(r) for r in a.rates.split(',')]:
        say('high-band carry, bf16, %s, %d streams x %d frames at %d Hz: carry against plain, device pointers, %d alternating runs, medians of %d repeats each' %
            (torch.cuda.get_device_name(0), B, T, rate, a.runs, a.repeats))
        rng = np.random.default_rng(1)
        base = rng.integers(-8192, 8193, size=(64, T * rate * 256 // 16000)).astype(np.int16)  # (energy up to Nyquist; the cost does not depend on it)
        rows = np.ascontiguousarray(np.tile(base, (B // 64 + 1, 1))[:B])
        handles = {}
        for name, mode in (('plain', None), ('carry', 'carry')):
            h = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, sample_rate=rate, high_band=mode)
            x = torch.from_numpy(rows).cuda()
            h.set_stream(stream.cuda_stream)
            handles[name] = (h, x, torch.zeros_like(x))
        names = list(handles)

        def run(name, n):
            h, x, y = handles[name]
            for _ in range(n):
                h.process_device(T, x.data_ptr(), y.data_ptr())

        torch.cuda.synchronize()
        for name in names:  # (priming: every handle has run before anything is timed)
            run(name, 2)
        stream.synchronize()
        t0 = time.perf_counter()
        run('plain', 4)
        stream.synchronize()
        calls = a.calls or max(2, int(0.02 / ((time.perf_counter() - t0) / 4)))
        say('%d calls per repeat' % calls)
        ratios, extra = [], []
        for k in range(a.runs):
            ms = {name: [] for name in names}
            for r in range(a.warmup + a.repeats):
                for name in names:  # (alternating: the handles share every drift of the clocks)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    run(name, calls)
                    e1.record(stream)
                    stream.synchronize()
                    if r >= a.warmup:
                        ms[name].append(e0.elapsed_time(e1) / calls)
            m = {name: statistics.median(ms[name]) for name in names}
            ratios.append(m['carry'] / m['plain'])
            extra.append((m['carry'] - m['plain']) * 1000)
            say('run %d' % (k + 1))
            for name in names:
                say('    %-6s  call %.4f ms [%.4f .. %.4f]   x %.4f of the plain call (%+.2f %%)' %
                    (name, m[name], min(ms[name]), max(ms[name]), m[name] / m['plain'], (m[name] / m['plain'] - 1) * 100))
        say('the carry at %d Hz, median of the runs [least .. most]: x %.4f [%.4f .. %.4f] of the plain call, %+.1f us [%+.1f .. %+.1f] per call'
            % (rate, statistics.median(ratios), min(ratios), max(ratios), statistics.median(extra), min(extra), max(extra)))
        for h, _, _ in handles.values():
            h.set_stream(0)
            h.delete()
        handles.clear()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
