"""
GPU: what the sample-rate stages cost (include/pv_koala_batch.h: pv_koala_batch_init_rate; koala_amd/csrc/kns_resample.hip), bf16, one
MI355X: 4096 streams x 64 frames on device pointers at --rates (8, 32, 48, 12 and 24 kHz) against the 16 kHz handle of the same build,
all handles ALTERNATING in one loop of the same process, in --runs runs (3) of --repeats timed repeats each.  A repeat is --calls calls
enqueued back to back and one synchronise, timed by HIP events on the handle's stream.  Every figure is the median of a run's repeats
after a warm-up; the ratio is taken to the 16 kHz handle of the same run.

The prediction to hold the figures against, by instruction count: about 25 k lane-FMAs per stream-frame for both
stages at 8, 12 and 32 kHz, about 37 k at 24 kHz, about 75 k at 48 kHz.  There is no bar on the time: a 16 kHz handle launches the parent
commit's kernels (tools/asm_same.py) and nothing else.

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

MARK = '== measured (tools/sample_rate_bench.py)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms at 16 kHz)')
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--rates', type=int, nargs='+', default=[8000, 32000, 48000, 12000, 24000], help='the rates next to 16 kHz')
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    rates = [16000] + [r for r in a.rates if r != 16000]

    import torch
    if not torch.cuda.is_available():
        sys.exit('sample_rate_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    say('rate handles, bf16, %s, %d streams x %d frames, device pointers, %d alternating runs, medians of %d repeats each' %
        (torch.cuda.get_device_name(0), B, T, a.runs, a.repeats))
    stream = torch.cuda.Stream()
    handles = {}
    for rate in rates:
        h = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, sample_rate=rate)
        fl = h.frame_length
        base = koala_amd.workload.synth_streams(64, T * fl // 256 + 1, 1)[:, :T * fl]  # (the bench's streams, taken as samples at `rate`)
        x = torch.from_numpy(np.ascontiguousarray(np.tile(base, (B // 64 + 1, 1))[:B])).cuda()
        h.set_stream(stream.cuda_stream)
        handles[rate] = (h, x, torch.zeros_like(x))

    def run(rate, n):
        h, x, y = handles[rate]
        for _ in range(n):
            h.process_device(T, x.data_ptr(), y.data_ptr())

    torch.cuda.synchronize()
    for rate in rates:  # (priming: every handle has run before anything is timed)
        run(rate, 2)
    stream.synchronize()
    t0 = time.perf_counter()
    run(16000, 4)
    stream.synchronize()
    calls = a.calls or max(2, int(0.02 / ((time.perf_counter() - t0) / 4)))
    say('%d calls per repeat' % calls)
    ratios = {rate: [] for rate in rates}
    for k in range(a.runs):
        ms = {rate: [] for rate in rates}
        for r in range(a.warmup + a.repeats):
            for rate in rates:  # (alternating: the handles share every drift of the clocks)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                run(rate, calls)
                e1.record(stream)
                stream.synchronize()
                if r >= a.warmup:
                    ms[rate].append(e0.elapsed_time(e1) / calls)
        base = statistics.median(ms[16000])
        say('run %d' % (k + 1))
        for rate in rates:
            m = statistics.median(ms[rate])
            ratios[rate].append(m / base)
            say('    %5d Hz   call %.4f ms [%.4f .. %.4f]   x %.4f of the 16 kHz call (%+.2f %%)' %
                (rate, m, min(ms[rate]), max(ms[rate]), m / base, (m / base - 1) * 100))
    say('ratio to the 16 kHz handle, median of the runs [least .. most]')
    for rate in rates[1:]:
        v = sorted(ratios[rate])
        say('    %5d Hz   x %.4f [%.4f .. %.4f]' % (rate, statistics.median(v), v[0], v[-1]))
    for h, _, _ in handles.values():
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
