"""
GPU: what the sample-rate stages cost (include/pv_koala_batch.h: pv_koala_batch_init_rate; koala_amd/csrc/kns_resample.hip), bf16, one
MI355X: 4096 streams x 64 frames on device pointers at 8, 32 and 48 kHz against the 16 kHz handle of the same build.  The four handles
ALTERNATE in one loop of the same process; a repeat is --calls calls enqueued back to back and one synchronise, timed by HIP events on the
handle's stream.  Every figure is the median of --repeats timed repeats after a warm-up.

The prediction to hold the figures against, by instruction count: about 25 k lane-FMAs per stream-frame at 8 and 32 kHz for both stages
(+8 % on the step), about 75 k at 48 kHz (+23 %).  There is no bar on the time: a 16 kHz handle launches the parent commit's kernels
(tools/asm_same.py) and nothing else.

Writes the section "== 3. measured" of profiles/r11_sample_rate.txt (or --out); what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 3. measured (tools/sample_rate_bench.py)'
RATES = (16000, 8000, 32000, 48000)


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms at 16 kHz)')
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_sample_rate.txt'))
    a = ap.parse_args()

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
    say('sample-rate handles, bf16, %s, %d streams x %d frames, device pointers, medians of %d repeats [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, T, a.repeats))
    stream = torch.cuda.Stream()
    handles = {}
    for rate in RATES:
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
    for rate in RATES:  # (priming: every handle has run before anything is timed)
        run(rate, 2)
    stream.synchronize()
    t0 = time.perf_counter()
    run(16000, 4)
    stream.synchronize()
    calls = a.calls or max(2, int(0.02 / ((time.perf_counter() - t0) / 4)))
    ms = {rate: [] for rate in RATES}
    for r in range(a.warmup + a.repeats):
        for rate in RATES:  # (alternating: the handles share every drift of the clocks)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            run(rate, calls)
            e1.record(stream)
            stream.synchronize()
            if r >= a.warmup:
                ms[rate].append(e0.elapsed_time(e1) / calls)
    base = statistics.median(ms[16000])
    say('%d calls per repeat' % calls)
    for rate in RATES:
        d = med_spread(ms[rate])
        say('    %5d Hz   call %.4f ms [%.4f .. %.4f]   %+.2f %% on the 16 kHz call   %.1f M stream-frames/s' %
            ((rate,) + d + ((d[0] / base - 1) * 100, B * T / d[0] / 1e3)))
    for h, _, _ in handles.values():
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
