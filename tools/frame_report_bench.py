"""
GPU: what the frame report costs (include/pv_koala_batch.h: pv_koala_batch_process_call with `report`; the synthesis_report_kernel forms of
koala_amd/csrc/kns_stft.hip), bf16, one MI355X.  Every figure is the median of --repeats timed repeats after a warm-up.

 (1) 4096 x 64 on device pointers, with and without a report: ONE handle, the two forms ALTERNATE in one loop of the same process; a repeat
     is --calls calls enqueued back to back and one synchronise, timed by HIP events on the handle's stream.  The synthesis launch alone is
     read from the handle's own profile (pv_koala_batch_profile_*: events around every launch) in a second, shorter loop.
 (2) the one-frame step of the single-stream handle (pv_koala_process / pv_koala_process_report, the hipGraph path): p50 / p99 of the
     host clock around the call, without a report, with one, and again without (the plain graphs are still there).

The prediction to hold the figures against: about 135 full-rate VALU instructions per lane and frame on the ~1 700 of the synthesis kernel,
roughly 8 % of the synthesis launch and 0.7 % of the bench step, for calls that ask.  There is no bar on the time: the guarantee for callers
who do not ask is that their kernels are the parent commit's instructions (tools/asm_same.py).

Writes the section "== 4. measured" of profiles/r10_frame_report.txt (or --out): what stands in front of that heading -- bars, registers,
assembly comparison -- is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 4. measured (tools/frame_report_bench.py)'


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms)')
    ap.add_argument('--frames', type=int, default=4000, help='frames per phase of the single-stream measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r10_frame_report.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('frame_report_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('frame report, bf16, %s, medians of %d repeats [10th .. 90th percentile]' % (torch.cuda.get_device_name(0), a.repeats))
    B, T = 4096, 64
    h = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (B // 64, 1)))).cuda()
    y = torch.zeros_like(x)
    rep = torch.zeros((B, T, 4), dtype=torch.float32, device='cuda')
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    forms = [('no report', 0), ('with a report', rep.data_ptr())]

    def run(rp, n):
        for _ in range(n):
            h.process_device_call(T, x.data_ptr(), y.data_ptr(), rp)

    torch.cuda.synchronize()
    for _, rp in forms:  # (priming, as the bench does: both forms have run before anything is timed)
        run(rp, 2)
    stream.synchronize()
    t0 = time.perf_counter()
    run(0, 4)
    stream.synchronize()
    calls = a.calls or max(4, int(0.02 / ((time.perf_counter() - t0) / 4)))
    dev = {f[0]: [] for f in forms}
    for r in range(a.warmup + a.repeats):
        for name, rp in forms:  # (alternating: the forms share every drift of the clocks)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            run(rp, calls)
            e1.record(stream)
            stream.synchronize()
            if r >= a.warmup:
                dev[name].append(e0.elapsed_time(e1) / calls)
    syn, seen = {}, (0.0, 0)
    h.profile_enable(True)
    for r in range(a.warmup + a.repeats):
        for name, rp in forms:
            run(rp, 4)
            stream.synchronize()
            p = h.profile_read()['synthesis']  # (running totals since profile_enable)
            ms, n = p['ms'] - seen[0], p['launches'] - seen[1]
            seen = (p['ms'], p['launches'])
            if r >= a.warmup and n:
                syn.setdefault(name, []).append(ms / n)
    say('(1) %d streams x %d frames, device pointers, %d calls per repeat' % (B, T, calls))
    base, sbase = statistics.median(dev[forms[0][0]]), statistics.median(syn[forms[0][0]])
    for name, _ in forms:
        d, s = med_spread(dev[name]), med_spread(syn[name])
        say('    %-16s call %.4f ms [%.4f .. %.4f] (%+.2f %%)   synthesis launch %.4f ms [%.4f .. %.4f] (%+.2f %%)' %
            ((name,) + d + ((d[0] / base - 1) * 100,) + s + ((s[0] / sbase - 1) * 100,)))
    h.set_stream(0)
    h.delete()

    frame = np.ascontiguousarray(koala_amd.workload.synth_streams(1, 1, 2)[0])
    os.environ['KOALA_AMD_PRECISION'] = 'bf16'  # (the single-stream handle takes its precision from the environment)
    k = koala_amd.create('key', model_path=model)
    say('(2) one stream, one frame per call (hipGraph replay), %d calls per phase, host clock, us' % a.frames)
    for name, fn in (('no report', k.process), ('with a report', k.process_with_report), ('no report again', k.process)):
        v = []
        for i in range(200 + a.frames):
            t0 = time.perf_counter()
            fn(frame)
            if i >= 200:
                v.append((time.perf_counter() - t0) * 1e6)
        v.sort()
        say('    %-16s p50 %.1f   p90 %.1f   p99 %.1f' % (name, v[len(v) // 2], v[len(v) * 9 // 10], v[len(v) * 99 // 100]))
    k.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
