"""
GPU: what the per-stream attenuation limit costs (include/pv_koala_batch.h: pv_koala_batch_set_min_gain; the kMinGain arm of
koala_amd/csrc/kns_stft.hip's synthesis kernel), bf16, device pointers, one MI355X.  Every figure is the median of --repeats timed
repeats after a warm-up.

 (b1) the limited call (every stream at gain 0.25) against the plain call of the same build at 4096 x 64, 1024 x 64 and 4096 x 1: two
      handles of the same shape, one with the limit and one without, ALTERNATE in one loop; a repeat is --calls calls enqueued back to back
      and one synchronise, timed by HIP events on the handles' stream.  The synthesis launch alone is read from the handles' own profile
      (pv_koala_batch_profile_*: events around every launch) in a second, shorter loop.
 (b2) the one-frame single-stream call (pv_koala_process, the hipGraph path): p50 / p99 of the host clock around the call, without a limit,
      with gain 0.25, again without (the plain graphs are still there), and with another gain before EVERY call: each such call uploads
      its table, the path where the upload is the largest share of a call.  The setter stands outside the timed span.

The prediction to hold the figures against: the arm adds 34 full-rate VALU instructions per lane and frame (17 products, 17 sums) to a
kernel that issues roughly 1 700, about 2 % of the synthesis launch and 0.2 % of the bench step.

(a), the bench's headline on this build against the parent commit's, is tools/ab.sh with the two libraries; its lines are added to the same
file by hand, as are the file's first sections (assembly comparison, registers).  --library: another build of the library (an A/B
against a parent commit: the two alternate in one session); --one-frame-only: (b2) alone.  Writes the section "== 3. measured" of
profiles/r09_min_gain.txt (or --out): what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


MARK = '== 3. measured (tools/min_gain_bench.py)'


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms)')
    ap.add_argument('--frames', type=int, default=4000, help='frames per phase of the single-stream measurement')
    ap.add_argument('--gain', type=float, default=0.25)
    ap.add_argument('--library', default=None, help='alternative libpv_koala.so')
    ap.add_argument('--one-frame-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_min_gain.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('min_gain_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    lib = a.library or koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('per-stream attenuation limit, bf16, %s, medians of %d repeats [10th .. 90th percentile]' % (torch.cuda.get_device_name(0), a.repeats))
    for B, T in () if a.one_frame_only else ((4096, 64), (1024, 64), (4096, 1)):
        plain = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, library_path=lib)
        limited = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, library_path=lib)
        limited.set_min_gain(a.gain)
        x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (B // 64, 1)))).cuda()
        y = torch.zeros_like(x)
        stream = torch.cuda.Stream()
        forms = [('plain call', plain), ('every stream at gain %g' % a.gain, limited)]
        for _, h in forms:
            h.set_stream(stream.cuda_stream)

        def run(h, n):
            for _ in range(n):
                h.process_device(T, x.data_ptr(), y.data_ptr())

        torch.cuda.synchronize()
        run(plain, 2)
        run(limited, 2)
        stream.synchronize()
        t0 = time.perf_counter()
        run(plain, 4)
        stream.synchronize()
        calls = a.calls or max(4, int(0.02 / ((time.perf_counter() - t0) / 4)))
        dev = {f[0]: [] for f in forms}
        for r in range(a.warmup + a.repeats):
            for name, h in forms:  # (alternating: the forms share every drift of the clocks)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                run(h, calls)
                e1.record(stream)
                stream.synchronize()
                if r >= a.warmup:
                    dev[name].append(e0.elapsed_time(e1) / calls)
        # the synthesis launch alone: the handles' own events around every launch
        syn, seen = {}, {}
        for name, h in forms:
            h.profile_enable(True)
            seen[name] = (0.0, 0)
        for r in range(a.warmup + a.repeats):
            for name, h in forms:
                run(h, 4)
                stream.synchronize()
                p = h.profile_read()['synthesis']  # (running totals since profile_enable)
                ms, n = p['ms'] - seen[name][0], p['launches'] - seen[name][1]
                seen[name] = (p['ms'], p['launches'])
                if r >= a.warmup and n:
                    syn.setdefault(name, []).append(ms / n)
        say('(b1) %d streams x %d frames, device pointers, %d calls per repeat' % (B, T, calls))
        base, sbase = statistics.median(dev[forms[0][0]]), statistics.median(syn[forms[0][0]])
        for name, _ in forms:
            d, s = med_spread(dev[name]), med_spread(syn[name])
            say('    %-28s call %.4f ms [%.4f .. %.4f] (%+.2f %%)   synthesis launch %.4f ms [%.4f .. %.4f] (%+.2f %%)' %
                ((name,) + d + ((d[0] / base - 1) * 100,) + s + ((s[0] / sbase - 1) * 100,)))
        for _, h in forms:
            h.set_stream(0)
            h.delete()

    # ---- the single-stream handle, one frame per call
    frame = np.ascontiguousarray(koala_amd.workload.synth_streams(1, 1, 2)[0])
    os.environ['KOALA_AMD_PRECISION'] = 'bf16'  # (the single-stream handle takes its precision from the environment)
    k = koala_amd.create('key', model_path=model, library_path=lib)
    say('(b2) pv_koala_process, one stream, one frame per call (hipGraph replay), %d calls per phase, host clock, us' % a.frames)
    for name, g in (('no limit', 0.0), ('gain %g' % a.gain, a.gain), ('no limit again', 0.0), ('a new gain every call', None)):
        k.set_min_gain(g or 0.0)
        v = []
        for i in range(200 + a.frames):
            if g is None:
                k.set_min_gain(a.gain + 0.001 * (i % 500))
            t0 = time.perf_counter()
            k.process(frame)
            if i >= 200:
                v.append((time.perf_counter() - t0) * 1e6)
        v.sort()
        say('    %-22s p50 %.1f   p90 %.1f   p99 %.1f' % (name, v[len(v) // 2], v[len(v) * 9 // 10], v[len(v) * 99 // 100]))
    k.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
