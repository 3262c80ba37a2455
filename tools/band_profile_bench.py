"""
GPU: what the band profile costs (include/pv_koala_batch.h: pv_koala_batch_set_band_profile; synthesis_profile_kernel of
koala_amd/csrc/kns_stft.hip), bf16, device pointers, one MI355X, 4096 streams x 64 frames (--streams, --frames).  Every figure is the
median of --repeats timed repeats after a warm-up, with the 10th and 90th percentile beside it.

Two handles of the same build and shape, one under a profile that differs per stream (a high-pass ceiling, a depth-limit floor, random pairs)
and one neutral -- which runs the kernels a handle without the feature runs -- ALTERNATE in one loop, so they share every drift of the clocks;
a repeat is --calls calls enqueued back to back and one synchronise, timed by HIP events on the handles' stream.  The synthesis launch alone
is read from the handles' own profile (pv_koala_batch_profile_*: events around every launch) in a second, shorter loop.

The prediction to hold the figures against is in DESIGN.md section 6 (Band profile).  The bench's headline on this build against the parent
commit's is tools/ab.sh with the two libraries; its lines are added to the same file by hand, as are the file's first sections (assembly
comparison, registers).  Writes the section "== 3. measured" of profiles/r22_band_profile.txt (or --out): what stands in front of that
heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 3. measured (tools/band_profile_bench.py)'


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_band_profile.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('band_profile_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import bands
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    say('band profile, bf16, %s, %d streams x %d frames, device pointers, medians of %d repeats [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, T, a.repeats))
    rng = np.random.default_rng(0)
    p, q = rng.random((B, bands.NUM_BINS), dtype=np.float32), rng.random((B, bands.NUM_BINS), dtype=np.float32)
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    lo[0::3], hi[0::3] = 0.0, bands.highpass(90.0)
    lo[1::3], hi[1::3] = bands.depth_limit_db([(0, 6), (300, 18)]), 1.0
    neutral = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    profiled = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, band_profile=(lo, hi))
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (-(-B // 64), 1))[:B])).cuda()
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream()
    forms = [('neutral call', neutral), ('a profile per stream', profiled)]
    for _, h in forms:
        h.set_stream(stream.cuda_stream)

    def run(h, n):
        for _ in range(n):
            h.process_device(T, x.data_ptr(), y.data_ptr())

    torch.cuda.synchronize()
    run(neutral, 2)
    run(profiled, 2)
    stream.synchronize()
    t0 = time.perf_counter()
    run(neutral, 4)
    stream.synchronize()
    calls = a.calls or max(4, int(0.02 / ((time.perf_counter() - t0) / 4)))
    dev = {f[0]: [] for f in forms}
    for r in range(a.warmup + a.repeats):
        for name, h in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            e0.record(stream)
            run(h, calls)
            e1.record(stream)
            stream.synchronize()
            if r >= a.warmup:
                dev[name].append(e0.elapsed_time(e1) / calls)
    syn, seen = {}, {}
    for name, h in forms:
        h.profile_enable(True)
        seen[name] = (0.0, 0)
    for r in range(a.warmup + a.repeats):
        for name, h in forms:
            run(h, 4)
            stream.synchronize()
            pr = h.profile_read()['synthesis']  # (running totals since profile_enable)
            ms, n = pr['ms'] - seen[name][0], pr['launches'] - seen[name][1]
            seen[name] = (pr['ms'], pr['launches'])
            if r >= a.warmup and n:
                syn.setdefault(name, []).append(ms / n)
    say('%d calls per repeat' % calls)
    base, sbase = statistics.median(dev[forms[0][0]]), statistics.median(syn[forms[0][0]])
    for name, _ in forms:
        d, s = med_spread(dev[name]), med_spread(syn[name])
        say('    %-22s call %.4f ms [%.4f .. %.4f] (x %.4f)   synthesis launch %.4f ms [%.4f .. %.4f] (x %.4f)' %
            ((name,) + d + (d[0] / base,) + s + (s[0] / sbase,)))
    for _, h in forms:
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
