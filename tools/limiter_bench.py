"""
GPU: what the peak limiter costs (include/pv_koala_batch.h: pv_koala_batch_set_limiter; limit_kernel of koala_amd/csrc/kns_limit.hip), bf16,
device pointers, one MI355X, 4096 streams x 64 frames (--streams, --frames).  Every figure is the median of --repeats timed repeats after a
warm-up, with the 10th and 90th percentile beside it.

Four handles of the same build and shape -- the plain call, the limiter alone, the leveller alone, and both -- ALTERNATE in one loop, so
they share every drift of the clocks; a repeat is --calls calls enqueued back to back and one synchronise, timed by HIP events on the
handles' stream.  The ceiling is 1000 (-30 dBFS) with the default release, so every stream of the bench's input limits in most frames and no
frame takes the kernel's early return; the leveller's settings class every frame as speech, as tools/level_bench.py's do.  The limiter alone
is one launch behind the plain call; with the leveller it stands in level_apply_kernel's place, so "both" against "the leveller alone" is
the difference of the two launches.

The prediction to hold the figures against is in DESIGN.md section 6 (Peak limiter): the launch reads and writes every sample once, B T 512
bytes each way.  The bench's headline on this build against the parent commit's is tools/ab.sh with the two libraries; its lines are added
to the same file by hand.  Writes the section "== 2. measured" of profiles/r25_limiter.txt (or --out): what stands in front of that
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

MARK = '== 2. measured (tools/limiter_bench.py)'


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r25_limiter.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('limiter_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import level, limiter
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    say('peak limiter, bf16, %s, %d streams x %d frames, device pointers, medians of %d repeats [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, T, a.repeats))
    lev, lim = level.settings(theta=0.0, floor_dbfs=-200.0), limiter.settings(ceiling_dbfs=-30.0)
    neutral = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    limits = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, limiter=lim)
    levels = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, level=lev)
    both = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, level=lev, limiter=lim)
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (-(-B // 64), 1))[:B])).cuda()
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream()
    forms = [('plain call', neutral), ('limiter alone', limits), ('leveller alone', levels), ('leveller and limiter', both)]
    for _, h in forms:
        h.set_stream(stream.cuda_stream)

    def run(h, n):
        for _ in range(n):
            h.process_device(T, x.data_ptr(), y.data_ptr())

    torch.cuda.synchronize()
    for _, h in forms:
        run(h, 2)
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
    say('%d calls per repeat' % calls)
    base = statistics.median(dev[forms[0][0]])
    moved = B * T * 512 * 2 / 1e6
    for name, _ in forms:
        d = med_spread(dev[name])
        say('    %-22s call %.4f ms [%.4f .. %.4f] (x %.4f)   over the plain call %.1f us' % ((name,) + d + (d[0] / base, 1e3 * (d[0] - base))))
    d = {name: statistics.median(dev[name]) for name, _ in forms}
    say("    the limiter's launch in level_apply_kernel's place: %.1f us over the leveller alone" % (1e3 * (d['leveller and limiter'] - d['leveller alone'])))
    say('    byte-count prediction (not measured): the launch moves %.0f MB each way, about 60-70 us at the achievable bandwidth' % (moved / 2))
    assert (limits.limiter_state() < 1.0).any() and (both.limiter_state() < 1.0).any()  # (the limiter did its work)
    assert (both.level_state()[:, 1] != 1.0).all()
    for _, h in forms:
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
