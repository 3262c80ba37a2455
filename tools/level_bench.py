"""
GPU: what the output leveller costs (include/pv_koala_batch.h: pv_koala_batch_set_level; level_track_kernel and level_apply_kernel of
koala_amd/csrc/kns_level.hip), bf16, device pointers, one MI355X, 4096 streams x 64 frames (--streams, --frames).  Every figure is the
median of --repeats timed repeats after a warm-up, with the 10th and 90th percentile beside it.

Three handles of the same build and shape -- one that never levels, which runs the launches a handle without the feature runs, one with
every stream on and one with every second stream on -- ALTERNATE in one loop, so they share every drift of the clocks; a repeat is --calls
calls enqueued back to back and one synchronise, timed by HIP events on the handles' stream.  The settings class every frame as speech
(theta = 0, no floor), so every levelling stream's gain moves and no frame takes the apply kernel's early return.  The stage is two
launches behind a call that now writes its frame report (into a buffer of the engine's): the difference of the calls is the two launches
AND the report form of the call's synthesis launch.  A kernel trace tells them apart (profiles/r23_level.txt, section 3).

The prediction to hold the figures against is in DESIGN.md section 6 (Output leveller): the apply launch moves B T 512 bytes each way.  The
bench's headline on this build against the parent commit's is tools/ab.sh with the two libraries; its lines are added to the same file by
hand.  Writes the section "== 2. measured" of profiles/r23_level.txt (or --out): what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 2. measured (tools/level_bench.py)'


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23_level.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('level_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import level
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    say('output leveller, bf16, %s, %d streams x %d frames, device pointers, medians of %d repeats [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, T, a.repeats))
    on = level.settings(theta=0.0, floor_dbfs=-200.0)
    neutral = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    profiled = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, level=on)
    half = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    half.set_level([on if b % 2 else None for b in range(B)])
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (-(-B // 64), 1))[:B])).cuda()
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream()
    forms = [('plain call', neutral), ('every stream levels', profiled), ('every second stream', half)]
    for _, h in forms:
        h.set_stream(stream.cuda_stream)

    def run(h, n):
        for _ in range(n):
            h.process_device(T, x.data_ptr(), y.data_ptr())

    torch.cuda.synchronize()
    run(neutral, 2)
    run(profiled, 2)
    run(half, 2)
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
    say('    byte-count prediction (not measured): the apply launch moves %.0f MB each way, about 60-70 us at the achievable bandwidth; the tracker moves %.1f MB'
        % (moved / 2, B * T * 16 / 1e6 + B * T * 8 / 1e6))
    assert (profiled.level_state()[:, 1] != 1.0).all()  # (every stream's gain moved: the apply launch did its work)
    for _, h in forms:
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
