"""
GPU: what comfort noise costs (include/pv_koala_batch.h: pv_koala_batch_set_comfort_noise; synthesis_comfort_kernel of
koala_amd/csrc/kns_stft.hip, comfort_count_kernel of kns_comfort.hip), bf16, device pointers, one MI355X, 4096 streams x 64 frames
(--streams, --frames).  Every figure is the median of --repeats timed repeats after a warm-up, with the 10th and 90th percentile beside it.

Three handles of the same build and shape ALTERNATE in one loop, so they share every drift of the clocks: one with comfort noise on every
stream (a -60 dBFS pink curve, a seed per stream), one neutral -- which runs the kernels a handle without the feature runs -- and one under
a band profile that differs per stream (tools/band_profile_bench.py's).  A repeat is --calls calls enqueued back to back and one
synchronise, timed by HIP events on the handles' stream.  The synthesis launch alone is read from the handles' own profile
(pv_koala_batch_profile_*: events around every launch) in a second, shorter loop.

--trace DIR: no measurement; summarises the kernel-trace CSV files a profiler run of this tool left under DIR (one line per kernel whose
name holds "synthesis" or "comfort": launches, median and minimum duration) into the section "== 4." of the output file.

The prediction to hold the figures against is in DESIGN.md section 6 (Comfort noise).  The bench's headline on this build against the parent
commit's is tools/ab.sh with the two libraries; its lines are added to the same file by hand, as is the file's first section (assembly
comparison).  Writes the section "== 3. measured" of profiles/r24_comfort_noise.txt (or --out): what stands in front of that heading is kept.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 3. measured (tools/comfort_bench.py)'
TRACE = '== 4. the launches apart (tools/comfort_bench.py --trace: one kernel trace of a short run of the same loop; us)'


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def put(out, mark, lines, keep_behind=None):
    """the section `mark` of the file := lines; what stands in front of it is kept (and the section `keep_behind`, if it follows)"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    text = open(out).read() if os.path.exists(out) else ''
    head, _, rest = text.partition(mark)
    if head and not head.endswith('\n\n'):
        head = head.rstrip('\n') + '\n\n'
    tail = ''
    if keep_behind and keep_behind in rest:
        tail = '\n' + keep_behind + rest.split(keep_behind, 1)[1]
    with open(out, 'w') as f:
        f.write(head + mark + '\n\n' + '\n'.join(lines) + '\n' + tail)


def summarise(directory, out):
    rows = {}
    for path in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
        with open(path, newline='') as f:
            for r in csv.DictReader(f):
                name = r.get('Kernel_Name') or r.get('kernel_name') or ''
                if 'synthesis' not in name and 'comfort' not in name:
                    continue
                t0, t1 = r.get('Start_Timestamp') or r.get('start_timestamp'), r.get('End_Timestamp') or r.get('end_timestamp')
                rows.setdefault(name.split('(')[0], []).append((int(t1) - int(t0)) / 1e3)
    if not rows:
        sys.exit('comfort_bench: no kernel trace under %s' % directory)
    lines = ['    %-100s %5d launches   median %7.1f   min %7.1f' % (n[-100:], len(v), statistics.median(v), min(v)) for n, v in sorted(rows.items())]
    for s in lines:
        print(s)
    put(out, TRACE, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms)')
    ap.add_argument('--trace', default=None, metavar='DIR', help='summarise the kernel-trace CSV files under DIR instead of measuring')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r24_comfort_noise.txt'))
    a = ap.parse_args()
    if a.trace:
        return summarise(a.trace, a.out)

    import torch
    if not torch.cuda.is_available():
        sys.exit('comfort_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import bands, comfort
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    say('comfort noise, bf16, %s, %d streams x %d frames, device pointers, medians of %d repeats [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, T, a.repeats))
    rng = np.random.default_rng(0)
    p, q = rng.random((B, bands.NUM_BINS), dtype=np.float32), rng.random((B, bands.NUM_BINS), dtype=np.float32)
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    lo[0::3], hi[0::3] = 0.0, bands.highpass(90.0)
    lo[1::3], hi[1::3] = bands.depth_limit_db([(0, 6), (300, 18)]), 1.0
    neutral = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    profiled = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, band_profile=(lo, hi))
    filled = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, comfort_noise=comfort.curve(-60.0, 'pink'))
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (-(-B // 64), 1))[:B])).cuda()
    y = torch.zeros_like(x)
    stream = torch.cuda.Stream()
    forms = [('neutral call', neutral), ('a profile per stream', profiled), ('comfort noise, every stream', filled)]
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
        say('    %-28s call %.4f ms [%.4f .. %.4f] (x %.4f)   synthesis launch %.4f ms [%.4f .. %.4f] (x %.4f)' %
            ((name,) + d + (d[0] / base,) + s + (s[0] / sbase,)))
    pd, ps = statistics.median(dev[forms[1][0]]), statistics.median(syn[forms[1][0]])
    cd, cs = statistics.median(dev[forms[2][0]]), statistics.median(syn[forms[2][0]])
    say('    comfort noise against the profile call: call x %.4f, synthesis launch x %.4f' % (cd / pd, cs / ps))
    for _, h in forms:
        h.set_stream(0)
        h.delete()
    put(a.out, MARK, lines, keep_behind=TRACE)


if __name__ == '__main__':
    main()
