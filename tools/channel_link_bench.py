"""
GPU: what linked channels cost (include/pv_koala_batch.h: LINKED CHANNELS; the kLink arm of koala_amd/csrc/kns_stft_synthesis.inc), bf16, one
MI355X: a channels = 2 handle with the link on against the same handle with the link off, of the same build, 4096 streams x 64 frames each
on device pointers, the two ALTERNATING in one loop of the same process, in --runs runs (3) of --repeats timed repeats each.  A repeat is
--calls calls enqueued back to back and one synchronise, timed by HIP events on the handle's stream.  Every figure is the median of a run's
repeats after a warm-up; the ratio is taken to the unlinked handle of the same run.

The unlinked call runs the parent commit's kernels instruction for instruction (tools/asm_same.py), so its figure is the parent's.  The
prediction to hold the ratio against: per partner 17 loads and 17 v_max per lane and frame, and for this call --
out of place, so the spectrum is recomputed and the linked kernel is a report form -- the report's sums, on ~1 700 instructions.  There is
no bar on the ratio.

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

MARK = '== measured (tools/channel_link_bench.py)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms of the unlinked handle)')
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--channels', type=int, default=2)
    ap.add_argument('--out', required=True)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('channel_link_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd.channels import interleave
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T, C = a.streams, a.frames, a.channels
    say('linked channels, bf16, %s, %d streams x %d frames, channels = %d: link on against link off, device pointers, %d alternating runs, medians of %d repeats each' %
        (torch.cuda.get_device_name(0), B, T, C, a.runs, a.repeats))
    stream = torch.cuda.Stream()
    base = koala_amd.workload.synth_streams(64, T, 1)
    planar = np.ascontiguousarray(np.tile(base, (B // 64 + 1, 1))[:B])
    handles = {}
    for name, link in (('unlinked', None), ('linked', 'max')):
        h = koala_amd.create_batch('key', B, T, 'bf16', model_path=model, channels=C, channel_link=link)
        x = torch.from_numpy(interleave(planar, C)).cuda()
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
    run('unlinked', 4)
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
        ratios.append(m['linked'] / m['unlinked'])
        extra.append((m['linked'] - m['unlinked']) * 1000)
        say('run %d' % (k + 1))
        for name in names:
            say('    %-9s  call %.4f ms [%.4f .. %.4f]   x %.4f of the unlinked call (%+.2f %%)' %
                (name, m[name], min(ms[name]), max(ms[name]), m[name] / m['unlinked'], (m[name] / m['unlinked'] - 1) * 100))
    say('the link, median of the runs [least .. most]: x %.4f [%.4f .. %.4f] of the unlinked call, %+.1f us [%+.1f .. %+.1f] per call'
        % (statistics.median(ratios), min(ratios), max(ratios), statistics.median(extra), min(extra), max(extra)))
    for h, _, _ in handles.values():
        h.set_stream(0)
        h.delete()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ''
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
