"""
GPU: what the sample formats of batch handles cost (include/pv_koala_batch.h: pv_koala_batch_init_config; koala_amd/csrc/kns_format.hip),
bf16, one MI355X, one run:

  device pointers   4096 streams x 64 frames, 16 kHz, frames/s for each of the four formats (the yardstick of the format rows is this build's
                    own s16 row; the yardstick of the s16 row is bench.py on the parent commit)
  host pointers     the same shape through pageable and through page-locked host memory.  The s16 handle's host path is pipelined in
                    sub-chunks; a format handle's is one copy in, the device route, one copy out.
  packet handle     8 kHz, 80-sample (10 ms) packets, 4096 streams with mixed phases: a mu-law packet handle against the same handle in s16,
                    wall milliseconds per call

Per row: the median of the timed calls [10th .. 90th percentile].  There is no bar on speed.

Writes the section "== 2. measured" of profiles/r13_sample_format.txt (or --out); what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 2. measured (tools/sample_format_bench.py)'
FORMATS = ('s16', 'f32', 'ulaw', 'alaw')


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_sample_format.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('sample_format_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import formats
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = a.streams, a.frames
    total = a.calls + a.warmup
    s16 = koala_amd.workload.synth_streams(B, T, 7)
    say('sample formats, bf16, %s, %d timed calls after %d, wall time per call: median [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), a.calls, a.warmup))
    say('')
    say('%d streams x %d frames, 16 kHz' % (B, T))
    base = {}
    for where in ('device pointers', 'host pointers, pageable', 'host pointers, page-locked'):
        for fmt in FORMATS:
            kb = koala_amd.create_batch('bench', B, T, 'bf16', model_path=model, sample_format=fmt)
            x = formats.encode(fmt, s16)
            t = []
            if where == 'device pointers':
                xd = torch.from_numpy(x).cuda()
                yd = torch.empty_like(xd)
                torch.cuda.synchronize()
                for i in range(total):
                    t0 = time.perf_counter()
                    kb.process_device(T, xd.data_ptr(), yd.data_ptr())
                    kb.synchronize()
                    t.append(time.perf_counter() - t0)
            else:
                if where.endswith('page-locked'):
                    xin, out = kb.alloc_host(T), kb.alloc_host(T)
                    xin[:] = x
                else:
                    xin, out = x, np.empty_like(x)
                for i in range(total):
                    t0 = time.perf_counter()
                    kb.process_into(xin, out)
                    t.append(time.perf_counter() - t0)
            kb.delete()
            m, lo, hi = med_spread([v * 1e3 for v in t[a.warmup:]])
            base.setdefault(where, m)
            say('    %-27s %-5s %8.3f ms per call [%.3f .. %.3f]   %8.2f M frames/s   (%+6.1f %% time against s16)' %
                (where, fmt, m, lo, hi, B * T / m / 1e3, 100 * (m / base[where] - 1)))

    rate, P = 8000, 80
    say('')
    say('packet handle, %d Hz, %d-sample packets, %d streams, mixed phases, device pointers' % (rate, P, B))
    calls, warmup = 6 * a.calls, 4 * a.warmup
    xs = koala_amd.workload.synth_streams(B, (calls + warmup + 2) * P // 256 + 2, 9)
    first = ((np.arange(B) * 37) % (P + 1)).astype(np.int32)
    counts = np.full(B, P, np.int32)
    for fmt in ('s16', 'ulaw'):
        kp = koala_amd.create_batch('bench', B, precision='bf16', model_path=model, sample_rate=rate, packet_samples=P, sample_format=fmt)
        xd = torch.from_numpy(formats.encode(fmt, np.ascontiguousarray(xs[:, :P]))).cuda()
        yd = torch.zeros_like(xd)
        torch.cuda.synchronize()
        kp.process_device_packets(P, first, xd.data_ptr(), yd.data_ptr())
        t = []
        for i in range(calls + warmup):
            xd.copy_(torch.from_numpy(formats.encode(fmt, np.ascontiguousarray(xs[:, (i + 1) * P:(i + 2) * P]))))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kp.process_device_packets(P, counts, xd.data_ptr(), yd.data_ptr())
            kp.synchronize()
            t.append(time.perf_counter() - t0)
        kp.delete()
        m, lo, hi = med_spread([v * 1e3 for v in t[warmup:]])
        base.setdefault('packets', m)
        say('    %-5s %8.4f ms per call [%.4f .. %.4f]   (%+6.1f %% time against s16)' % (fmt, m, lo, hi, 100 * (m / base['packets'] - 1)))

    head = ''
    if os.path.exists(a.out):
        head = open(a.out).read().split(MARK)[0]
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n' + '\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
