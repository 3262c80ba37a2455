"""
GPU: what packet handles cost (include/pv_koala_batch.h: pv_koala_batch_process_packets; koala_amd/csrc/kns_packet.hip), bf16, one MI355X,
4096 streams, for 10 ms and 20 ms packets at 16 kHz and 20 ms packets at 48 kHz.  Three ways of serving the same traffic, every stream
delivering one packet per call:

  packets, mixed phases    a packet handle on device pointers, the streams' phases uniformly mixed (stream b starts with b's own first
                           packet length): most calls are sub-calls with holds.  At 16 kHz / 10 ms 62.5 % of the streams complete a frame
                           per call.
  packets, aligned phases  the same handle with every stream in phase: equal frame counts, the plain route without holds.
  frames, host rebuffering what a server does on a FRAME handle: a host FIFO per stream in both directions, per call the slots that have a
                           whole frame, `process_chunk_hold` through host pointers with `hold` for the others (the rebuffering is on the
                           host, so the pointers are).  Its FIFO bookkeeping is vectorised numpy here: a lower bound for a real server's loop.

Per row: wall milliseconds per call (median of the timed calls, [10th .. 90th percentile]) and useful frames/s (frames completed / wall
time).  There is no bar on speed; `bench.py` (a frame handle) must read as before.

Writes the section "== 2. measured" of profiles/r12_packets.txt (or --out); what stands in front of that heading is kept.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARK = '== 2. measured (tools/packet_bench.py)'
CASES = ((16000, 10), (16000, 20), (48000, 20))


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=120)
    ap.add_argument('--warmup', type=int, default=16)
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_packets.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('packet_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    from koala_amd import packets
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B = a.streams
    say('packet handles, bf16, %s, %d streams, %d timed calls after %d, wall time per call: median [10th .. 90th percentile]' %
        (torch.cuda.get_device_name(0), B, a.calls, a.warmup))
    for rate, ms in CASES:
        F, P = rate * 256 // 16000, rate * ms // 1000
        Tmax = -(-P // F)
        total = a.calls + a.warmup
        x = koala_amd.workload.synth_streams(B, (total + 2) * P // 256 + 2, 7)
        say('')
        say('%d Hz, %d ms packets (%d samples; a frame is %d)' % (rate, ms, P, F))
        rows = {}
        for name in ('packets, mixed phases', 'packets, aligned phases'):
            kp = koala_amd.create_batch('bench', B, precision='bf16', model_path=model, sample_rate=rate, packet_samples=P)
            first = (np.arange(B) * 37) % (P + 1) if name.endswith('mixed phases') else np.full(B, P)
            xd = torch.from_numpy(np.ascontiguousarray(x[:, :P])).cuda()
            yd = torch.zeros_like(xd)
            torch.cuda.synchronize()
            kp.process_device_packets(P, first.astype(np.int32), xd.data_ptr(), yd.data_ptr())
            counts = np.full(B, P, np.int32)
            t, frames = [], 0
            for i in range(total):
                xd.copy_(torch.from_numpy(np.ascontiguousarray(x[:, (i + 1) * P:(i + 2) * P])))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fr = kp.process_device_packets(P, counts, xd.data_ptr(), yd.data_ptr())
                kp.synchronize()
                if i >= a.warmup:
                    t.append(time.perf_counter() - t0)
                    frames += int(fr.sum())
            kp.delete()
            rows[name] = (t, frames)
        # a frame handle behind host FIFOs: the same traffic, the same phases as the mixed case
        kf = koala_amd.create_batch('bench', B, Tmax, 'bf16', model_path=model, sample_rate=rate)
        fill = ((np.arange(B) * 37) % (P + 1)) % F  # (the first packet's whole frames are not timed)
        fifo = np.zeros((B, F + P), np.int16)
        out_fifo = np.zeros((B, 2 * F + P), np.int16)
        out_fill = np.full(B, F - 1)
        t, frames = [], 0
        for i in range(total):
            pk = x[:, (i + 1) * P:(i + 2) * P]
            t0 = time.perf_counter()
            idx = fill[:, None] + np.arange(P)[None]
            np.put_along_axis(fifo, idx, pk, axis=1)
            k, new_fill = packets.frames_due(fill, np.full(B, P), F)
            done = 0
            for c0, T, hold in packets.plan(k, Tmax):
                pcm = np.ascontiguousarray(fifo[:, c0 * F:(c0 + T) * F])
                enh = kf.process(pcm) if hold is None else kf.process_hold(pcm, hold)
                run_ = np.ones(B, bool) if hold is None else hold == 0
                dst = out_fill[run_, None] + np.arange(T * F)[None]
                sub = out_fifo[run_]
                np.put_along_axis(sub, dst, enh[run_], axis=1)
                out_fifo[run_] = sub
                out_fill[run_] += T * F
                done += int(run_.sum()) * T
            # shift the residue to the front of each FIFO, hand P samples out
            shift = (k * F)[:, None] + np.arange(F)[None]
            fifo[:, :F] = np.take_along_axis(fifo, np.minimum(shift, F + P - 1), axis=1)
            delivered = out_fifo[:, :P].copy()
            out_fifo[:, :2 * F] = out_fifo[:, P:P + 2 * F]
            out_fill -= P
            fill = new_fill
            if i >= a.warmup:
                t.append(time.perf_counter() - t0)
                frames += done
            del delivered
        kf.delete()
        rows['frames, host rebuffering'] = (t, frames)
        base = statistics.median(rows['packets, aligned phases'][0])
        for name, (t, frames) in rows.items():
            m, lo, hi = med_spread([v * 1e3 for v in t])
            say('    %-26s %8.4f ms per call [%.4f .. %.4f]  (%+6.1f %% of aligned)   %9.3f M useful frames/s (%d frames, %.1f %% of streams per call)' %
                (name, m, lo, hi, 100 * (m / (base * 1e3) - 1), frames / sum(t) / 1e6, frames, 100.0 * frames / (len(t) * B)))

    head = ''
    if os.path.exists(a.out):
        head = open(a.out).read().split(MARK)[0]
    with open(a.out, 'w') as f:
        f.write(head + MARK + '\n' + '\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
