"""
GPU: what stream records and held streams cost (include/pv_koala_batch.h: pv_koala_batch_export_state / import_state /
process_chunk_hold; koala_amd/csrc/kns_state.hip), bf16, one MI355X.  Every figure is the median of --repeats timed repeats after a warm-up.

 (a) export and import of all 4096 streams: wall time of the ABI call (host clock around it: the call ends in a stream synchronise).
     The device time of the two kernels alone comes from a run of its own under the profiler,
         rocprofv3 --kernel-trace --stats -d <dir> -- python tools/state_bench.py --kernels-only
     and a second run with --kernel-db <dir>/..._results.db prints them, against the floor of the bytes they must move -- the
     records read and written, streams x state_size x 2 -- at the 6.3 TB/s the project records as achievable.
 (b) pv_koala_batch_process_chunk_hold with every second stream held against pv_koala_batch_process_chunk, device pointers, at
     4096 x 64, 4096 x 1 and 1024 x 64: the two forms ALTERNATE in one loop on one handle; a repeat is --calls calls enqueued back to back
     and one synchronise, timed by HIP events on the handle's stream and by the host clock.  With --parent-library (a build of the
     parent commit) the plain call of that library is timed in the same loop, next to this build's: no existing launch changed, so the
     two agree within the spread of the repeats.

Writes profiles/r08_stream_state.txt (or --out).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BPS = 6.3e12  # what a streaming kernel reaches of the MI355X's 8 TB/s


def med_spread(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


class PlainHandle(object):
    """The plain device-pointer call of ANOTHER build of the library (one without the stream-record entry points, which the package's
    binding asks for), straight through ctypes."""

    def __init__(self, library, model, B, T):
        import ctypes as C
        self._l = C.CDLL(library)
        self._l.pv_koala_batch_init.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        self._l.pv_koala_batch_process_chunk.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        self._l.pv_koala_batch_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        self._l.pv_koala_batch_delete.argtypes = [C.c_void_p]
        self._l.pv_koala_batch_delete.restype = None
        self._h = C.c_void_p()
        if self._l.pv_koala_batch_init(b'key', model.encode(), b'best', B, T, 1, C.byref(self._h)) != 0:
            sys.exit('state_bench: %s: pv_koala_batch_init failed' % library)

    def process_device(self, T, x, y):
        if self._l.pv_koala_batch_process_chunk(self._h, T, x, y) != 0:
            sys.exit('state_bench: process_chunk failed')

    def set_stream(self, s):
        self._l.pv_koala_batch_set_stream(self._h, s)

    def delete(self):
        self._l.pv_koala_batch_delete(self._h)


def kernel_times(db, nbytes):
    """lines with the two kernels' device times out of the rocpd database of a `--kernels-only` run under rocprofv3 --kernel-trace"""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, end - start from kernels where name like '%state_%port_kernel%'").fetchall()
    out = []
    for key, moved in (('state_export_kernel', nbytes), ('state_import_kernel', nbytes * 3 // 2)):  # (import writes both ping-pong copies)
        v = [d / 1e3 for n, d in rows if key in n]
        if v:
            floor = moved / ACHIEVABLE_BPS * 1e6
            out.append('    %s, device (rocprofv3 --kernel-trace, %d dispatches): %.1f us [%.1f .. %.1f]; %.0f MB at 6.3 TB/s = %.1f us: ratio %.2f' %
                       ((key, len(v)) + med_spread(v) + (moved / 1e6, floor, statistics.median(v) / floor)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=0, help='calls per repeat (0: enough for about 20 ms)')
    ap.add_argument('--kernels-only', action='store_true', help='export / import loops only (for a rocprofv3 --kernel-trace --stats run)')
    ap.add_argument('--kernel-db', default=None, help='rocpd database (*_results.db) of a --kernels-only run under rocprofv3: adds the kernel times to (a)')
    ap.add_argument('--parent-library', default=None, help='libpv_koala.so built from the parent commit (A/B of the plain call)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_stream_state.txt'))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit('state_bench: no GPU (this tool measures; it has no CPU form)')
    import koala_amd
    import koala_amd.workload
    koala_amd.build_native()
    model = koala_amd.default_model_path()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('stream records and held streams, bf16, %s, medians of %d repeats [10th .. 90th percentile]' % (torch.cuda.get_device_name(0), a.repeats))

    # ---- (a) export / import of every stream
    B = 4096
    kb = koala_amd.create_batch('key', B, 64, 'bf16', model_path=model)
    x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, 64, 1), (B // 64, 1)))).cuda()
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    kb.process_device(64, x.data_ptr(), y.data_ptr())
    kb.synchronize()
    recs = kb.export_state()
    t_exp, t_imp = [], []
    for r in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        recs = kb.export_state()
        t1 = time.perf_counter()
        kb.import_state(recs)
        t2 = time.perf_counter()
        if r >= a.warmup:
            t_exp.append((t1 - t0) * 1e3)
            t_imp.append((t2 - t1) * 1e3)
    nbytes = 2 * B * kb.state_size
    say('(a) %d streams x %d bytes; kernel floor %.1f us (%.1f MB read + written at 6.3 TB/s)' %
        (B, kb.state_size, nbytes / ACHIEVABLE_BPS * 1e6, nbytes / 1e6))
    say('    export_state, wall (kernel + %.0f MB to pageable host memory): %.3f ms [%.3f .. %.3f]' % ((nbytes / 2e6,) + med_spread(t_exp)))
    say('    import_state, wall (%.0f MB from pageable host memory + kernel): %.3f ms [%.3f .. %.3f]' % ((nbytes / 2e6,) + med_spread(t_imp)))
    if a.kernel_db:
        for line in kernel_times(a.kernel_db, nbytes):
            say(line)
        say('    (the repeats move the same 84 MB, which fit the 256 MB last-level cache: warm figures.  In the loop of (b) at 4096 x 1 a whole')
        say('     frame step runs between export and import; there the two kernels cost what (b) shows for 2048 held streams)')
    if a.kernels_only:
        kb.delete()
        return
    kb.delete()

    # ---- (b) held streams against the plain call
    libs = [('this build', None)] + ([('parent commit', a.parent_library)] if a.parent_library else [])
    for B, T in ((4096, 64), (4096, 1), (1024, 64)):
        hs = [(name, PlainHandle(lib, model, B, T) if lib else koala_amd.create_batch('key', B, T, 'bf16', model_path=model)) for name, lib in libs]
        x = torch.from_numpy(np.ascontiguousarray(np.tile(koala_amd.workload.synth_streams(64, T, 1), (B // 64, 1)))).cuda()
        y = torch.zeros_like(x)
        hold = (np.arange(B) % 2).astype(np.uint8)
        zero = np.zeros(B, np.uint8)
        stream = torch.cuda.Stream()
        for _, h in hs:
            h.set_stream(stream.cuda_stream)
        forms = [('process_chunk, this build', hs[0][1], None), ('process_chunk_hold, all-zero mask', hs[0][1], zero),
                 ('process_chunk_hold, every second stream held', hs[0][1], hold)]
        if len(hs) > 1:
            forms.append(('process_chunk, parent commit', hs[1][1], None))

        def run(h, m, n):
            for _ in range(n):
                if m is None:
                    h.process_device(T, x.data_ptr(), y.data_ptr())
                else:
                    h.process_device_hold(T, x.data_ptr(), y.data_ptr(), m)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(hs[0][1], None, 4)
        stream.synchronize()
        calls = a.calls or max(4, int(0.02 / ((time.perf_counter() - t0) / 4)))
        dev = {f[0]: [] for f in forms}
        wall = {f[0]: [] for f in forms}
        for r in range(a.warmup + a.repeats):
            for name, h, m in forms:  # (alternating: the forms share every drift of the clocks)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                run(h, m, calls)
                e1.record(stream)
                stream.synchronize()
                t1 = time.perf_counter()
                if r >= a.warmup:
                    dev[name].append(e0.elapsed_time(e1) / calls)
                    wall[name].append((t1 - t0) * 1e3 / calls)
        say('(b) %d streams x %d frames, device pointers, %d calls per repeat, ms per call' % (B, T, calls))
        base = statistics.median(dev[forms[0][0]])
        for name, _, _ in forms:
            d, w = med_spread(dev[name]), med_spread(wall[name])
            say('    %-46s device %.4f [%.4f .. %.4f] (%+.1f %%)   wall %.4f [%.4f .. %.4f]' %
                ((name,) + d + ((d[0] / base - 1) * 100,) + w))
        for _, h in hs:
            h.set_stream(0)
            h.delete()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
