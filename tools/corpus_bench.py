"""
GPU: what per-frame stream resets cost and what they buy (include/pv_koala_batch.h, pv_koala_batch_process_chunk_resets; koala_amd/corpus.py).

 (a) the call with resets against the plain pv_koala_batch_process_chunk at 4096 streams x 64 frames, bf16 and fp32, device pointers: every
     stream resets once at a random frame of every call.  The two calls alternate on the engine's stream after bench.py's priming and
     warm-up, and each is timed with HIP events around it.
 (b) a ragged corpus -- log-normal lengths (median 6 s, clipped to 1-60 s) cut from synthetic streams (koala_amd.workload.synth_streams) --
     through 4096 slots x 64 frames in bf16, device mode.  Three figures side by side: useful frames/s (utterance frames / wall time), the
     padded-to-longest figure (one stream per file, every file zero-padded to the longest: the equal-length rate x the useful share) and
     the equal-length figure (the plain call of (a)).
 (c) the same corpus in async host mode (three page-locked buffer pairs; the numpy gathers and scatters of every call are on the host).

Writes profiles/r07_corpus.txt (or --out).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--prime-seconds', type=float, default=0.5)
    ap.add_argument('--utterances', type=int, default=20000)
    ap.add_argument('--no-async', action='store_true')
    ap.add_argument('--no-corpus', action='store_true', help='(a) only (e.g. under rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r07_corpus.txt'))
    a = ap.parse_args()

    import torch

    import koala_amd
    from koala_amd import corpus, params
    from koala_amd.workload import synth_streams

    B, T = a.streams, a.frames
    model = params.ensure_params(os.path.join(ROOT, 'build', 'adaptive_v4.kns'), 'adaptive', 1234)
    lines = ['# tools/corpus_bench.py on %s (%s)' % (torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d')),
             '# model: the default (adaptive-gate-v4); device pointers; HIP events on the engine stream', '']

    def log(s):
        print(s, flush=True)
        lines.append(s)

    # ---- (a)
    log('(a) %d streams x %d frames: plain call vs call with resets (every stream resets once per call at a random frame)' % (B, T))
    rng = np.random.default_rng(1)
    eq_rate = {}
    for precision in ('bf16', 'fp32'):
        kb = koala_amd.create_batch('key', B, T, precision, model_path=model)
        stream = torch.cuda.Stream()  # (the engine on a stream of torch's: the events below bracket its calls)
        torch.cuda.set_stream(stream)
        kb.set_stream(stream.cuda_stream)
        x = torch.from_numpy(synth_streams(B, T, seed=3)).cuda()
        y = torch.empty_like(x)
        masks = []
        for _ in range(8):
            m = np.zeros((B, T), np.uint8)
            m[np.arange(B), rng.integers(0, T, B)] = 1
            masks.append(m)

        def plain():
            kb.process_device(T, x.data_ptr(), y.data_ptr())

        def resets(i=[0]):
            i[0] += 1
            kb.process_device_resets(T, x.data_ptr(), y.data_ptr(), masks[i[0] % len(masks)])

        t_end = time.perf_counter() + a.prime_seconds
        while time.perf_counter() < t_end:
            plain()
            resets()
            torch.cuda.synchronize()
        for _ in range(a.warmup):
            plain()
            resets()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4 * a.steps)]
        for s in range(a.steps):
            for j, fn in enumerate((plain, resets)):
                e0, e1 = ev[2 * s + j]
                e0.record(stream)
                fn()
                e1.record(stream)
        torch.cuda.synchronize()
        tp = np.array([ev[2 * s][0].elapsed_time(ev[2 * s][1]) for s in range(a.steps)])
        tr = np.array([ev[2 * s + 1][0].elapsed_time(ev[2 * s + 1][1]) for s in range(a.steps)])
        kb.set_stream(0)
        kb.delete()
        torch.cuda.set_stream(torch.cuda.default_stream())
        eq_rate[precision] = B * T / (np.median(tp) * 1e-3)
        log('  %s  plain %.3f ms (median of %d; min %.3f)  resets %.3f ms (min %.3f)  cost %+.2f %%  plain %.1f M frames/s  resets %.1f M frames/s'
            % (precision, np.median(tp), a.steps, tp.min(), np.median(tr), tr.min(), 100 * (np.median(tr) / np.median(tp) - 1),
               eq_rate[precision] / 1e6, B * T / (np.median(tr) * 1e-3) / 1e6))
    log('')

    if a.no_corpus:
        return
    # ---- (b), (c)
    rng = np.random.default_rng(7)
    n = a.utterances
    secs = np.clip(rng.lognormal(np.log(6.0), 0.6, n), 1.0, 60.0)
    lengths = np.rint(secs * 16000).astype(np.int64)
    pool_rows = 64
    pool = synth_streams(pool_rows, int(np.ceil(lengths.max() / 256)) + 1, seed=11)
    off = rng.integers(0, pool.shape[1] - lengths.max() + 1, n) if pool.shape[1] > lengths.max() else np.zeros(n, np.int64)
    signals = [pool[i % pool_rows, off[i]:off[i] + lengths[i]] for i in range(n)]
    useful = int(np.sum((lengths + 255) // 256))
    plan = corpus.plan_corpus(lengths, B, T)
    laid = int(plan.frames.sum())
    log('(b) ragged corpus: %d utterances, %.0f s of audio (median %.1f s, mean %.1f s, longest %.1f s), %d slots x %d frames, bf16, device mode'
        % (n, lengths.sum() / 16000, np.median(secs), secs.mean(), secs.max(), B, T))
    log('  plan: %d calls, %d useful frames (+%d flush frames), slot occupancy %.1f %%'
        % (plan.num_calls, useful, laid - useful, 100.0 * laid / (plan.num_calls * B * T)))
    kb = koala_amd.create_batch('key', B, T, 'bf16', model_path=model)
    corpus.enhance_corpus(kb, signals[:B], T, 'device')  # (warm-up: kernels loaded, clocks up)
    torch.cuda.synchronize()
    table = corpus.corpus_table(signals, plan)
    t0 = time.perf_counter()
    corpus.enhance_corpus(kb, signals, T, 'device', plan=plan, table=table)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rate = useful / wall
    padded = eq_rate['bf16'] * useful / (n * ((lengths.max() + 255) // 256))
    log('  wall %.3f s (the corpus upload, the calls with their gathers / scatters, the download and trimming of the result; not the host'
        ' table of the corpus, built before)' % wall)
    log('  useful frames/s  %.1f M  |  padded-to-longest %.1f M (equal-length rate x useful share %.1f %%)  |  equal-length %.1f M  ->  %.1f %% of equal-length'
        % (rate / 1e6, padded / 1e6, 100.0 * useful / (n * ((lengths.max() + 255) // 256)), eq_rate['bf16'] / 1e6, 100 * rate / eq_rate['bf16']))
    # the GPU side alone: the device mode's loop of calls (gather, call with resets, scatter) on a resident corpus, HIP events around it
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    kb.set_stream(stream.cuda_stream)
    tab = torch.from_numpy(table).cuda()
    res = torch.zeros_like(tab)
    src = torch.from_numpy(plan.src.astype(np.int64)).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for c in range(plan.num_calls):
        x = tab[src[c]].reshape(B, T * 256)
        y = torch.empty_like(x)
        kb.process_device_resets(T, x.data_ptr(), y.data_ptr(), plan.reset[c])
        res[src[c].reshape(-1)] = y.reshape(B * T, 256)
    e1.record(stream)
    torch.cuda.synchronize()
    gpu_s = e0.elapsed_time(e1) * 1e-3
    kb.set_stream(0)
    torch.cuda.set_stream(torch.cuda.default_stream())
    del tab, res, src
    log('  GPU side alone (the %d calls with their gathers / scatters, corpus resident): %.3f s, useful frames/s %.1f M = %.1f %% of equal-length;'
        ' lower bound of the plan: %d calls x the plain call = %.1f M frames/s'
        % (plan.num_calls, gpu_s, useful / gpu_s / 1e6, 100 * useful / gpu_s / eq_rate['bf16'], plan.num_calls,
           useful / (plan.num_calls * B * T / eq_rate['bf16']) / 1e6))
    log('  makespan: the longest utterance is %d frames, the mean load per slot %.0f frames -- the plan cannot be shorter than %d calls'
        % (int(plan.frames.max()), laid / B, int(np.ceil(plan.frames.max() / T))))
    log('')
    if not a.no_async:
        t0 = time.perf_counter()
        corpus.enhance_corpus(kb, signals, T, 'async', plan=plan, table=table)
        wall = time.perf_counter() - t0
        log('(c) the same corpus, async host mode: wall %.3f s, useful frames/s %.1f M (host-side numpy gathers / scatters included)'
            % (wall, useful / wall / 1e6))
    kb.delete()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
