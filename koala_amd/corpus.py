"""
Many independent utterances through one batch handle (include/pv_koala_batch.h, pv_koala_batch_process_chunk_resets): every stream of
the handle is a SLOT that plays one utterance after the other, and a slot whose utterance ends inside a call starts the next one at the
following frame with a per-frame stream reset -- no zero-padding to the longest file, no call cut at utterance boundaries.

  plan_corpus     pure numpy: which frame of which utterance every (call, slot, frame) processes, and the reset mask
  enhance_corpus  runs a plan on a KoalaBatch (modes `host`, `async`, `device`) and returns one trimmed int16 array per utterance
  process_split   the reference meaning of one call with resets: the call cut at its reset frames into sub-calls with masked resets
                  between them (works on anything with process() and reset(mask), the CPU oracle included)

Layout: utterance u of n samples takes ceil(n / 256) + 1 frames -- its samples zero-padded to whole frames, then one zero FLUSH frame
(delay_sample = 256: the engine's output lags its input by one frame) -- stored back to back in a corpus frame table of
`total_frames` frames plus one zero frame at the end, which idle slots read.
"""

import heapq
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

FRAME = 256


class CorpusPlan(NamedTuple):
    src: np.ndarray      # int32 [calls, slots, T]: corpus frame processed by (call, slot, frame); zero_frame where the slot is idle
    reset: np.ndarray    # uint8 [calls, slots, T]: 1 at the first frame of every utterance in its slot
    offsets: np.ndarray  # int64 [N]: first corpus frame of utterance u (utterances stored in index order)
    frames: np.ndarray   # int64 [N]: frames of utterance u, ceil(n / 256) + 1
    slot: np.ndarray     # int64 [N]: the slot that plays utterance u
    start: np.ndarray    # int64 [N]: frame of the slot's timeline (call * T + frame) at which utterance u starts
    zero_frame: int      # index of the zero frame = total frames of the corpus

    @property
    def num_calls(self) -> int:
        return int(self.src.shape[0])


def utterance_frames(lengths: Sequence[int]) -> np.ndarray:
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("utterance lengths must be non-negative")
    return (n + FRAME - 1) // FRAME + 1


def plan_corpus(lengths: Sequence[int], num_slots: int, frames_per_call: int, order: str = 'longest') -> CorpusPlan:
    """Lays utterances of `lengths` samples out over `num_slots` slots and calls of `frames_per_call` frames.  Each utterance goes, as a
    whole, to the slot that becomes free first (ties: the lower slot) and starts there at the next frame; `order` = 'longest' takes the
    longest utterances first (ties: lower index), which keeps the drain at the end short -- the last utterances to start are the shortest --
    and 'given' takes them in index order."""
    if num_slots <= 0 or frames_per_call <= 0:
        raise ValueError("num_slots and frames_per_call must be positive")
    nf = utterance_frames(lengths)
    N, T = nf.size, int(frames_per_call)
    offsets = np.zeros(N, np.int64)
    if N:
        offsets[1:] = np.cumsum(nf)[:-1]
    F = int(nf.sum())
    if order == 'longest':
        seq = np.lexsort((np.arange(N), -nf))
    elif order == 'given':
        seq = np.arange(N)
    else:
        raise ValueError("order must be 'longest' or 'given'")
    slot = np.zeros(N, np.int64)
    start = np.zeros(N, np.int64)
    free = [(0, s) for s in range(num_slots)]  # (first free frame, slot)
    for u in seq:
        at, s = heapq.heappop(free)
        slot[u], start[u] = s, at
        heapq.heappush(free, (at + int(nf[u]), s))
    span = int((start + nf).max()) if N else 0
    calls = max(1, (span + T - 1) // T)
    src = np.full((num_slots, calls * T), F, np.int32)
    reset = np.zeros((num_slots, calls * T), np.uint8)
    if N:
        owner = np.repeat(np.arange(N), nf)                       # utterance of corpus frame f
        src[slot[owner], start[owner] + (np.arange(F) - offsets[owner])] = np.arange(F, dtype=np.int32)
        reset[slot, start] = 1
    src = np.ascontiguousarray(src.reshape(num_slots, calls, T).transpose(1, 0, 2))
    reset = np.ascontiguousarray(reset.reshape(num_slots, calls, T).transpose(1, 0, 2))
    return CorpusPlan(src, reset, offsets, nf, slot, start, F)


def corpus_table(signals: Sequence[np.ndarray], plan: CorpusPlan) -> np.ndarray:
    """int16 [total_frames + 1, 256]: every utterance zero-padded to its frames, back to back; the last row is the zero frame."""
    table = np.zeros((plan.zero_frame + 1, FRAME), np.int16)
    flat = table.reshape(-1)
    for u, x in enumerate(signals):
        x = np.asarray(x, dtype=np.int16).reshape(-1)
        o = int(plan.offsets[u]) * FRAME
        flat[o:o + x.size] = x
    return table


def trim(out_table: np.ndarray, signals: Sequence[np.ndarray], plan: CorpusPlan, delay_sample: int = FRAME) -> List[np.ndarray]:
    """One int16 array per utterance: its frames' output from `delay_sample` on, as long as its input."""
    flat = np.asarray(out_table).reshape(-1)
    res = []
    for u, x in enumerate(signals):
        o = int(plan.offsets[u]) * FRAME + delay_sample
        res.append(flat[o:o + len(x)].copy())
    return res


def process_split(proc, pcm: np.ndarray, reset: Optional[np.ndarray]) -> np.ndarray:
    """The meaning of one call with per-frame stream resets: pcm int16 [streams, T * 256] cut at every frame where some stream resets into
    consecutive sub-calls of proc.process(), with proc.reset(mask of the streams that reset there) in front of each."""
    S = pcm.shape[0]
    T = pcm.shape[1] // FRAME
    out = np.empty_like(pcm)
    r = np.zeros((S, T), np.uint8) if reset is None else np.asarray(reset, np.uint8).reshape(S, T)
    cuts = sorted(set([0, T] + [int(t) for t in np.nonzero(r.any(axis=0))[0]]))
    for a, b in zip(cuts[:-1], cuts[1:]):
        if r[:, a].any():
            proc.reset((r[:, a] != 0).astype(np.uint8))
        out[:, a * FRAME:b * FRAME] = proc.process(np.ascontiguousarray(pcm[:, a * FRAME:b * FRAME]))
    return out


def enhance_corpus(batch, signals: Sequence[np.ndarray], frames_per_call: int, mode: str = 'device',
                   plan: Optional[CorpusPlan] = None, table: Optional[np.ndarray] = None, report: bool = False):
    """Enhances every utterance of `signals` (int16 arrays of any length) on `batch` (a KoalaBatch whose streams are the slots, opened
    with max_frames_per_call >= frames_per_call) and returns one trimmed int16 array per utterance.  Modes:
      host    synchronous host calls (process_resets)
      async   three page-locked buffer pairs in rotation (process_async_resets): gathering call n + 3 runs beside calls n .. n + 2
      device  the corpus uploaded once as a torch int16 [frames + 1, 256] tensor; each call's input gathered and its output scattered
              by frame index on the GPU, on torch's current stream (no per-call host copy of audio)
    The handle's streams need no reset before: every slot's first utterance starts with one.  `plan` / `table`: a plan_corpus() of the
    signals' lengths and its corpus_table(), when the caller has them already.
    report=True: returns (arrays, reports), reports[u] = float32 [frames of u, 4], the frame report (koala_amd/report.py) of utterance u's
    own frames and its flush frame -- what the same file reports when it is run alone from a fresh stream."""
    T = int(frames_per_call)
    if T > batch.max_frames_per_call:
        raise ValueError("frames_per_call %d exceeds the handle's max_frames_per_call %d" % (T, batch.max_frames_per_call))
    S = batch.num_streams
    if plan is None:
        plan = plan_corpus([len(x) for x in signals], S, T)
    if plan.src.shape[1:] != (S, T):
        raise ValueError("plan shape %r does not match %d slots x %d frames" % (plan.src.shape[1:], S, T))
    if table is None:
        table = corpus_table(signals, plan)
    rep = np.zeros((table.shape[0], 4), np.float32) if report else None  # by corpus frame, like `out`
    if mode == 'host':
        out = np.zeros_like(table)
        for c in range(plan.num_calls):
            idx = plan.src[c]
            if report:
                y, r = batch.process_call(table[idx].reshape(S, T * FRAME), reset=plan.reset[c], report=True)
                rep[idx] = r
            else:
                y = batch.process_resets(table[idx].reshape(S, T * FRAME), plan.reset[c])
            out[idx] = y.reshape(S, T, FRAME)
    elif mode == 'async':
        out = np.zeros_like(table)
        pins = [(batch.alloc_host(T), batch.alloc_host(T)) for _ in range(3)]
        rpins = [batch.alloc_host_report(T) for _ in range(3)] if report else None

        def collect(c):
            out[plan.src[c]] = pins[c % 3][1].reshape(S, T, FRAME)
            if report:
                rep[plan.src[c]] = rpins[c % 3]

        for c in range(plan.num_calls):
            if c >= 3:
                batch.wait(2)  # call c - 3 has completed: its pair is free
                collect(c - 3)
            pin_in, pin_out = pins[c % 3]
            np.take(table, plan.src[c], axis=0, out=pin_in.reshape(S, T, FRAME))
            if report:
                batch.process_async_call(pin_in, pin_out, report=rpins[c % 3], reset=plan.reset[c])
            else:
                batch.process_async_resets(pin_in, pin_out, plan.reset[c])
        batch.wait(0)
        for c in range(max(0, plan.num_calls - 3), plan.num_calls):
            collect(c)
    elif mode == 'device':
        import torch
        dev = torch.device('cuda')
        tab = torch.from_numpy(table).to(dev)
        res = torch.zeros_like(tab)
        rres = torch.zeros((table.shape[0], 4), dtype=torch.float32, device=dev) if report else None
        src = torch.from_numpy(plan.src.astype(np.int64)).to(dev)
        # one stream of its own for torch's gathers / scatters and the engine's kernels, in order (torch's default stream is the null
        # stream, which the engine cannot be put on: set_stream(0) means the handle's own stream)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        batch.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                for c in range(plan.num_calls):
                    idx = src[c]
                    x = tab[idx].reshape(S, T * FRAME)
                    y = torch.empty_like(x)
                    if report:
                        r = torch.empty((S, T, 4), dtype=torch.float32, device=dev)
                        batch.process_device_call(T, x.data_ptr(), y.data_ptr(), r.data_ptr(), reset=plan.reset[c])
                        rres[idx.reshape(-1)] = r.reshape(S * T, 4)
                    else:
                        batch.process_device_resets(T, x.data_ptr(), y.data_ptr(), plan.reset[c])
                    res[idx.reshape(-1)] = y.reshape(S * T, FRAME)
                out = res.cpu().numpy()
                if report:
                    rep = rres.cpu().numpy()
        finally:
            batch.set_stream(0)
    else:
        raise ValueError("mode must be 'host', 'async' or 'device'")
    enhanced = trim(out, signals, plan, batch.delay_sample)
    if not report:
        return enhanced
    return enhanced, [rep[int(o):int(o) + int(n)].copy() for o, n in zip(plan.offsets, plan.frames)]


__all__ = ['CorpusPlan', 'plan_corpus', 'utterance_frames', 'corpus_table', 'trim', 'process_split', 'enhance_corpus']
