"""
Multi-GPU host logic: streams are independent, so a job of N streams is cut into contiguous
per-rank ranges (or, for a ragged corpus of utterances, balanced by duration: balanced_assignment), one process and one engine per GPU, and nothing crosses GPUs on the data path.  The only
collective is the final reduction of {frames processed (sum), elapsed seconds (max)} for the aggregate rate.
"""

import heapq
from typing import List, Optional, Sequence, Tuple

import numpy as np


def shard_range(num_streams: int, rank: int, world_size: int) -> Tuple[int, int]:
    """Contiguous [begin, end) of the streams owned by `rank`; sizes differ by at most one."""
    if world_size <= 0 or not 0 <= rank < world_size:
        raise ValueError("bad rank/world_size")
    base, extra = divmod(num_streams, world_size)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def balanced_assignment(durations: Sequence[float], world_size: int) -> List[List[int]]:
    """
    Utterances of a ragged corpus onto `world_size` ranks by duration, longest-processing-time first: each utterance, longest first
    (ties: lower index first), goes to the rank with the least audio so far (ties: lower rank).  Returns per rank the ascending list of
    its utterance indices.  Deterministic; ranks may be empty when there are fewer utterances than ranks.  (`shard_range` cuts by
    stream COUNT: on a ragged corpus the rank holding the longest files would set the wall time.)
    """
    if world_size <= 0:
        raise ValueError("bad world_size")
    d = np.asarray(durations, dtype=np.float64).reshape(-1)
    if d.size and (not np.all(np.isfinite(d)) or d.min() < 0):
        raise ValueError("durations must be finite and non-negative")
    order = np.lexsort((np.arange(d.size), -d))  # longest first, then by index
    heap = [(0.0, r) for r in range(world_size)]
    ranks: List[List[int]] = [[] for _ in range(world_size)]
    for i in order:
        load, r = heapq.heappop(heap)
        ranks[r].append(int(i))
        heapq.heappush(heap, (load + float(d[i]), r))
    return [sorted(x) for x in ranks]


def aggregate_throughput(frames_local: int, elapsed_local: float, device: Optional[str] = None) -> Tuple[int, float]:
    """
    All-reduce of the per-rank counters: returns (total frames over all ranks, slowest rank's elapsed seconds).
    Uses the default torch.distributed group (backend `nccl` = RCCL over xGMI on GPUs, `gloo` on CPU); a
    run without a process group passes through unchanged.
    """
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return int(frames_local), float(elapsed_local)
    # (a one-rank group still goes through the collective: `torchrun --nproc-per-node 1` on a single-GPU box is how the RCCL
    # branch -- communicator creation on the device, all-reduce of device tensors -- gets executed at all)
    dev = device or ("cuda" if dist.get_backend() == "nccl" else "cpu")
    frames = torch.tensor([frames_local], dtype=torch.int64, device=dev)
    elapsed = torch.tensor([elapsed_local], dtype=torch.float64, device=dev)
    dist.all_reduce(frames, op=dist.ReduceOp.SUM)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    return int(frames.item()), float(elapsed.item())


__all__ = ["shard_range", "balanced_assignment", "aggregate_throughput"]
