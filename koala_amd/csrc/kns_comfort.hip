// kns_comfort.hip -- comfort noise (twelfth extension; section 6): the small launch in front of a call whose synthesis
// kernels fill what the mask removed with shaped noise (kns_stft.hip, synthesis_comfort_kernel).  The noise of a frame is a hash of the
// stream's seed, the bin and the stream's frame counter n_b, one uint32 of state per stream: counted only while the stream's comfort noise is
// on, 0 for a fresh stream, wrapping modulo 2^32.
//
// comfort_count_kernel: one lane per stream, sequential over the call's T frames.  It writes the counter value of every frame to n[b][t],
//   which the synthesis kernels read -- a segment of a launch that replays the frame in front of it finds that frame's value there -- and
//   the counter behind the call.  A per-frame reset makes n = 0 before its frame.  A held stream's row is written, since its frames are
//   synthesised like any other's, but its counter stays, whatever else the call's bytes say.  A stream whose comfort noise is off does not
//   count (its row reads 0, the kernels do not use it); a per-frame reset leaves its counter at 0 all the same, as pv_koala_batch_reset
//   does.  Rows past the last stream read 0.
// comfort_reset_kernel: the counters of the masked streams := 0.
// Plain HIP C++, vector loads and stores only.
#include "kns_kernels.h"

namespace kns {

__global__ __launch_bounds__(256) void comfort_count_kernel(ComfortArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.Bpad) return;
    uint32_t *row = a.n + (size_t) b * a.T;
    const uint8_t *ctl = a.ctl && b < a.B ? a.ctl + (size_t) b * (a.T + 1) : nullptr;
    if (b >= a.B || !a.set[b].on) {  // (off: no frame counts, but a reset is a reset -- like pv_koala_batch_reset, it leaves n = 0)
        bool restart = false;
        for (int t = 0; t < a.T; ++t) {
            row[t] = 0u;
            restart = restart || (ctl && ctl[1 + t]);
        }
        if (restart && !ctl[0]) a.state[b] = 0u;
        return;
    }
    uint32_t n = a.state[b];
    for (int t = 0; t < a.T; ++t) {
        if (ctl && ctl[1 + t]) n = 0u;
        row[t] = n;
        n = n + 1u;
    }
    if (!(ctl && ctl[0])) a.state[b] = n;
}

__global__ __launch_bounds__(256) void comfort_reset_kernel(uint32_t *state, const uint8_t *mask, int Bpad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= Bpad || (mask && !mask[b])) return;
    state[b] = 0u;
}

void launch_comfort(const ComfortArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(comfort_count_kernel, dim3((a.Bpad + 255) / 256), dim3(256), 0, s, a);
}

void launch_comfort_reset(uint32_t *state, const uint8_t *mask, int Bpad, hipStream_t s) {
    hipLaunchKernelGGL(comfort_reset_kernel, dim3((Bpad + 255) / 256), dim3(256), 0, s, state, mask, Bpad);
}

}  // namespace kns
