// Host stand-ins for what koala_amd/csrc/kns_resample.hip and kns_highband.hip use of HIP: a workgroup is 256 OS threads, __syncthreads a
// barrier, LDS a static array (one workgroup runs at a time).  tests/high_band_emulator.py puts this file, the sample-rate and high-band
// sections of kns_kernels.h, the kernels of both files (kns_highband.hip's inside a namespace of their own: both files have a to_pcm) and
// driver.inc into one translation unit and runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>
#include <thread>
#include <algorithm>
#include <pthread.h>
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define KNS_HD inline
struct Idx { int x; };
static thread_local Idx threadIdx;
static Idx blockIdx;
static pthread_barrier_t bar;
static void __syncthreads() { pthread_barrier_wait(&bar); }
using std::min;
namespace kns { constexpr int kFrame = 256; }
