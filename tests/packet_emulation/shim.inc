// Host stand-ins for what koala_amd/csrc/kns_packet.hip uses of HIP: a workgroup is 256 OS threads, __syncthreads a barrier, LDS a static
// array (one workgroup runs at a time).  tests/test_packet_kernels_cpu.py puts this file, the two argument structs of kns_kernels.h, the
// kernels of kns_packet.hip and driver.inc into one translation unit and runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <thread>
#include <algorithm>
#include <pthread.h>
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct Idx { int x; };
static thread_local Idx threadIdx;
static Idx blockIdx;
static pthread_barrier_t bar;
static void __syncthreads() { pthread_barrier_wait(&bar); }
using std::min;
