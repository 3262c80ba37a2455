// Host stand-ins for what koala_amd/csrc/kns_format.hip uses of HIP: its kernels have no LDS and no barrier, so a workgroup is a loop over
// 256 values of threadIdx.x.  uint4 is 16-byte aligned here, as on the device: the alignment check of the sanitizer build sees every vector
// load and store.  tests/test_format_kernels_cpu.py puts this file, the format section of kns_kernels.h, the kernels of kns_format.hip and
// driver.inc into one translation unit and runs it under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <vector>
struct alignas(16) uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define KNS_HD static inline
struct Idx { unsigned x; };
static Idx threadIdx, blockIdx;
