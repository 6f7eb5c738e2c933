// device_util.h -- three fragments that the query kernels share: device code, no arithmetic that rounds.
#pragma once
#include <hip/hip_runtime.h>

namespace nbody {

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000ll); }

// the live rows of a shard among its n_upper: *count is never negative in a valid handle, the clamp only keeps a kernel
// inside its arrays whatever the word holds
__device__ __forceinline__ int live_count(const int* __restrict__ count, int n_upper) { return max(0, min(*count, n_upper)); }

// the sum of v over the wave into *total (an integer: the order cannot show); every lane of the wave calls it
__device__ __forceinline__ void wave_add(unsigned long long v, unsigned long long* total) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (threadIdx.x % 64 == 0 && v) atomicAdd(total, v);
}

}  // namespace nbody
