// The scalar reduction of the pixel-side kernels, shared by temporal.hip, pixel_prior.hip and color.hip: ONE statement of
// the "last block by integer ticket" protocol, the only memory-ordering code of those files.  N sums of type T over a whole
// grid of 256-thread workgroups, the same bits on every run, no float atomics:
//   - every block reduces its threads' N values by a fixed tree (block_sum_256<T, N>) and thread 0 stores them j-major,
//     partials[j * gridDim.x + blockIdx.x];
//   - thread 0 fences (the partials are visible device-wide before the ticket moves) and takes a ticket, atomicAdd(ticket);
//   - the block that draws the last ticket fences again and sums the partials in a fixed order -- thread t adds partials
//     t, t + 256, ... of every j in ascending order, through agent-scope relaxed atomic loads (another block wrote them:
//     they must not come from a stale line), then the same tree -- and thread 0 stores out[j] = sum_j * scale and puts the
//     ticket back to 0 for the next launch on the stream.
// The workspace a caller hands in is {unsigned ticket (0 before the first launch), 12 bytes of padding, T partials[N * grid]}.
// Barriers: ALL 256 threads of EVERY block must call ticket_sum_256 (no thread may have returned before it): both barriers
// of the first block_sum_256 and the one that publishes *is_last are reached by all of them; the blocks that are not last
// return only behind those three.  *is_last is written by thread 0 before that third barrier and read behind it.
// Arithmetic: nothing here multiplies into an add (a += load; then a * scale), so the floating-point contraction mode of
// the including file (pixel_prior.hip compiles with contraction off, the others with it on) cannot change a bit.
#pragma once
#include "common.h"

// Block-wide sums of N values for blockDim.x == 256 (4 waves), in every thread; `red` is 4 x N values of LDS.  One barrier
// pair for all N; per value the tree of block_sum_256(float, float*): a fixed shuffle tree, the 4 waves in a fixed order.
template <class T, int N>
__device__ __forceinline__ void block_sum_256(T (&a)[N], T (*red)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = wave_sum(a[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[threadIdx.x >> 6][k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

template <class T, int N>
__device__ __forceinline__ void ticket_sum_256(T (&a)[N], T scale, T* __restrict__ out, unsigned* __restrict__ ticket,
                                               T* __restrict__ partials, T (*red)[N], int* is_last) {
  const unsigned nblocks = gridDim.x;
  block_sum_256(a, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) partials[(size_t)j * nblocks + blockIdx.x] = a[j];
    __threadfence();                                  // the partials are visible before the ticket is taken
    *is_last = atomicAdd(ticket, 1u) == nblocks - 1;
  }
  __syncthreads();
  if (!*is_last) return;
  __threadfence();
#pragma unroll
  for (int j = 0; j < N; ++j) a[j] = (T)0;
  for (unsigned i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      a[j] += __hip_atomic_load(&partials[(size_t)j * nblocks + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_sum_256(a, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = a[j] * scale;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
  }
}
