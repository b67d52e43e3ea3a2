// vgpu_lean.hh -- the bookkeeping kernels of a validate step that do no collision work (vgpu_kernels.hip):
// the per-check scan of a staged pass with its totals, boundaries and plan, and the back-step item total.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// children class of every check of a staged pass (vgpu_<name>_staged_class), handed to staged_scan_kernel
struct StagedClassTable {
    uint8_t of[64];
};

// The back-step item total of a validate call: a device accumulator and ticket that are zero between calls (the
// kernel that sums leaves them so) and the pinned word the total is stored into.
struct ItemTotalArgs {
    unsigned long long* acc;
    uint32_t* ticket;
    unsigned long long* host_total;
};
constexpr unsigned kTailCountBlocks = 512;  // grid cap of the tail_counts kernels: two same-address atomics per block

#ifdef __HIPCC__
namespace vgpu {
// The end of a kernel that wrote cnt[0 .. n_edges): every thread of every block calls it once, with the sum of the
// counts it wrote.  Thread 0 of block 0 writes the count scan's last input cnt[n_edges]; each block adds its
// 64-bit sum with one atomic; the block whose ticket comes last stores the total into pinned memory and zeroes
// the accumulator and the ticket.  The add has returned before the ticket is taken, so the last ticket holder's
// exchange sees every block's add (all three are agent-scope read-modify-writes).
template <int BLOCK>
__device__ __forceinline__ void item_total_block(unsigned long long s, uint32_t* __restrict__ cnt, size_t n_edges,
                                                 const ItemTotalArgs& t)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n_edges] = 0u;
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    __shared__ unsigned long long part[BLOCK / 64];
    if (__lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long sum = 0;
    for (int w = 0; w < BLOCK / 64; ++w) sum += part[w];
    const unsigned long long before = __hip_atomic_fetch_add(t.acc, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(before) : "memory");
    if (__hip_atomic_fetch_add(t.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
    *t.host_total = __hip_atomic_exchange(t.acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace vgpu
#endif

extern "C" {
hipError_t vgpu_launch_item_total(uint32_t* cnt, size_t n, const ItemTotalArgs* t, hipStream_t st);
hipError_t vgpu_launch_staged_scan(const uint32_t* counts, uint32_t* offs, uint32_t nb, int checks, uint32_t* fired,
                                   uint32_t* bnd, uint32_t* ticket, uint32_t* host_fired, void* plan,
                                   const StagedClassTable* cls, uint64_t set, uint32_t W, uint32_t n_groups,
                                   hipStream_t st);
}
