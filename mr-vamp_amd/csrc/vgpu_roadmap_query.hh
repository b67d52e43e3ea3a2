// vgpu_roadmap_query.hh -- the host driver interface of the roadmap query kernels (vgpu_roadmap_query.hip),
// called by the C ABI wrappers in vgpu_api.cpp, which own the context.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vgpu {

// a context's query workspace: grow-only device scratch, the pinned word the round totals are read from, and
// the last call's counters (rounds, slots relaxed, frontier items, host reads)
struct QueryState {
    void* dev = nullptr;
    size_t dev_bytes = 0;
    uint32_t* host = nullptr;  // pinned, 4 words
    uint64_t stats[4] = {0, 0, 0, 0};
};

// outcome of a driver: a VGPU_* code, the failing HIP call's error (code VGPU_ERR_HIP) and a message
struct QueryStatus {
    int code = 0;
    hipError_t hip = hipSuccess;
    const char* msg = "";
};

QueryStatus query_sssp(QueryState& q, uint32_t n, const unsigned long long* offsets, const uint32_t* adj,
                       const float* w, const uint32_t* sources, const uint32_t* limits, uint32_t S, float* g,
                       uint32_t* hops, uint32_t* parent, hipStream_t st);
QueryStatus query_bottleneck(QueryState& q, uint32_t n, const unsigned long long* offsets, const uint32_t* adj,
                             const uint32_t* sources, uint32_t S, uint32_t* b, hipStream_t st);
QueryStatus query_extract(const uint32_t* parent, uint32_t n, const uint32_t* targets, uint32_t S, uint32_t cap,
                          uint32_t* idx, uint32_t* len, hipStream_t st);
void query_free(QueryState& q);

}  // namespace vgpu
