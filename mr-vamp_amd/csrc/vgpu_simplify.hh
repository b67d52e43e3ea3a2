// vgpu_simplify.hh -- arguments of the batched path-simplification kernels (vgpu_simplify.hip), shared with
// the driver in vgpu_api.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace vgpu {

// per-path control words (st[p * kSimplifyWords + ...]); the path's length lives in the caller's len[p]
enum : uint32_t {
    SP_PHASE = 0,    // what the path's next round validates (SPH_*)
    SP_ITER = 1,     // simplify.hh:243 result.iterations
    SP_OP = 2,       // index of the running operation in settings.operations
    SP_ANY = 3,      // simplify.hh:245 any
    SP_I = 4,        // shortcut_path's i
    SP_STEP = 5,     // smooth_bspline's step
    SP_CHANGED = 6,  // the running operation's return value so far
    SP_BUF = 7,      // which of the two waypoint buffers holds the path
    SP_STATUS = 8,   // VGPU_SIMPLIFY_*
    kSimplifyWords = 9
};
enum : uint32_t { SPH_DONE = 0, SPH_STRAIGHT = 1, SPH_SHORTCUT = 2, SPH_BSPLINE = 3 };

struct SimplifyArgs {
    float* buf[2];      // [n_paths][cap][dim]: the caller's waypoints and the ping-pong copy
    uint32_t* len;      // [n_paths]
    uint32_t* st;       // [n_paths][kSimplifyWords]
    uint32_t* cnt;      // [n_paths + 1] edges each path emits this round
    uint32_t* off;      // [n_paths + 1] their exclusive scan
    uint32_t* cand;     // [n_paths][cap] B-spline candidate indices of this round
    float* starts;      // [n_paths * cap][dim] the round's edge list
    float* goals;
    const uint8_t* ok;  // [n_paths * cap] its validate_motion results
    uint32_t* host;     // pinned: [0] the round's edge total, [1] paths still working
    uint32_t n_paths, cap, limit, dim;
    uint32_t max_iterations, max_steps, n_ops, ops[8];  // ops: 1 = shortcut, 0 = B-spline
    float min_change, midpoint;
};

}  // namespace vgpu

extern "C" {
hipError_t vgpu_launch_simplify_init(const vgpu::SimplifyArgs* a, hipStream_t st);
// one round: prepare (B-spline subdivide + candidates, per-path edge counts) and the counts' scan, which
// stores the totals into a->host
hipError_t vgpu_launch_simplify_prepare(const vgpu::SimplifyArgs* a, hipStream_t st);
hipError_t vgpu_launch_simplify_emit(const vgpu::SimplifyArgs* a, hipStream_t st);
hipError_t vgpu_launch_simplify_resolve(const vgpu::SimplifyArgs* a, hipStream_t st);
hipError_t vgpu_launch_simplify_finish(const vgpu::SimplifyArgs* a, uint32_t* iterations, uint8_t* status, float* cost,
                                       hipStream_t st);
}
