// vgpu_rrtc.hh -- arguments of the batched RRT-Connect kernels (vgpu_rrtc.hip: one environment per call, or one per
// problem), shared with the driver in vgpu_api.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vamp_gpu.h"
#include "vgpu_device.hh"

namespace vgpu {

// per-problem control words (ctl[p * kRrtcWords + ...]): what a problem carries from one launch to the next.
// The sampler's index lives in the caller's rng_index[p], the trees in the arena.
enum : uint32_t {
    RC_PHASE = 0,    // RPH_*
    RC_NODES = 1,    // parents.size()
    RC_SIZE0 = 2,    // start_tree.size()
    RC_SIZE1 = 3,    // goal_tree.size()
    RC_A = 4,        // which tree is tree_a (0 start, 1 goal): tree_a_is_start = (RC_A == 0)
    RC_ITER_LO = 5,  // iter, 64 bits
    RC_ITER_HI = 6,
    kRrtcWords = 8
};
enum : uint32_t { RPH_NEW = 0, RPH_SEARCH = 1, RPH_DONE = 2 };

struct RrtcArgs {
    const float* starts;  // [P][7]
    const float* goals;   // [P][n_goals][7]
    uint64_t* rng;        // [P] next draw of each problem's sampler, in and out
    // the arena: per problem node_cap nodes, in insertion order (index = position in the CPU's buffer)
    float* nodes;      // [P][node_cap][7]
    uint32_t* parent;  // [P][node_cap]
    float* radius;     // [P][node_cap] dynamic-domain radius
    uint8_t* tree;     // [P][node_cap] 0 start tree, 1 goal tree
    uint32_t* ctl;     // [P][kRrtcWords]
    float* paths;      // [P][path_cap][7]
    uint32_t* path_len;
    vgpu_plan_result* results;
    uint8_t* status;  // may be null
    uint32_t P, n_goals, node_cap, path_cap;
    uint32_t max_nodes;    // min(settings.max_samples, node_cap)
    uint32_t cap_limited;  // node_cap < settings.max_samples
    uint32_t slice;        // iterations per problem and launch
    uint64_t max_iterations;
    float range, radius0, alpha, min_radius, tree_ratio;
    int32_t dynamic_domain, balance, start_tree_first;
    float bx, by, bz;
};

}  // namespace vgpu

extern "C" {
// totals[5] (device, zero before the first launch, as the control words: RPH_NEW = 0): [0] problems the last
// launch left unfinished, [1] iterations summed over the finished problems, [2] the largest iteration count of
// one problem, [3] problems whose rng entry is 0 (the argument check; they do not run), [4] problems whose
// env_index entry is outside the view table (likewise; vgpu_launch_rrtc_scenes only).
// one slice of every unfinished problem; then totals -> host_totals[5] (pinned) and totals[0] = 0
hipError_t vgpu_launch_rrtc(const vgpu::RrtcArgs* a, const EnvView* env, unsigned long long* totals,
                            unsigned long long* host_totals, hipStream_t st);
// the same with one environment per problem: problem p searches in views[env_index[p]] (views: a device table of
// n_envs views, env_index: device [P]); ext: some view has a heightfield or a point cloud
hipError_t vgpu_launch_rrtc_scenes(const vgpu::RrtcArgs* a, const EnvView* views, const uint32_t* env_index,
                                   uint32_t n_envs, int ext, unsigned long long* totals,
                                   unsigned long long* host_totals, hipStream_t st);
}
