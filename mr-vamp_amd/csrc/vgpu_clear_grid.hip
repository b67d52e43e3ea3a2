// vgpu_clear_grid.hip -- the clearance grid of a primitive environment: per cell of a box around the obstacles,
// a lower bound of the distance from any point of the cell to the nearest obstacle surface.  The bound kernels
// that opt in (vgpu_staged.hh ClearKinds) look a sphere's centre up before scanning the records: a sphere whose
// radius is below its cell's bound touches nothing, so its lane drops out of the scans (vgpu_device.hh
// clear_lane).  It changes no answer.
//
// Cell value (uint8, saturating at 255; unit kClrStep = 1/512 m):
//     floor((d(centre) - half diagonal - margin - slack) / kClrStep),   0 when that is negative or NaN
// d(centre) is the exact distance from the cell centre to the nearest record -- sphere: |p - c| - r; capsule: the
// distance to the segment less r; cuboid (orthonormal axes): the box distance, 0 inside.  Distances are
// 1-Lipschitz, so every point of the cell is at least d(centre) - half diagonal away.  margin = 1 mm + 1e-5 of the
// box's extent separates "clear" from every value the reference's float tests could round to a collision; slack
// (2^-20 of the largest coordinate, ~16 float ulps) covers the float rounding of d(centre) itself, so the stored
// bound never exceeds the real-number formula without it.
// One thread per cell (storage order: 4 x 4 x 4 bricks, capt_cell_index), looping over the records in the device
// layout; 64^3 cells x 14 spheres take a few microseconds.
#include "vgpu_device.hh"

namespace vgpu {

constexpr int kClearBlock = 256;

__global__ __launch_bounds__(kClearBlock) void clear_grid_kernel(ClearGridArgs g)
{
    const uint32_t n = (uint32_t)g.nc;
    const uint32_t cell = blockIdx.x * (uint32_t)kClearBlock + threadIdx.x;
    if (cell >= n * n * n) return;
    // the cell stored at index `cell` (the inverse of capt_cell_index, bricks)
    const uint32_t b = cell >> 6, l = cell & 63u, nb = n >> 2;
    const uint32_t ix = (b % nb) * 4u + (l & 3u);
    const uint32_t iy = ((b / nb) % nb) * 4u + ((l >> 2) & 3u);
    const uint32_t iz = (b / (nb * nb)) * 4u + (l >> 4);
    const float x = g.lo[0] + ((float)ix + 0.5f) * g.h[0];
    const float y = g.lo[1] + ((float)iy + 0.5f) * g.h[1];
    const float z = g.lo[2] + ((float)iz + 0.5f) * g.h[2];
    float d = __builtin_inff();
    {  // spheres: pair blocks md_a md_b x_a x_b y_a y_b z_a z_b r_a r_b
        const VGPU_CONST float* o = g.obs[OBS_SPHERE];
        for (int i = 0; i < g.n[OBS_SPHERE]; ++i) {
            const VGPU_CONST float* p = o + (size_t)(i >> 1) * kSphereBlock + (i & 1);
            const float xs = x - p[2], ys = y - p[4], zs = z - p[6];
            d = fminf(d, __builtin_sqrtf(xs * xs + ys * ys + zs * zs) - p[8]);
        }
    }
    for (int t = OBS_CAPSULE; t <= OBS_ZCAPSULE; ++t) {  // md x1 y1 z1 xv yv zv r rdv
        const VGPU_CONST float* o = g.obs[t];
        for (int i = 0; i < g.n[t]; ++i, o += kObsStride[OBS_CAPSULE]) {
            const float vx = t == OBS_CAPSULE ? o[4] : 0.0f, vy = t == OBS_CAPSULE ? o[5] : 0.0f, vz = o[6];
            const float dot = (x - o[1]) * vx + (y - o[2]) * vy + (z - o[3]) * vz;
            const float cdf = fminf(fmaxf(dot * o[8], 0.0f), 1.0f);
            const float xs = x - (o[1] + vx * cdf), ys = y - (o[2] + vy * cdf), zs = z - (o[3] + vz * cdf);
            d = fminf(d, __builtin_sqrtf(xs * xs + ys * ys + zs * zs) - o[7]);
        }
    }
    for (int t = OBS_CUBOID; t <= OBS_ZCUBOID; ++t) {  // md x y z a1 a2 a3 r1 r2 r3
        const VGPU_CONST float* o = g.obs[t];
        for (int i = 0; i < g.n[t]; ++i, o += kObsStride[OBS_CUBOID]) {
            const float xs = x - o[1], ys = y - o[2], zs = z - o[3];
            float a1, a2, a3;
            if (t == OBS_CUBOID) {
                a1 = max0(__builtin_fabsf(o[4] * xs + o[5] * ys + o[6] * zs) - o[13]);
                a2 = max0(__builtin_fabsf(o[7] * xs + o[8] * ys + o[9] * zs) - o[14]);
                a3 = max0(__builtin_fabsf(o[10] * xs + o[11] * ys + o[12] * zs) - o[15]);
            } else {  // the z-cuboid's test reads a1, a2 in the xy plane and the z axis
                a1 = max0(__builtin_fabsf(o[4] * xs + o[5] * ys) - o[13]);
                a2 = max0(__builtin_fabsf(o[7] * xs + o[8] * ys) - o[14]);
                a3 = max0(__builtin_fabsf(zs) - o[15]);
            }
            d = fminf(d, __builtin_sqrtf(a1 * a1 + a2 * a2 + a3 * a3));
        }
    }
    const float hd = 0.5f * __builtin_sqrtf(g.h[0] * g.h[0] + g.h[1] * g.h[1] + g.h[2] * g.h[2]);
    const float q = __builtin_floorf((d - hd - g.margin - g.slack) * (1.0f / kClrStep));
    uint32_t v = 0u;
    if (q >= 1.0f) v = q >= 255.0f ? 255u : (uint32_t)q;  // NaN: 0
    g.out[cell] = (uint8_t)v;
}

}  // namespace vgpu

// g->out: nc^3 bytes; nc a multiple of 4
extern "C" hipError_t vgpu_launch_clear_grid(const ClearGridArgs* g, hipStream_t st)
{
    if (g->nc <= 0 || (g->nc & 3) || g->nc > 256 || !g->out) return hipErrorInvalidValue;
    const uint32_t cells = (uint32_t)g->nc * (uint32_t)g->nc * (uint32_t)g->nc;
    const dim3 grid((cells + vgpu::kClearBlock - 1) / vgpu::kClearBlock), block(vgpu::kClearBlock);
    hipLaunchKernelGGL(vgpu::clear_grid_kernel, grid, block, 0, st, *g);
    return hipGetLastError();
}
