/* vamp_oracle.h -- CPU restatement of the reference motion-validation rake.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load this library, and only as the checker / the timed CPU
 * baseline.  The product (mr-vamp_amd/, libvampgpu.so) never links or calls it.
 *
 * Parity pin (see DESIGN.md "Oracle and parity"):
 *   - sin/cos, max_extent sqrt, l2_norm, rake construction, Halton: bit-exact against
 *     oracle/_ref/ref_probe built from the reference's own vector layer + halton.hh;
 *   - FK sphere centres and fkcc masks: against fixtures produced by evaluating the
 *     reference's generated fk.hh expression DAG (tools/fkhh_interp.py), FK within 1e-5,
 *     masks bit-exact on the margin-filtered set.  The reference fk.hh/validity.hh cannot
 *     be compiled here (Eigen/pdqsort absent), so that pin is "partial" by construction.
 */
#ifndef VAMP_ORACLE_H
#define VAMP_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Environment<float> (collision/environment.hh:12-82), each list sorted ascending by
 * min_distance.  Row layouts (float32):
 *   sphere  [5]  x y z r min_distance
 *   capsule [9]  x1 y1 z1 xv yv zv r rdv min_distance   (also z-aligned capsules)
 *   cuboid  [16] x y z a1x a1y a1z a2x a2y a2z a3x a3y a3z r1 r2 r3 min_distance */
/* HeightField<float> (collision/shapes.hh:250-312) as made by factory::heightfield::flat
 * (factory.hh:365-386): xs/ys/zs are the reciprocal scales; data row-major, xd*yd floats. */
typedef struct vo_heightfield {
    float x, y, z, xs, ys, zs;
    int xd, yd;
    const float *data;
} vo_heightfield;

/* CAPT (collision/capt.hh:91-398): the four arrays of the built tree.
 *   tests      [2^nlog2 - 1]      split values, implicit binary tree
 *   aabbs      [2^nlog2][6]       leaf Volume {lower xyz, upper xyz}
 *   aff_starts [2^nlog2 + 1]      affordance vector range per leaf
 *   aff        [n_aff][3][8]      affordance vectors (x8, y8, z8), +inf padded */
typedef struct vo_capt {
    int nlog2;
    float r_min, r_max, r_point;
    float aabb_top[6];
    float *tests;
    float *aabbs;
    uint32_t *aff_starts;
    float *aff;
    size_t n_aff;
} vo_capt;

typedef struct vo_env {
    int n_spheres, n_capsules, n_zcapsules, n_cuboids, n_zcuboids;
    const float *spheres, *capsules, *zcapsules, *cuboids, *zcuboids;
    int n_heightfields, n_pointclouds;
    const vo_heightfield *heightfields;
    const vo_capt *pointclouds;
} vo_env;

typedef struct vo_stats {
    double test_margin;   /* min |signed test value| over evaluated primitive tests */
    double cull_margin;   /* min |min_distance - max_extent| over evaluated cull tests */
    double flops;         /* executed floating-point operations (fma = 2) */
} vo_stats;

/* ---- vector-layer semantics (vector/interface.hh, vector/avx.hh) ---- */
float vo_sin(float x);                     /* interface.hh:438-456 as compiled (Horner/FMA) */
float vo_cos(float x);                     /* interface.hh:458-469 */
float vo_rsqrt_native(float x);            /* _mm_rsqrt_ss of this host (avx.hh:411-415) */
float vo_max_extent(float x, float y, float z, float r); /* validity.hh:55-59 */
float vo_l2_norm7(const float v[7]);       /* interface.hh:402-410 + avx.hh:441-452 */

/* Probe this host's rsqrt approximation as a table indexed by (exponent parity, top K
 * mantissa bits).  lut must hold 2 << 16 entries.  Returns 0 and sets *kbits on success,
 * <0 if the host's rsqrt is not such a table function (then the GPU path refuses to run). */
int vo_rsqrt_probe(uint32_t *lut, int *kbits);
/* sqrt emulated from a probed table (the GPU kernels' algorithm, for testing) */
float vo_sqrt_lut(float v, const uint32_t *lut, int kbits);

/* ---- shapes (collision/shapes.hh) ---- */
float vo_sphere_min_distance(float x, float y, float z, float r);              /* shapes.hh:238 */
float vo_cuboid_min_distance(const float c[15]);                               /* shapes.hh:52-67 */
float vo_capsule_min_distance(const float c[8]);                               /* shapes.hh:165-189 */

/* sphere_heightfield (sphere_heightfield.hh:9-30): signed test value, collision = sign bit.
 * *oob is set when the reference's gather index falls outside the data (undefined in the
 * reference; the GPU path reports a collision there). */
float vo_sphere_heightfield(const vo_heightfield *h, float x, float y, float z, float r, int *oob);

/* ---- CAPT (collision/capt.hh) ---- */
/* CAPT::CAPT(points, r_min, r_max, r_point) (capt.hh:327-398, subdivide :156-325).  points: n x 3.  Ties in a
 * split coordinate are ordered by point index (the reference's pdqsort_branchless leaves
 * their order unspecified).  Returns 0 on success; free with vo_capt_free. */
int vo_capt_build(const float *points, size_t n, float r_min, float r_max, float r_point, vo_capt *out);
void vo_capt_free(vo_capt *t);
/* CAPT::collides(center, r) (capt.hh:403-443) */
int vo_capt_collides(const vo_capt *t, const float c[3], float r, vo_stats *st);
/* one lane of CAPT::collides_simd (capt.hh:457-541): the result of the SIMD call is the OR
 * of this over the lanes */
int vo_capt_collides_lane(const vo_capt *t, const float c[3], float r, vo_stats *st);
/* batch of raw queries (centres n x 3, radii n); simd != 0 selects the per-lane collides_simd
 * semantics.  margin (optional, n) receives each query's smallest |comparison difference|. */
void vo_capt_collides_batch(const vo_capt *t, const float *centers, const float *radii, size_t n, int simd,
                            uint8_t *out, double *margin);

/* expression-level pins (ref_probe "sql2" / "capt_box"): collision::sql2_3 on FloatVector,
 * the collides_simd leaf-box distance (FloatVector clamp), Volume::distsq_to and the
 * contained_by_internal_ball sum (scalar) */
float vo_sql2_3(float ax, float ay, float az, float bx, float by, float bz);
/* scalar float sphere_sphere_sql2 (sphere_sphere.hh:20-22) as the release build contracts it (ref_probe
 * "sql2s"): fma(xs, xs, ys*ys) + fma(zs, zs, -(rs*rs)) */
float vo_sql2_scalar(float ax, float ay, float az, float ar, float bx, float by, float bz, float br);
float vo_capt_box_vec(const float c[3], const float lo[3], const float up[3]);
float vo_capt_vol_distsq(const float p[3], const float lo[3], const float up[3]);
float vo_capt_vol_ball(const float p[3], const float lo[3], const float up[3]);

/* ---- robots ---- */
/* robot ids (same values as the product's VGPU_ROBOT_*): Panda = PandaBase<X100,Y100,Z100>
 * (robots/panda_base.hh:15-75), Fetch (robots/fetch.hh:8-48, 8 dof, no base offset) */
#define VO_ROBOT_PANDA 1
#define VO_ROBOT_FETCH 2
#define VO_ROBOT_UR5 4    /* robots/ur5.hh: 6 dof */
#define VO_ROBOT_BAXTER 5 /* robots/baxter.hh: 14 dof dual arm, resolution 64 */
int vo_robot_dim(int robot);
int vo_robot_nspheres(int robot);
float vo_l2_norm(const float *v, int dim);                                   /* dim <= 16 */
void vo_robot_scale(int robot, float *q);                                    /* scale_configuration */
void vo_robot_sphere_fk(int robot, const float *q, int bx100, int by100, int bz100, float out_xyz[][3]);
/* filter_robot_from_pointcloud (bindings/common.hh:36-87): keep[i] = 1 when point i (radius
 * point_radius) overlaps no robot sphere at q and is clear of the environment */
void vo_robot_filter_pointcloud(int robot, const vo_env *env, const float *q, int bx100, int by100, int bz100,
                                const float *pc, size_t n, float point_radius, uint8_t *keep);
/* q is [G][dim]; returns 1 = valid */
int vo_robot_fkcc_block(int robot, const vo_env *env, const float *q, int G, int bx100, int by100, int bz100,
                        vo_stats *stats);
/* validate_vector with the caller's distance (planning/validate.hh:23-65; RRT-Connect's extension check) */
int vo_robot_validate_vector(int robot, const vo_env *env, const float *start, const float *vector, float distance,
                             int bx100, int by100, int bz100, int *n_out);
int vo_robot_validate_motion(int robot, const vo_env *env, const float *start, const float *goal, int bx100,
                             int by100, int bz100, int *n_out, vo_stats *stats);
void vo_robot_fkcc_configs(int robot, const vo_env *env, const float *q, size_t n, int bx100, int by100,
                           int bz100, uint8_t *valid, int threads);
void vo_robot_validate_motions(int robot, const vo_env *env, const float *starts, const float *goals,
                               size_t n_edges, int bx100, int by100, int bz100, uint8_t *ok, int32_t *n_out,
                               int threads);

/* Attachment<float> (collision/attachments.hh:14-123): spheres (x y z r) relative to a frame
 * tf = (x y z, qx qy qz qw) attached to the end effector (bindings/environment.cc:197-249). */
typedef struct vo_attachment {
    float tf[7];
    int n;
    const float *spheres;
} vo_attachment;
/* Robot::fkcc_attach (panda: robots/panda/fk.hh:6278-11397); returns -1 for robots without an
 * extracted attachment hierarchy */
int vo_robot_fkcc_attach_block(int robot, const vo_env *env, const vo_attachment *att, const float *q, int G,
                               int bx100, int by100, int bz100, vo_stats *stats);
/* validate_motion with env.attachments set: first block fkcc_attach, back-steps fkcc (validate.hh:43) */
int vo_robot_validate_motion_att(int robot, const vo_env *env, const vo_attachment *att, const float *start,
                                 const float *goal, int bx100, int by100, int bz100, int *n_out, vo_stats *stats);
void vo_robot_fkcc_attach_configs(int robot, const vo_env *env, const vo_attachment *att, const float *q, size_t n,
                                  int bx100, int by100, int bz100, uint8_t *valid, int threads);
void vo_robot_validate_motions_att(int robot, const vo_env *env, const vo_attachment *att, const float *starts,
                                   const float *goals, size_t n_edges, int bx100, int by100, int bz100, uint8_t *ok,
                                   int32_t *n_out, int threads);

/* ---- Panda (robots/panda_base.hh, robots/panda/fk.hh): wrappers of the vo_robot_* calls ---- */
void vo_panda_scale(float q[7]);                                               /* fk.hh:34-37 */
void vo_panda_sphere_fk(const float q[7], int bx100, int by100, int bz100,
                        float out_xyz[][3]);                                    /* fk.hh:104-1333 */
/* fkcc on one block of G lanes (G = 8: a reference rake block; G = 1: a configuration
 * broadcast to all lanes, i.e. the per-configuration mask).  q is [G][7].
 * Returns 1 = valid (fk.hh:1335-6276 via robots/panda_base.hh:53-58). */
int vo_panda_fkcc_block(const vo_env *env, const float *q, int G, int bx100, int by100, int bz100,
                        vo_stats *stats);
/* validate_motion<Panda, 8, 32> (planning/validate.hh:23-75). *n_out = back-step count n. */
int vo_panda_validate_motion(const vo_env *env, const float start[7], const float goal[7],
                             int bx100, int by100, int bz100, int *n_out, vo_stats *stats);

/* the same, with the first rake block's work counted in *head and the back-steps in *tail */
int vo_panda_validate_motion_split(const vo_env *env, const float start[7], const float goal[7], int bx100,
                                   int by100, int bz100, int *n_out, vo_stats *head, vo_stats *tail);

/* batched, multi-threaded drivers (CPU baseline / fixture generation) */
void vo_panda_fkcc_configs(const vo_env *env, const float *q /*[N][7]*/, size_t n, int bx100,
                           int by100, int bz100, uint8_t *valid, int threads);
void vo_panda_validate_motions(const vo_env *env, const float *starts, const float *goals,
                               size_t n_edges, int bx100, int by100, int bz100, uint8_t *ok,
                               int32_t *n_out, int threads);

/* ---- two-Panda composite (BASELINE configs[4]; composed from reference primitives) ---- */
/* q is [G][14] = arm A joints 0..6, arm B joints 7..13; bases in centimetres.  Valid iff
 * fkcc_A && fkcc_B && no A-B sphere overlap (link-bounding pairs first, then their spheres). */
int vo_pair_fkcc_block(const vo_env *env, const float *q, int G, const int ba100[3], const int bb100[3],
                       vo_stats *stats);
int vo_pair_validate_vector(const vo_env *env, const float start[14], const float v[14], float distance,
                            const int ba100[3], const int bb100[3], int *n_out, vo_stats *st);
int vo_pair_validate_motion(const vo_env *env, const float start[14], const float goal[14], const int ba100[3],
                            const int bb100[3], int *n_out, vo_stats *stats);
void vo_pair_fkcc_configs(const vo_env *env, const float *q, size_t n, const int ba100[3], const int bb100[3],
                          uint8_t *valid, int threads);
void vo_pair_validate_motions(const vo_env *env, const float *starts, const float *goals, size_t n_edges,
                              const int ba100[3], const int bb100[3], uint8_t *ok, int32_t *n_out, int threads);

/* ---- Halton (random/halton.hh:73-104), closed form ---- */
/* Sample with 1-based draw index k (k-th call to next()) of Halton<dim>, dim <= 16. */
void vo_halton(int dim, uint64_t k, float *out);

/* ---- PRM roadmap edge stage (planning/prm.hh:235-283, roadmap.hh:42-77, nn.hh:53-57) ---- */
size_t vo_prm_max_neighbors(int dim, size_t num_states);
float vo_prm_neighbor_radius(int dim, double space_measure, double gamma_scale, size_t num_states);
float vo_config_distance(const float *a, const float *b, int dim);
void vo_roadmap_knn(int dim, const float *V, size_t n, double space_measure, double gamma_scale, uint32_t kmax,
                    uint32_t *nbr, float *dist, uint32_t *cnt, int threads);
/* The same loop with caller-chosen parameters: k[n], r[n] indexed by vertex (k clamped to kmax), row j of
 * nbr[m][kmax], dist, cnt answers vertex queries[j] (NULL: vertex j) against the vertices before it. */
void vo_roadmap_knn_kr(int dim, const float *V, size_t n, const uint32_t *queries, size_t m, const uint32_t *k,
                       const float *r, uint32_t kmax, uint32_t *nbr, float *dist, uint32_t *cnt, int threads);

/* ---- Point-cloud filter (collision/filter.hh:101-121,175-268) ---- */
/* remap_point (filter.hh:101-104): float quotient * 1000 converted to uint32 the way GCC's x86-64
 * codegen does it (cvttss2si to 64 bits, low 32 bits kept), so out-of-range inputs wrap. */
uint32_t vo_remap_point(float x, float mn, float mx);
/* morton_pdep (filter.hh:124-127): x -> bits 0,3,..,30; y -> 1,4,..,31; z -> 2,5,..,29. */
uint32_t vo_morton_encode(uint32_t x, uint32_t y, uint32_t z);
/* filter_pointcloud (filter.hh:175-268). pc: n x 3 f32. Writes the kept point indices (in the
 * final sort order) to out_idx (capacity n) and returns their count. Ties among equal Morton
 * codes are ordered by position in the previous pass (a stable sort); the reference uses
 * pdqsort_branchless (unstable), so results on tied codes are parity unpinned. Reproduces the
 * reference's quirks: the upper bound starts as min(origin + max_range) over axes (filter.hh:192),
 * and with cull the Morton list keeps its full length n, its unfilled tail naming point 0
 * (filter.hh:194-214). */
size_t vo_filter_pointcloud(const float *pc, size_t n, float min_dist, float max_range, const float origin[3],
                            const float ws_min[3], const float ws_max[3], int cull, uint32_t *out_idx);

#ifdef __cplusplus
}
#endif
#endif
