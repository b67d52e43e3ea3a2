// vcpu_simplify.cpp -- path simplification on the CPU rake (the post-processing step of every planner call:
// vamp.<robot>.simplify(plan.path, env, settings, rng), bindings/common.hh:677-683).
//
// Restates vamp::planning::simplify<Robot, 8, Robot::resolution> (planning/simplify.hh:192-260) with
// SimplifySettings (simplify_settings.hh:41-51) over this build's validate_motion:
//   * straight-line test first (:222-230): two waypoints, or a valid front -> back motion, give
//     [front, back] with iterations = 0; fewer than two waypoints are returned as they are;
//   * up to max_iterations iterations (:239-256), each running the listed operations in order and
//     stopping after the first one in which no operation changed the path;
//   * shortcut_path (:116-141): from waypoint i the farthest j > i + 1 with a valid motion i -> j erases
//     the waypoints between them; the loop bound is re-read after every erase;
//   * smooth_bspline (:14-53): Path::subdivide (plan.hh:34-49), then every even index moves to the
//     midpoint of its two half-way points when that moves it by more than min_change and both new
//     edges are valid; a step that updates nothing ends the operation (the path stays subdivided);
//   * float ops as the source states them: interpolate(a, b, t) = a + (b - a) * t, unfused
//     (interface.hh:422-425; the release build may contract the multiply into the add -- simplify.hh
//     cannot be compiled here, so that is unpinned); distance = l2_norm of the
//     difference in the reference's lane order;
//   * REDUCE and PERTURB (the reference's mt19937 distribution) and settings.interpolate are not
//     built: VGPU_ERR_UNSUPPORTED.
// Extension: max_path_len (0 = none) stops a path before a subdivide that would exceed it, with
// status VGPU_SIMPLIFY_CAPACITY -- the limit a fixed-capacity device buffer imposes (vgpu_simplify.hip),
// so that the two stay comparable.
#include <algorithm>
#include <chrono>
#include <limits>
#include <vector>

#include "vcpu_robot.hh"
#include "../vgpu_abi.hh"

using namespace vcpu;

extern "C" int vgpu_simplify_settings_default(vgpu_simplify_settings* s)
try {
    if (!s) return VGPU_ERR_INVALID_ARG;
    *s = vgpu_simplify_settings{};
    s->max_iterations = 5;
    s->interpolate = 0;
    s->n_operations = 2;
    s->operations[0] = VGPU_SIMPLIFY_SHORTCUT;
    s->operations[1] = VGPU_SIMPLIFY_BSPLINE;
    s->bspline_max_steps = 1;
    s->bspline_min_change = 0.1f;
    s->bspline_midpoint_interpolation = 0.5f;
    s->max_path_len = 0;
    return VGPU_OK;
} VGPU_ABI_CATCH

namespace vcpu {

// the settings both simplify entry points accept: VGPU_OK, or the error with *field naming the cause
int simplify_settings_check(const vgpu_simplify_settings* s, const char** field)
{
    *field = "";
    if (!s) return *field = "settings", VGPU_ERR_INVALID_ARG;
    if (s->n_operations < 0 || s->n_operations > 8) return *field = "n_operations", VGPU_ERR_INVALID_ARG;
    if (s->interpolate) return *field = "interpolate", VGPU_ERR_UNSUPPORTED;
    for (int i = 0; i < s->n_operations; ++i) {
        const int op = s->operations[i];
        if (op == VGPU_SIMPLIFY_REDUCE) return *field = "operations: REDUCE", VGPU_ERR_UNSUPPORTED;
        if (op == VGPU_SIMPLIFY_PERTURB) return *field = "operations: PERTURB", VGPU_ERR_UNSUPPORTED;
        if (op != VGPU_SIMPLIFY_BSPLINE && op != VGPU_SIMPLIFY_SHORTCUT) return *field = "operations", VGPU_ERR_INVALID_ARG;
    }
    return VGPU_OK;
}

}  // namespace vcpu

extern "C" int vgpu_cpu_simplify(const vgpu_robot* robot, vgpu_env* env, const float* path, size_t len,
                                 const vgpu_simplify_settings* settings, float* out, size_t out_cap,
                                 vgpu_plan_result* result, int32_t* status)
try {
    Bound b;
    Env e;
    const char* field;
    if ((len && !path) || !result || (out_cap && !out)) return VGPU_ERR_INVALID_ARG;
    if (int rc = simplify_settings_check(settings, &field)) return rc;
    if (int rc = bind(robot, b)) return rc;
    if (int rc = view(env, e)) return rc;
    if (e.attached && !b.R->fkcc_attach) return VGPU_ERR_UNSUPPORTED;
    const size_t D = (size_t)b.R->dim;
    const vgpu_simplify_settings& S = *settings;

    std::vector<float> p(path, path + len * D);  // result.path, D floats per waypoint
    auto size = [&] { return p.size() / D; };
    auto at = [&](size_t i) -> float* { return p.data() + i * D; };
    uint64_t checks = 0;
    auto valid = [&](const float* s, const float* g) {
        ++checks;
        return validate_one(b, e, s, g, nullptr, nullptr);
    };
    auto distance = [&](const float* x, const float* y) {  // x.distance(y) = (y - x).l2_norm()
        float d[kMaxDim];
        for (size_t j = 0; j < D; ++j) d[j] = y[j] - x[j];
        return l2_norm(d, (int)D);
    };
    auto interpolate = [&](const float* x, const float* y, float t, float* r) {  // interface.hh:422-425
        for (size_t j = 0; j < D; ++j) r[j] = x[j] + (y[j] - x[j]) * t;
    };
    int32_t st = VGPU_SIMPLIFY_DONE;

    auto shortcut = [&]() -> bool {  // simplify.hh:116-141
        if (size() < 3) return false;
        bool changed = false;
        for (size_t i = 0; i < size() - 2; ++i) {
            for (size_t j = size() - 1; j > i + 1; --j) {
                if (valid(at(i), at(j))) {
                    p.erase(p.begin() + (i + 1) * D, p.begin() + j * D);
                    changed = true;
                    break;
                }
            }
        }
        return changed;
    };
    auto bspline = [&]() -> bool {  // simplify.hh:14-53
        if (size() < 3) return false;
        bool changed = false;
        std::vector<float> next;
        float t1[kMaxDim], t2[kMaxDim], mid[kMaxDim];
        for (uint64_t step = 0; step < S.bspline_max_steps; ++step) {
            const size_t n = size();
            if (S.max_path_len && 2 * n - 1 > S.max_path_len) {
                st = VGPU_SIMPLIFY_CAPACITY;
                return changed;
            }
            next.resize((2 * n - 1) * D);  // Path::subdivide (plan.hh:34-49)
            for (size_t i = 0; i + 1 < n; ++i) {
                std::copy(at(i), at(i) + D, next.data() + 2 * i * D);
                interpolate(at(i), at(i + 1), 0.5f, next.data() + (2 * i + 1) * D);
            }
            std::copy(at(n - 1), at(n - 1) + D, next.data() + (2 * n - 2) * D);
            p.swap(next);
            bool updated = false;
            for (size_t index = 2; index < size() - 1; index += 2) {
                interpolate(at(index), at(index - 1), S.bspline_midpoint_interpolation, t1);
                interpolate(at(index), at(index + 1), S.bspline_midpoint_interpolation, t2);
                interpolate(t1, t2, 0.5f, mid);
                if (distance(at(index), mid) > S.bspline_min_change && valid(at(index - 1), mid) &&
                    valid(mid, at(index + 1))) {
                    std::copy(mid, mid + D, at(index));
                    changed = updated = true;
                }
            }
            if (!updated) break;
        }
        return changed;
    };

    const auto t0 = std::chrono::steady_clock::now();
    *result = vgpu_plan_result{};
    uint64_t iterations = 0;
    if (len == 2 || (len > 2 && valid(at(0), at(len - 1)))) {  // simplify.hh:222-230
        if (len > 2) p.erase(p.begin() + D, p.begin() + (len - 1) * D);
    } else if (len > 2) {
        for (uint64_t i = 0; i < S.max_iterations && st == VGPU_SIMPLIFY_DONE; ++i) {  // simplify.hh:239-256
            ++iterations;
            bool any = false;
            for (int k = 0; k < S.n_operations && st == VGPU_SIMPLIFY_DONE; ++k)
                any |= S.operations[k] == VGPU_SIMPLIFY_SHORTCUT ? shortcut() : bspline();
            if (!any) break;
        }
    }
    float cost = std::numeric_limits<float>::infinity();  // Path::cost (plan.hh:13-32)
    if (size() > 2) {
        cost = 0.0f;
        for (size_t i = 0; i + 1 < size(); ++i) cost += distance(at(i), at(i + 1));
    } else if (size() == 2) {
        cost = distance(at(0), at(1));
    }
    result->nanoseconds =
        (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    result->solved = 1;
    result->iterations = iterations;
    result->size[0] = checks;
    result->cost = cost;
    result->path_len = size();
    if (status) *status = st;
    if (result->path_len > out_cap) return VGPU_ERR_INVALID_ARG;
    std::copy(p.begin(), p.end(), out);
    return VGPU_OK;
} VGPU_ABI_CATCH
