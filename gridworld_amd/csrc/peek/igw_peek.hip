// igw_peek.hip -- libigw_peek.so: igw_peek (include/igw_peek.h), the peek query for the walking Discrete(18) space.
//
// The kernel -- its organisation, the step's functions restated for a quad per candidate, the shared argument checks --
// is igw_peek_core.h's and igw_peek_body.h's, which libigw_peek_dict.so uses for the Dict spaces.  This file holds what belongs to
// the space: the action parser (parse_walking_discrete of igw_kernels.hip), the strafe heading of its nine possible
// strafes, the bound of the yaw wrap, and the entry.
#include "../igw_device.h"
#include "igw_peek_core.h"

namespace {

using namespace igw;
using namespace igw::peek;

// parse_walking_discrete_action (core/world.py:360-394)
__device__ inline Act parse_walking_discrete(int action) {
    // 1 fwd (s0 = -1), 2 back (+1), 3 left (s1 = -1), 4 right (+1), 5 jump, 6..11 hotbar 1..6, 12 / 13 yaw -+ 5,
    // 14 / 15 pitch -+ 5, 16 break, 17 place; anything else is a no-op
    const int a = action;
    const int twice = 2 * a;
    const auto pair = [&](int lo, int centre) { return (unsigned)(a - lo) < 2u ? twice - centre : 0; };
    Act w;
    w.s0 = (double)pair(1, 3);
    w.s1 = (double)pair(3, 7);
    w.cam0 = (double)__mul24(5, pair(12, 25));
    w.cam1 = (double)__mul24(5, pair(14, 29));
    w.dy = a == 5 ? 1.0 : 0.0;
    w.inventory = (unsigned)(a - 6) < 6u ? a - 5 : 0;
    w.remove = a == 16;
    w.add = a == 17;
    return w;
}

struct Discrete18 {
    struct Actions {
        const int32_t* actions;
    };
    static constexpr bool kFly = false;
    // poses are validated to |yaw| <= IGW_CAMERA_MAX and a step turns by 5 degrees, so this many subtractions always
    // suffice (one, from the second step of an episode on)
    static constexpr int kWrapMax = (int)(IGW_CAMERA_MAX / 360.0) + 2;
    static __device__ inline const int32_t* first(const Actions& a, int64_t at) { return a.actions + at; }
    static __device__ inline Act parse(const Actions&, const int32_t* first, int h) { return parse_walking_discrete(gload(first + h)); }
    // (s0, s1) = (-1, 0) -> -90, (1, 0) -> 90, (0, -1) -> 180, (0, 1) -> 0
    static __device__ inline double strafe_deg(double s0, double s1) {
        const int i0 = (int)s0, i1 = (int)s1;
        const uint32_t hi = (((uint32_t)(i0 < 0) << 31) | ((0u - (uint32_t)((i0 != 0) | (i1 < 0))) & 0x40568000u)) +
                            ((uint32_t)(i1 < 0) << 20);
        return __hiloint2double((int)hi, 0);
    }
};
using PeekParams = Params<Discrete18::Actions>;

__global__ __launch_bounds__(BLOCK) void igw_peek_kernel(const PeekParams p) {
    using Space = Discrete18;
#include "igw_peek_body.h"
}

}  // namespace

#ifndef IGW_PEEK_BUILD_ID
#define IGW_PEEK_BUILD_ID "igw-peek-build-id:unstamped"
#endif

extern "C" {

int igw_peek_version(void) { return IGW_PEEK_VERSION; }
// (the string carries a marker so that peek.py can read the id of a library file without loading it)
const char* igw_peek_build_id(void) { return &IGW_PEEK_BUILD_ID[sizeof("igw-peek-build-id:") - 1]; }
const char* igw_peek_last_error(void) { return g_err; }

int igw_peek(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux, const void* agent,
             const int8_t* task_target, const int8_t* task_start, const void* task_meta, const uint8_t* task_index,
             int32_t n, int32_t K, int32_t H, const int32_t* actions, int32_t per_env, double right_placement_scale,
             double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma, float* reward,
             int16_t* ends, int16_t* change, float* pose, float* ret, void* stream) {
    PeekParams p;
    p.act.actions = actions;
    return check_and_launch("igw_peek: ", igw_peek_kernel, p, actions ? nullptr : "actions must not be NULL", aligned(actions, 4),
                            "actions, reward, pose and ret must be 4-byte, ends and change 2-byte aligned", grid, occ, hist, aux,
                            agent, task_target, task_start, task_meta, task_index, n, K, H, per_env, right_placement_scale,
                            wrong_placement_scale, max_steps, select_and_place, gamma, reward, ends, change, pose, ret, stream);
}

}  // extern "C"
