// igw_peek_dict.hip -- libigw_peek_dict.so: igw_peek_flying and igw_peek_walking_dict (include/igw_peek_dict.h), the peek
// query for the flying and the walking Dict action spaces.
//
// The kernel -- its organisation, the step's functions restated for a quad per candidate, the shared argument checks --
// is ../peek/igw_peek_core.h's and igw_peek_body.h's, which libigw_peek.so uses for the Discrete(18) space.  This file holds what
// belongs to the two spaces: the action parsing with the step's treatment of invalid components (parse_flying_action /
// parse_walking_action of step_kernel in igw_kernels.hip), the general strafe heading, the bound of the yaw wrap, one
// kernel per space (FLY) and the entries.
#include "../igw_device.h"
#include "../peek/igw_peek_core.h"
#include "../../../include/igw_peek_dict.h"

namespace {

using namespace igw;
using namespace igw::peek;

static_assert(IGW_PEEK_DICT_MAX_H == IGW_PEEK_MAX_H && IGW_PEEK_DICT_MAX_K == IGW_PEEK_MAX_K && IGW_PEEK_DICT_POSE == IGW_PEEK_POSE,
              "the limits are igw_peek's");

struct DictActions {
    const float* movement;      // flying
    const float* camera;        // both spaces
    const int32_t* inventory;   // flying
    const int32_t* placement;   // flying
    const uint8_t* buttons;     // walking Dict
};
using PeekParams = Params<DictActions>;

// A camera delta the step accepts: finite and |v| <= IGW_CAMERA_MAX (camera_ok of igw_kernels.hip); false for NaN / inf
__device__ inline bool camera_ok(double v) { return __builtin_fabs(v) <= IGW_CAMERA_MAX; }

// parse_flying_action (core/world.py:416-432) with the step's treatment of invalid components: each runs as a no-op
__device__ inline Act parse_flying(const DictActions& p, int64_t at) {
    double f[5];
#pragma unroll
    for (int i = 0; i < 3; i++) f[i] = (double)gload(p.movement + 3 * at + i);
    f[3] = (double)gload(p.camera + 2 * at);
    f[4] = (double)gload(p.camera + 2 * at + 1);
    int inventory = gload(p.inventory + at);
    const int placement = gload(p.placement + at);
    if ((unsigned)inventory > 6u) inventory = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        if (i < 3 ? !__builtin_isfinite(f[i]) : !camera_ok(f[i])) f[i] = 0.0;
    }
    Act a;
    a.s0 = f[0]; a.s1 = f[1]; a.dy = f[2]; a.cam0 = f[3]; a.cam1 = f[4];
    a.inventory = inventory;
    a.remove = placement == 2;
    a.add = placement == 1;
    return a;
}

// parse_walking_action (core/world.py:396-414), likewise
__device__ inline Act parse_walking_dict(const DictActions& p, int64_t at) {
    const uint2 bw = gload(reinterpret_cast<const uint2*>(p.buttons + IGW_PEEK_DICT_BUTTONS * at));
    const bool fwd = bw.x & 0xffu, back = bw.x & 0xff00u, left = bw.x & 0xff0000u, right = bw.x & 0xff000000u;
    const bool jump = bw.y & 0xffu, attack = bw.y & 0xff00u, use = bw.y & 0xff0000u;
    int hotbar = (int)(bw.y >> 24);
    double c0 = (double)gload(p.camera + 2 * at), c1 = (double)gload(p.camera + 2 * at + 1);
    if (hotbar > 6) hotbar = 0;
    if (!camera_ok(c0)) c0 = 0.0;
    if (!camera_ok(c1)) c1 = 0.0;
    Act a;
    a.s0 = (fwd ? -1.0 : 0.0) + (back ? 1.0 : 0.0);
    a.s1 = (left ? -1.0 : 0.0) + (right ? 1.0 : 0.0);
    a.dy = jump ? 1.0 : 0.0;
    a.cam0 = c0; a.cam1 = c1;
    a.inventory = hotbar;
    a.remove = attack;
    a.add = use;
    return a;
}

template <bool FLY>
struct DictSpace {
    using Actions = DictActions;
    static constexpr bool kFly = FLY;
    // poses are validated to |yaw| <= IGW_CAMERA_MAX and so is the camera delta of a step, so this many subtractions
    // always suffice
    static constexpr int kWrapMax = (int)(2.0 * IGW_CAMERA_MAX / 360.0) + 2;
    static __device__ inline int64_t first(const Actions&, int64_t at) { return at; }
    static __device__ inline Act parse(const Actions& a, int64_t first, int h) { return FLY ? parse_flying(a, first + h) : parse_walking_dict(a, first + h); }
    static __device__ inline double strafe_deg(double s0, double s1) {
        double deg = 0.0;
        if (s0 != 0.0 || s1 != 0.0) {
            if (!FLY && s1 == 0.0) deg = s0 < 0.0 ? -90.0 : 90.0;       // degrees(atan2(-+1, 0))
            else if (!FLY && s0 == 0.0) deg = s1 < 0.0 ? 180.0 : 0.0;   // degrees(atan2(0, -+1))
            else deg = igw_atan2(s0, s1) * D180_OVER_PI;
        }
        return deg;
    }
};

template <bool FLY>
__global__ __launch_bounds__(BLOCK) void igw_peek_dict_kernel(const PeekParams p) {
    using Space = DictSpace<FLY>;
#include "../peek/igw_peek_body.h"
}

// an entry's own action checks fail with this; the rest is check_and_launch's
int bad_actions(const char* what) { return fail("igw_peek_dict: ", IGW_PEEK_ERR_INVALID, what); }
constexpr const char* kTailMsg = "reward, pose and ret must be 4-byte, ends and change 2-byte aligned";

}  // namespace

#ifndef IGW_PEEK_DICT_BUILD_ID
#define IGW_PEEK_DICT_BUILD_ID "igw-peek-dict-build-id:unstamped"
#endif

extern "C" {

int igw_peek_dict_version(void) { return IGW_PEEK_DICT_VERSION; }
// (the string carries a marker so that peek_dict.py can read the id of a library file without loading it)
const char* igw_peek_dict_build_id(void) { return &IGW_PEEK_DICT_BUILD_ID[sizeof("igw-peek-dict-build-id:") - 1]; }
const char* igw_peek_dict_last_error(void) { return g_err; }

int igw_peek_flying(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux, const void* agent,
                    const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                    const uint8_t* task_index, int32_t n, int32_t K, int32_t H, const float* movement,
                    const float* camera, const int32_t* inventory, const int32_t* placement, int32_t per_env,
                    double right_placement_scale, double wrong_placement_scale, int32_t max_steps,
                    int32_t select_and_place, double gamma, float* reward, int16_t* ends, int16_t* change, float* pose,
                    float* ret, void* stream) {
    if (!movement || !camera || !inventory || !placement)
        return bad_actions("movement, camera, inventory and placement must not be NULL");
    if (!aligned(movement, 4) || !aligned(camera, 4) || !aligned(inventory, 4) || !aligned(placement, 4))
        return bad_actions("movement, camera, inventory and placement must be 4-byte aligned");
    PeekParams p = {};
    p.act.movement = movement; p.act.camera = camera; p.act.inventory = inventory; p.act.placement = placement;
    return check_and_launch("igw_peek_dict: ", igw_peek_dict_kernel<true>, p, nullptr, true, kTailMsg, grid, occ, hist, aux, agent,
                            task_target, task_start, task_meta, task_index, n, K, H, per_env, right_placement_scale,
                            wrong_placement_scale, max_steps, select_and_place, gamma, reward, ends, change, pose, ret, stream);
}

int igw_peek_walking_dict(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux,
                          const void* agent, const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                          const uint8_t* task_index, int32_t n, int32_t K, int32_t H, const uint8_t* buttons,
                          const float* camera, int32_t per_env, double right_placement_scale,
                          double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma,
                          float* reward, int16_t* ends, int16_t* change, float* pose, float* ret, void* stream) {
    if (!buttons || !camera) return bad_actions("buttons and camera must not be NULL");
    if (!aligned(buttons, 8) || !aligned(camera, 4)) return bad_actions("buttons must be 8-byte, camera 4-byte aligned");
    PeekParams p = {};
    p.act.buttons = buttons; p.act.camera = camera;
    return check_and_launch("igw_peek_dict: ", igw_peek_dict_kernel<false>, p, nullptr, true, kTailMsg, grid, occ, hist, aux, agent,
                            task_target, task_start, task_meta, task_index, n, K, H, per_env, right_placement_scale,
                            wrong_placement_scale, max_steps, select_and_place, gamma, reward, ends, change, pose, ret, stream);
}

}  // extern "C"
