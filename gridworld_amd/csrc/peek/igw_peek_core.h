// igw_peek_core.h -- the peek kernel, one copy for libigw_peek.so (igw_peek.hip, the Discrete(18) space) and
// libigw_peek_dict.so (igw_peek_dict.hip, the flying and the walking Dict space): what each env would be paid, when it
// would end, what it would build and where it would stand if it played each of K sequences of H actions from its live
// state, in one launch that writes nothing but those answers.
//
// One workgroup of 256 lanes serves 64 candidates of ONE env, a quad per candidate (Grp<4>): hit_test<4>,
// substeps_owned<4, FLY, ...> and the quad trig exchange of the step are compiled from igw_device.h unchanged, the
// double-double sin / cos / atan2 from igw_trig.h.  The block reads the env's records, its 1 KB histogram row and the
// 1,440-byte colour index of its task once.  What a candidate changes stays on chip:
//   occupancy   every candidate has its own 192-byte row in LDS behind the constant prefix and suffix hit_test and the
//               collision probes expect, so it collides with, stands on and aims at the blocks IT placed;
//   colours     a list of its changes so far (at most H entries: cell, new colour, old colour, start value); a break
//               takes its colour from the newest entry of its cell, else from the live grid row in HBM;
//   histogram   nothing is kept.  A step with wrong_placement != 0 copies the block's parked row into the wavefront's
//               1 KB scratch row, applies the votes of ALL the candidate's changes (vote_change of igw_vote.h), takes
//               the maximum and drops the scratch.  Candidates of a wavefront that need it in the same step are served
//               one after the other.
// The step's own functions are restated here for one quad per candidate (world_act_pre, world_act_post, finish_break,
// world_update, syn_size_delta, finish_step of igw_kernels.hip): same operations, same order, -ffp-contract=off.
// Nothing moves out of igw_kernels.hip or igw_device.h, whose build id is stamped on every profile.
// The kernel's statements are igw_peek_body.h, included inside each __global__ entry, which names its policy `Space`:
//   Space::Actions                the action pointers, a member of the kernel's parameters
//   Space::first(actions, at)     what the policy keeps of a candidate's first action `at`: a pointer, an index
//   Space::parse(actions, first, h)   action h of the candidate as World.step is handed it (Act), invalid components as no-ops
//   Space::kFly                   the flying agent: no gravity, a pitched motion vector, double-double trig
//   Space::kWrapMax               the subtractions that always suffice for the yaw wrap
//   Space::strafe_deg(s0, s1)     math.degrees(math.atan2(*agent.strafe)), 0 when not strafing
// Every loop is bounded by the code: H steps, 40 ray samples, at most 12 sub-steps, at most H list entries, a yaw wrap
// of at most kWrapMax subtractions.  No spin, nothing synchronises across workgroups.
#pragma once

#include <stdio.h>

#include "../igw_vote.h"
#include "../../../include/igw_peek.h"

namespace igw {
namespace peek {

constexpr int kCand = BLOCK / 4;                   // candidates per block
constexpr int kCandWave = WAVE / 4;                // ... per wavefront
constexpr int kMaxH = IGW_PEEK_MAX_H;
constexpr int kScratch = WAVE * 10;                // words of hit_test<4>'s scratch; its first 256 hold the recount's row
static_assert(HIST_ROW / 2 <= kScratch, "a wavefront's scratch holds a histogram row");
static_assert(CELLS <= 0x7ff, "a cell fits the low 11 bits of a change");

template <class Actions>
struct Params {
    const int8_t* grid;
    const uint32_t* occ;
    const uint16_t* hist;
    const AuxRec* aux;
    const AgentRec* agent;
    const int8_t* task_start;
    const TaskMeta* task_meta;
    const uint8_t* task_index;
    Actions act;
    float* reward;
    int16_t* ends;
    int16_t* change;
    float* pose;
    float* ret;
    double right_scale, wrong_scale, gamma;
    int32_t K, H, chunks, per_env, max_steps, select_and_place;
};

struct Shared {
    alignas(16) uint32_t occ[kCand][OCC_PITCH];             // 18 KB: the candidates' occupancy rows
    alignas(16) uint32_t hist[HIST_ROW / 2];                // the env's live histogram row
    alignas(16) uint32_t wscr[WAVES_PER_BLOCK][kScratch];   // per wavefront: the ray march's keys / the recount's row
    alignas(16) uint8_t index[IGW_TASK_INDEX_BYTES];        // the task's colour index
    // a candidate's changes: cell | new colour << 11 (the `change` output) | old colour byte << 16 | start byte << 24
    uint32_t list[kMaxH][kCand];
};

// ---------------------------------------------------------------- the step, restated for a quad per candidate

// What World.step is handed (core/world.py:434): strafe, dy, the hotbar slot (0: none), the camera deltas, remove, add
struct Act {
    double s0, s1, dy, cam0, cam1;
    int inventory;
    bool remove, add;
};

struct Motion {  // get_motion_vector (core/world.py:163-201): constant over the sub-steps of one step
    double x, y, z;
};
struct ActPre {
    bool want_sight, add, remove;
    double vx, vy, vz;  // sight vector (get_sight_vector, core/world.py:312-318); only when want_sight
};

// World.step (core/world.py:434-456) after action parsing, first half: movement, move_camera, the step's trig and the
// motion vector.  Every lane of the quad runs it with identical inputs; the three sin / cos pairs are evaluated one
// per lane and exchanged.
template <class Space>
__device__ inline ActPre world_act_pre(const Grp<4>& G, int select_and_place, Env& e, const TrigCtx& trig, const Act& w,
                                       Motion& mv) {
    constexpr bool FLY = Space::kFly;
    bool add = w.add, remove = w.remove;
    const double s0 = w.s0, s1 = w.s1, dy = w.dy;
    if (select_and_place && w.inventory != 0) { add = true; remove = false; }  // :444-446
    // movement, :344-356
    e.vy = ((dy != 0.0) & (e.vy == 0.0)) ? JUMP_SPEED * dy : e.vy;
    if (FLY) e.vy = dy == 0.0 ? 0.0 : e.vy;
    e.active = (unsigned)(w.inventory - 1) < 6u ? w.inventory : e.active;
    // move_camera, :338-342
    e.yaw = e.yaw + w.cam0;
    {
        double y = e.pitch + w.cam1;
        y = 90.0 < y ? 90.0 : y;
        y = -90.0 > y ? -90.0 : y;
        e.pitch = y;
    }
    ActPre a;
    a.add = add; a.remove = remove;
    a.want_sight = add != remove;
    const bool want_sight = a.want_sight;
    const bool strafing = s0 != 0.0 || s1 != 0.0;
    const double strafe_deg = Space::strafe_deg(s0, s1);   // :176
    // pitch serves the sight vector and, when flying, the motion vector: one evaluation, same argument => same value
    const bool want_pitch = want_sight || (FLY && strafing);
    const int l = G.gl & 3;
    const double deg = l == 1 ? e.yaw - 90.0 : l == 2 ? e.yaw + strafe_deg : e.pitch;
    const bool need = l == 1 ? want_sight : l == 2 ? strafing : want_pitch;
    double sv = 0.0, cv = 1.0;
    if (need) sincos_deg<!FLY>(trig, deg, sv, cv);
    const double sp = dpp_quad<QUAD_BCAST0>(sv), cp = dpp_quad<QUAD_BCAST0>(cv);
    const double sy = dpp_quad<QUAD_BCAST1>(sv), cy = dpp_quad<QUAD_BCAST1>(cv);
    const double sx = dpp_quad<QUAD_BCAST2>(sv), cx = dpp_quad<QUAD_BCAST2>(cv);
    // get_motion_vector, :163-201 (rotation and strafe are constant over the sub-steps)
    mv.x = 0.0; mv.y = 0.0; mv.z = 0.0;
    if (strafing) {
        if (FLY) {
            double mm = cp;
            mv.y = sp;
            if (s1 != 0.0) { mv.y = 0.0; mm = 1.0; }
            if (s0 > 0.0) mv.y *= -1.0;
            mv.x = cx * mm;
            mv.z = sx * mm;
        } else {
            mv.x = cx;
            mv.z = sx;
        }
    }
    // m = cos(radians(y)); dy = sin(radians(y)); dx = cos(radians(x - 90)) * m; dz = sin(radians(x - 90)) * m
    a.vx = cy * cp; a.vy = sp; a.vz = sy * cp;
    return a;
}

struct CellChange {
    int idx;               // dense cell index; -1: grid unchanged this step
    int old_val, new_val;  // the cell's colour before and after
};

// place_or_remove_block, :312-332, given the result of the ray march, on the candidate's own occupancy row and change
// list (`nch` entries of column `slot`); grid_g: the env's live grid row.
__device__ inline CellChange world_act_post(const Grp<4>& G, Env& e, uint32_t* occ_s, const uint32_t (*list)[kCand], int slot,
                                            int nch, const int8_t* grid_g, const ActPre& a, const Hit& h) {
    CellChange ch;
    const double x = e.x, z = e.z;
    const double y = e.y - 1.0 + PAD;  // y - (PLAYER_HEIGHT - 1) + Agent.PAD
    const double bx = (double)h.px - 0.5, by = (double)h.py, bz = (double)h.pz - 0.5;
    const bool overlap = (bx <= x) & (x <= bx + 1.0) & (bz <= z) & (z <= bz + 1.0) &
                         (((by <= y) & (y <= by + 1.0)) | ((by <= (y + 1.0)) & ((y + 1.0) <= by + 1.0)));
    const bool place = a.want_sight & a.add & h.hit & h.have_prev & (inv_get(e, e.active - 1) > 0) &
                       build_zone_i(h.px, h.py, h.pz) & !overlap;
    // (a block that is not the ground stands in the build zone: the test only keeps a clamped key out of the grid row)
    const bool brk = a.want_sight & a.remove & h.hit & (h.by != -2) & build_zone_i(h.bx, h.by, h.bz);
    const int cx = place ? h.px : h.bx, cy = place ? h.py : h.by, cz = place ? h.pz : h.bz;
    const int cell = cell_of(cx, cy, cz);
    ch.idx = (place || brk) ? cell : -1;
    ch.new_val = place ? e.active : 0;   // (`previous` is never occupied: old_val = 0 for a placement)
    ch.old_val = 0;
    inv_add(e, e.active - 1, place ? -1 : 0);
    if (brk) {
        // the colour of the block: the newest change of the cell by this candidate, else the live grid's
        int found = -1;
        for (int i = 0; i < nch; i++) {
            const uint32_t ent = list[i][slot];
            if ((int)(ent & 0x7ffu) == cell) found = (int)((ent >> 11) & 15u);
        }
        ch.old_val = found >= 0 ? found : (int)gload(grid_g + cell);
    }
    if (ch.idx >= 0) {
        wave_sync();
        if (G.gl == 0) {
            const int li = occ_bit_hbm(cx, cy, cz) + 32 * OCC_VAR0;  // the HBM row sits behind the constant prefix in LDS
            const uint32_t bit = 1u << (li & 31);
            const uint32_t w = occ_s[li >> 5];
            occ_s[li >> 5] = ch.new_val ? (w | bit) : (w & ~bit);
        }
        wave_sync();
    }
    return ch;
}

// remove_block's inventory refund (env.py:146-153 via the on_remove callback)
__device__ inline void finish_break(Env& e, const CellChange& ch) {
    if (ch.idx >= 0 && ch.new_val == 0) {
        const int texture = ch.old_val;
        if (texture >= 1 && texture <= 6) inv_add(e, texture - 1, 1);
    }
}

// World.step second half: update(dt = 1/20) (core/world.py:203-262) and the yaw wrap (:451-456); the reference wraps
// with `while yaw > 360: yaw -= 360`, Space::kWrapMax bounds it
template <class Space>
__device__ inline void world_update(const Grp<4>& G, Env& e, const uint32_t* occ_s, const Motion& mv) {
    const int m = tis_steps(e.tis_code);
    const double dt = tis_dt(e.tis_code);   // 0.05 / m
    if constexpr (Space::kFly) {
        // no gravity, no time_int_steps; a sub-step whose candidate position is outside the padded zone does nothing
        substeps_owned<4, true, false>(G, e, occ_s, mv.x, mv.y, mv.z, m, dt);
        e.vy = 0.0;
    } else {
        // (a walker well inside the padded zone cannot leave it within the step: substeps_owned's INSIDE skips the zone
        // test, whose outcome is known; both variants return the same bits there)
        const bool inside = __all((__builtin_fabs(e.x) < 6.0) & (__builtin_fabs(e.z) < 6.0) & (e.y >= -0.5) & (e.y < 9.0));
        double vy_pre;
        if (inside) vy_pre = substeps_owned<4, false, true>(G, e, occ_s, mv.x, mv.y, mv.z, m, dt);
        else vy_pre = substeps_owned<4, false, false>(G, e, occ_s, mv.x, mv.y, mv.z, m, dt);
        e.tis_code = (vy_pre < -5.0 ? 1 : 0) + (vy_pre < -10.0 ? 1 : 0) + (vy_pre < -14.0 ? 1 : 0);   // 2 / 4 / 8 / 12 sub-steps, :243-250
    }
    // yaw wrap with strict comparisons (0 and 360 both survive), :451-456
    for (int i = 0; i < Space::kWrapMax && e.yaw > 360.0; i++) e.yaw -= 360.0;
    for (int i = 0; i < Space::kWrapMax && e.yaw < 0.0; i++) e.yaw += 360.0;
}

// Task.step_intersection (tasks/task.py:103-119) part 1: block-count delta of the synthetic grid (grid - start)
__device__ inline int syn_size_delta(const CellChange& ch, int start_val) {
    if (ch.idx < 0) return 0;
    return ((ch.new_val - start_val) != 0 ? 1 : 0) - ((ch.old_val - start_val) != 0 ? 1 : 0);
}

// part 2 + GridWorld.step tail (env.py:290-296), without SizeReward
struct StepOut {
    double reward;
    bool done;
};
template <class P>
__device__ inline StepOut finish_step(const P& p, Env& e, int size_new, int mi) {
    const int wrong = e.prev_size - size_new;
    bool done = mi == e.target_size;
    e.prev_size = size_new;
    const int right = mi - e.max_int;
    e.max_int = mi;
    done = done || (e.step_no == p.max_steps);
    const double reward_right = (double)right * p.right_scale, reward_wrong = (double)wrong * p.wrong_scale;
    StepOut o;
    o.reward = right == 0 ? reward_wrong : reward_right;
    o.done = done;
    return o;
}

// ---------------------------------------------------------------- the host side

static thread_local char g_err[256] = "";

// `prefix`: the library's name and ": ", in front of every message of its entries
inline int fail(const char* prefix, int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s%s%s", prefix, what, detail);
    return code;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The checks every entry shares, then the launch of `kernel`.  `p` arrives with its action pointers set.  `act_null`: the
// message for an action pointer that is NULL, or nullptr when there is none (or the entry has said so itself);
// `tail_msg`: the message when `act_aligned` is false or an output is misaligned.
template <class Actions>
int check_and_launch(const char* prefix, void (*kernel)(const Params<Actions>), Params<Actions>& p, const char* act_null,
                     bool act_aligned, const char* tail_msg, const int8_t* grid, const uint32_t* occ, const uint16_t* hist,
                     const void* aux, const void* agent, const int8_t* task_target, const int8_t* task_start,
                     const void* task_meta, const uint8_t* task_index, int32_t n, int32_t K, int32_t H, int32_t per_env,
                     double right_placement_scale, double wrong_placement_scale, int32_t max_steps, int32_t select_and_place,
                     double gamma, float* reward, int16_t* ends, int16_t* change, float* pose, float* ret, void* stream) {
    const auto bad = [&](const char* what) { return fail(prefix, IGW_PEEK_ERR_INVALID, what); };
    if (!grid || !occ || !hist || !aux || !agent || !task_target || !task_start || !task_meta || !task_index)
        return bad("grid, occ, hist, aux, agent and the task-table buffers must not be NULL");
    if (act_null) return bad(act_null);
    if (!reward && !ends && !change && !pose && !ret) return bad("at least one output must not be NULL");
    if (n < 0) return bad("n must be >= 0");
    if (K < 1 || K > IGW_PEEK_MAX_K) return bad("K must be in 1..4096");
    if (H < 1 || H > IGW_PEEK_MAX_H) return bad("H must be in 1..32");
    if (max_steps < 1 || max_steps > 65534) return bad("max_steps must be in 1..65534");
    if (!__builtin_isfinite(gamma)) return bad("gamma must be finite");
    if (!aligned(grid, 16) || !aligned(occ, 16) || !aligned(hist, 16) || !aligned(aux, 16) || !aligned(agent, 16) ||
        !aligned(task_target, 16) || !aligned(task_start, 16) || !aligned(task_meta, 16) || !aligned(task_index, 16))
        return bad("the state and task-table buffers must be 16-byte aligned");
    if (!act_aligned || !aligned(reward, 4) || !aligned(ends, 2) || !aligned(change, 2) || !aligned(pose, 4) || !aligned(ret, 4))
        return bad(tail_msg);
    const int32_t chunks = (K + kCand - 1) / kCand;
    const int64_t blocks = (int64_t)n * chunks;
    if (blocks > 0x7fffffffll) return bad("n * ceil(K / 64) must be below 2^31");
    if (n == 0) return IGW_PEEK_OK;
    p.grid = grid; p.occ = occ; p.hist = hist; p.aux = static_cast<const AuxRec*>(aux); p.agent = static_cast<const AgentRec*>(agent);
    p.task_start = task_start; p.task_meta = static_cast<const TaskMeta*>(task_meta); p.task_index = task_index;
    p.reward = reward; p.ends = ends; p.change = change; p.pose = pose; p.ret = ret;
    p.right_scale = right_placement_scale; p.wrong_scale = wrong_placement_scale; p.gamma = gamma;
    p.K = K; p.H = H; p.chunks = chunks; p.per_env = per_env; p.max_steps = max_steps; p.select_and_place = select_and_place;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(prefix, IGW_PEEK_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_PEEK_OK;
}

}  // namespace peek
}  // namespace igw
