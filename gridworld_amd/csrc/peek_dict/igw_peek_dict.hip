// igw_peek_dict.hip -- libigw_peek_dict.so: igw_peek_flying and igw_peek_walking_dict (include/igw_peek_dict.h), what each
// env would be paid, when it would end, what it would build and where it would stand if it played each of K sequences
// of H actions of the flying or the walking Dict space from its live state, in one launch that writes nothing but
// those answers.
//
// The organisation is igw_peek.hip's (the Discrete(18) space): one workgroup of 256 lanes serves 64 candidates of ONE
// env, a quad per candidate (Grp<4>): hit_test<4>, substeps_owned<4, FLY, ...> and the quad trig exchange of the step
// are compiled here from igw_device.h unchanged, the double-double sin / cos / atan2 from igw_trig.h.  The block reads
// the env's records, its 1 KB histogram row and the 1,440-byte colour index of its task once.  What a candidate
// changes stays on chip:
//   occupancy   every candidate has its own 192-byte row in LDS behind the constant prefix and suffix hit_test and the
//               collision probes expect, so it collides with, stands on and aims at the blocks IT placed;
//   colours     a list of its changes so far (at most H entries: cell, new colour, old colour, start value); a break
//               takes its colour from the newest entry of its cell, else from the live grid row in HBM;
//   histogram   nothing is kept.  A step with wrong_placement != 0 copies the block's parked row into the wavefront's
//               1 KB scratch row, applies the votes of ALL the candidate's changes, takes the maximum and drops the
//               scratch.  Candidates of a wavefront that need it in the same step are served one after the other.
// One kernel template, instantiated per space (FLY): the action parsing with the step's treatment of invalid components
// (parse_flying_action / parse_walking_action of step_kernel in igw_kernels.hip), world_act_pre<.., MODE> with the
// general strafe heading, world_act_post, finish_break, world_update<.., MODE>, syn_size_delta and finish_step are
// restated below for one quad per candidate: same operations, same order, -ffp-contract=off.
// Every loop is bounded by the code: H steps, 40 ray samples, at most 12 sub-steps, at most H list entries, a yaw wrap
// of at most kWrapMax subtractions.  No spin, nothing synchronises across workgroups.
#include <stdio.h>

#include "../igw_device.h"
#include "../../../include/igw_peek.h"
#include "../../../include/igw_peek_dict.h"

namespace {

using namespace igw;

constexpr int kCand = BLOCK / 4;                   // candidates per block
constexpr int kCandWave = WAVE / 4;                // ... per wavefront
constexpr int kMaxH = IGW_PEEK_DICT_MAX_H;
constexpr int kLvlBytes = IGW_LEVEL_INDEX_BYTES;   // one level block of a task's colour index (include/igw.h)
constexpr int kLvlOffs = 16;                       // offs[15] behind the four rotation bounding boxes
constexpr int kLvlCells = 32;                      // cells[<= 121]: (x + 5) << 4 | (z + 5), sorted by colour class
constexpr int kScratch = WAVE * 10;                // words of hit_test<4>'s scratch; its first 256 hold the recount's row
// the reference wraps the yaw with `while yaw > 360: yaw -= 360`; poses are validated to |yaw| <= IGW_CAMERA_MAX and so is
// the camera delta of a step, so this many subtractions always suffice
constexpr int kWrapMax = (int)(2.0 * IGW_CAMERA_MAX / 360.0) + 2;
static_assert(IGW_PEEK_DICT_MAX_H == IGW_PEEK_MAX_H && IGW_PEEK_DICT_MAX_K == IGW_PEEK_MAX_K && IGW_PEEK_DICT_POSE == IGW_PEEK_POSE,
              "the limits are igw_peek's");
static_assert(kLvlCells + LEVEL <= kLvlBytes && kLvlBytes % 16 == 0, "level index block layout");
static_assert(IGW_TASK_INDEX_BYTES == IGW_GRID_Y * kLvlBytes && IGW_TASK_INDEX_BYTES % 16 == 0, "task colour index layout");
static_assert(HIST_ROW * 2 == WAVE * 16 && HIST_ROW / 2 <= kScratch, "a wavefront holds a histogram row as one dwordx4 per lane");
static_assert(CELLS <= 0x7ff, "a cell fits the low 11 bits of a change");

struct PeekParams {
    const int8_t* grid;
    const uint32_t* occ;
    const uint16_t* hist;
    const AuxRec* aux;
    const AgentRec* agent;
    const int8_t* task_start;
    const TaskMeta* task_meta;
    const uint8_t* task_index;
    const float* movement;      // flying
    const float* camera;        // both spaces
    const int32_t* inventory;   // flying
    const int32_t* placement;   // flying
    const uint8_t* buttons;     // walking Dict
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

// class + 1 of a synthetic colour in the colour index (0: nothing in a target can match it); a colour outside -7..7
// clamps to the empty slice behind the last class (include/igw.h)
__device__ inline int class1(int c) {
    const int k = min(max(c + 7 + (int)((uint32_t)c >> 31), 0), 15);
    return c == 0 ? 0 : k;
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ inline int row_piece_max(const uint4& v) {
    const us2 m = __builtin_elementwise_max(
        __builtin_elementwise_max(__builtin_bit_cast(us2, v.x), __builtin_bit_cast(us2, v.y)),
        __builtin_elementwise_max(__builtin_bit_cast(us2, v.z), __builtin_bit_cast(us2, v.w)));
    return (int)max((uint32_t)m.x, (uint32_t)m.y);
}

// ---------------------------------------------------------------- the step, restated for a quad per candidate

// A camera delta the step accepts: finite and |v| <= IGW_CAMERA_MAX (camera_ok of igw_kernels.hip); false for NaN / inf
__device__ inline bool camera_ok(double v) { return __builtin_fabs(v) <= IGW_CAMERA_MAX; }

// What World.step is handed (core/world.py:434): strafe, dy, the hotbar slot (0: none), the camera deltas, remove, add
struct DictAct {
    double s0, s1, dy, cam0, cam1;
    int inventory;
    bool remove, add;
};

// parse_flying_action (core/world.py:416-432) with the step's treatment of invalid components: each runs as a no-op
__device__ inline DictAct parse_flying(const PeekParams& p, int64_t at) {
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
    DictAct a;
    a.s0 = f[0]; a.s1 = f[1]; a.dy = f[2]; a.cam0 = f[3]; a.cam1 = f[4];
    a.inventory = inventory;
    a.remove = placement == 2;
    a.add = placement == 1;
    return a;
}

// parse_walking_action (core/world.py:396-414), likewise
__device__ inline DictAct parse_walking_dict(const PeekParams& p, int64_t at) {
    const uint2 bw = gload(reinterpret_cast<const uint2*>(p.buttons + IGW_PEEK_DICT_BUTTONS * at));
    const bool fwd = bw.x & 0xffu, back = bw.x & 0xff00u, left = bw.x & 0xff0000u, right = bw.x & 0xff000000u;
    const bool jump = bw.y & 0xffu, attack = bw.y & 0xff00u, use = bw.y & 0xff0000u;
    int hotbar = (int)(bw.y >> 24);
    double c0 = (double)gload(p.camera + 2 * at), c1 = (double)gload(p.camera + 2 * at + 1);
    if (hotbar > 6) hotbar = 0;
    if (!camera_ok(c0)) c0 = 0.0;
    if (!camera_ok(c1)) c1 = 0.0;
    DictAct a;
    a.s0 = (fwd ? -1.0 : 0.0) + (back ? 1.0 : 0.0);
    a.s1 = (left ? -1.0 : 0.0) + (right ? 1.0 : 0.0);
    a.dy = jump ? 1.0 : 0.0;
    a.cam0 = c0; a.cam1 = c1;
    a.inventory = hotbar;
    a.remove = attack;
    a.add = use;
    return a;
}

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
template <bool FLY>
__device__ inline ActPre world_act_pre(const Grp<4>& G, int select_and_place, Env& e, const TrigCtx& trig, const DictAct& w,
                                       Motion& mv) {
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
    // math.degrees(math.atan2(*agent.strafe)), :176
    double strafe_deg = 0.0;
    if (strafing) {
        if (!FLY && s1 == 0.0) strafe_deg = s0 < 0.0 ? -90.0 : 90.0;       // degrees(atan2(-+1, 0))
        else if (!FLY && s0 == 0.0) strafe_deg = s1 < 0.0 ? 180.0 : 0.0;   // degrees(atan2(0, -+1))
        else strafe_deg = igw_atan2(s0, s1) * D180_OVER_PI;
    }
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

// World.step second half: update(dt = 1/20) (core/world.py:203-262) and the yaw wrap (:451-456)
template <bool FLY>
__device__ inline void world_update(const Grp<4>& G, Env& e, const uint32_t* occ_s, const Motion& mv) {
    const int m = tis_steps(e.tis_code);
    const double dt = tis_dt(e.tis_code);   // 0.05 / m
    if constexpr (FLY) {
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
    for (int i = 0; i < kWrapMax && e.yaw > 360.0; i++) e.yaw -= 360.0;
    for (int i = 0; i < kWrapMax && e.yaw < 0.0; i++) e.yaw += 360.0;
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
__device__ inline StepOut finish_step(const PeekParams& p, Env& e, int size_new, int mi) {
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

// One change's votes on a histogram row in LDS, by the whole wavefront: the target cells of the changed cell's level
// whose colour is the cell's old synthetic colour lose a vote, those of its new one gain one, per rotation and
// admissible translation (resolve_changes of igw_kernels.hip, as igw_goal.hip and igw_peek.hip restate it).  Uniform
// arguments.
__device__ inline void vote_change(uint32_t* hrow, const uint8_t* index, int cell, int s0, int s1) {
    const int lane = __lane_id();
    const int q = lane & 3, mi = lane >> 2;
    const int lvl = cell / LEVEL, rem = cell - lvl * LEVEL, gx = rem / 11, gz = rem - gx * 11;
    const uint8_t* blk = index + lvl * kLvlBytes;
    const int ka = class1(s0), kb = class1(s1);
    const int oa0 = blk[kLvlOffs - 1 + ka], oa1 = blk[kLvlOffs + ka], ob0 = blk[kLvlOffs - 1 + kb], ob1 = blk[kLvlOffs + kb];
    const int na = ka != 0 ? oa1 - oa0 : 0, nv = na + (kb != 0 ? ob1 - ob0 : 0);
    const int bb = (int)reinterpret_cast<const uint32_t*>(blk)[q];
    const int xmin = (int)(int8_t)(bb & 0xff), dxlo = (int)(int8_t)((bb >> 8) & 0xff) - 10;
    const int zmin = (int)(int8_t)((bb >> 16) & 0xff), dzlo = (int)(int8_t)((bb >> 24) & 0xff) - 10;
    for (int i0 = 0; i0 < nv; i0 += WAVE / 4) {   // nv <= 2 * 121
        const int idx = i0 + mi;
        if (idx < nv) {
            const bool dec = idx < na;
            const int tc = blk[kLvlCells + (dec ? oa0 + idx : ob0 + (idx - na))];
            const int tx = tc >> 4, tz = tc & 15;
            const int bx = (q & 1) ? tz : tx, bz = (q & 1) ? tx : tz;
            const int rx = q >= 2 ? 10 - bx : bx, rz = (q == 1 || q == 2) ? 10 - bz : bz;
            const int u = rx - gx - dxlo, v = rz - gz - dzlo;
            if ((unsigned)u <= (unsigned)(xmin - dxlo) && (unsigned)v <= (unsigned)(zmin - dzlo)) {
                const int bin = q * LEVEL + u * 11 + v;
                atomicAdd(&hrow[bin >> 1], (dec ? 0xffffffffu : 1u) << (16 * (bin & 1)));
            }
        }
    }
}

template <bool FLY>
__global__ __launch_bounds__(BLOCK) void igw_peek_dict_kernel(const PeekParams p) {
    __shared__ Shared sh;
    const Grp<4> G;
    const int tid = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t bid = (int64_t)blockIdx.x;
    const int64_t env = bid / p.chunks;
    const int chunk = (int)(bid - env * p.chunks);
    const int slot = tid >> 2;
    const bool real = chunk * kCand + slot < p.K;
    const int k = real ? chunk * kCand + slot : p.K - 1;   // (a candidate past K plays the last one's actions and stores nothing)
    const bool writer = real && G.gl == 0;

    // ---- the env: records, task, live rows
    Env e;
    const int64_t task = (int64_t)__builtin_amdgcn_readfirstlane(env_load(e, p.agent + env, p.aux + env));
    const bool has_start = __builtin_amdgcn_readfirstlane((int)gload(&p.task_meta[task].has_start)) != 0;
    const int8_t* grid_g = p.grid + env * STRIDE;
    const int8_t* start_g = p.task_start + task * STRIDE;
    uint32_t* occ_s = sh.occ[slot];
    for (int w = G.gl; w < OCC_PITCH; w += 4) {   // words 0..15 and 64..71 constant (occ_const_word), 16..63 the env's
        const bool var = (w >= OCC_VAR0) & (w < OCC_VAR0 + OCC_WORDS);
        occ_s[w] = var ? gload(p.occ + env * OCC_WORDS + (var ? w - OCC_VAR0 : 0)) : occ_const_word(w);
    }
    if (tid < WAVE) reinterpret_cast<uint4*>(sh.hist)[tid] = gload(reinterpret_cast<const uint4*>(p.hist + env * HIST_ROW) + tid);
    else if (tid < WAVE + IGW_TASK_INDEX_BYTES / 16)
        reinterpret_cast<uint4*>(sh.index)[tid - WAVE] =
            gload(reinterpret_cast<const uint4*>(p.task_index + task * IGW_TASK_INDEX_BYTES) + (tid - WAVE));
    __syncthreads();

    TrigCtx trig;
    // sincos_deg<true> reads lut[2 * k] = cos and lut[2 * k + 1] = sin of entry k < IGW_LUT_N: the host table's layout
    static_assert(sizeof(IGW_TRIG_LUT_HOST) == sizeof(double) * 2 * IGW_LUT_N, "the trig table is IGW_LUT_N (cos, sin) pairs of doubles");
    trig.lut = &IGW_TRIG_LUT_HOST[0][0];   // a const table with a constant initialiser: constant memory of this code object

    const int64_t row = env * p.K + k;                                   // the candidate's row of the outputs
    const int64_t act0 = (p.per_env ? row : (int64_t)k) * p.H;           // ... and its first action
    uint32_t* const scratch = sh.wscr[wave];
    bool live = true;
    int ends = 0, nch = 0;
    double ret = 0.0, g = 1.0;
    for (int h = 0; h < p.H; h++) {
        CellChange ch;
        ch.idx = -1; ch.old_val = ch.new_val = 0;
        int size_new = e.prev_size;
        if (live) {
            const DictAct w = FLY ? parse_flying(p, act0 + h) : parse_walking_dict(p, act0 + h);
            e.step_no = min(e.step_no + 1, 65535);  // env.py:276
            Motion mv;
            const ActPre ap = world_act_pre<FLY>(G, p.select_and_place, e, trig, w, mv);
            Hit hit;
            hit.hit = false; hit.have_prev = false;
            hit.bx = hit.by = hit.bz = hit.px = hit.py = hit.pz = 0;
            if (ap.want_sight) hit = hit_test<4>(G, occ_s, e.x, e.y, e.z, ap.vx, ap.vy, ap.vz, false, scratch);
            ch = world_act_post(G, e, occ_s, sh.list, slot, nch, grid_g, ap, hit);
            int start_val = 0;
            if (ch.idx >= 0) {
                if (has_start) start_val = (int)gload(start_g + ch.idx);
                if (G.gl == 0)
                    sh.list[nch][slot] = (uint32_t)ch.idx | (uint32_t)ch.new_val << 11 | (uint32_t)(uint8_t)ch.old_val << 16 |
                                         (uint32_t)(uint8_t)start_val << 24;
                nch++;   // (at most one per step: nch <= H <= kMaxH)
            }
            world_update<FLY>(G, e, occ_s, mv);
            finish_break(e, ch);
            size_new = e.prev_size + syn_size_delta(ch, start_val);  // synthetic grid = grid - start (env.py:290)
        }
        // ---- max_int = maximal_intersection(grid) where wrong_placement != 0 (tasks/task.py:112): the live row with all
        // of the candidate's changes, one candidate of the wavefront after the other
        const bool need = live && size_new != e.prev_size;
        int mi = e.max_int;
        uint64_t todo = __ballot(need && G.gl == 0);
        while (todo != 0) {   // at most kCandWave rounds
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int cw = l >> 2, cs = wave * kCandWave + cw;
            const int n_c = __builtin_amdgcn_readlane(nch, l);
            wave_sync();
            reinterpret_cast<uint4*>(scratch)[G.lane] = reinterpret_cast<const uint4*>(sh.hist)[G.lane];
            wave_sync();
            for (int i = 0; i < n_c; i++) {
                const uint32_t ent = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.list[i][cs]);
                const int st = (int)(int8_t)(ent >> 24);
                vote_change(scratch, sh.index, (int)(ent & 0x7ffu), (int)(int8_t)((ent >> 16) & 0xffu) - st, (int)((ent >> 11) & 15u) - st);
            }
            wave_sync();
            const int best = wave_max_nonneg(row_piece_max(reinterpret_cast<const uint4*>(scratch)[G.lane]));
            if ((G.lane >> 2) == cw) mi = best;
        }
        wave_sync();
        float r32 = 0.0f;
        int chg = -1;
        if (live) {
            const StepOut o = finish_step(p, e, size_new, mi);
            ret = ret + g * o.reward;
            g = g * p.gamma;
            r32 = (float)o.reward;
            chg = ch.idx >= 0 ? (ch.idx | ch.new_val << 11) : -1;
            if (o.done) {
                live = false;
                ends = h + 1;
            }
        }
        if (writer) {
            if (p.reward) gstore(p.reward + row * p.H + h, r32);
            if (p.change) gstore(p.change + row * p.H + h, (int16_t)chg);
        }
    }
    if (writer) {
        if (p.ends) gstore(p.ends + row, (int16_t)ends);
        if (p.ret) gstore(p.ret + row, (float)ret);
        if (p.pose) {   // out_piece_step's casts (env.py:281-289)
            float* o = p.pose + row * IGW_PEEK_DICT_POSE;
            gstore(o + 0, (float)e.x);
            gstore(o + 1, (float)e.y);
            gstore(o + 2, (float)e.z);
            gstore(o + 3, (float)e.pitch);
            gstore(o + 4, (float)e.yaw);
        }
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_peek_dict: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The checks both entries share, then the launch.  `p` arrives with its action pointers set and checked.
int peek_common(bool fly, PeekParams& p, const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux,
                const void* agent, const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                const uint8_t* task_index, int32_t n, int32_t K, int32_t H, int32_t per_env, double right_placement_scale,
                double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma, float* reward,
                int16_t* ends, int16_t* change, float* pose, float* ret, void* stream) {
    if (!grid || !occ || !hist || !aux || !agent || !task_target || !task_start || !task_meta || !task_index)
        return fail(IGW_PEEK_ERR_INVALID, "grid, occ, hist, aux, agent and the task-table buffers must not be NULL");
    if (!reward && !ends && !change && !pose && !ret) return fail(IGW_PEEK_ERR_INVALID, "at least one output must not be NULL");
    if (n < 0) return fail(IGW_PEEK_ERR_INVALID, "n must be >= 0");
    if (K < 1 || K > IGW_PEEK_DICT_MAX_K) return fail(IGW_PEEK_ERR_INVALID, "K must be in 1..4096");
    if (H < 1 || H > IGW_PEEK_DICT_MAX_H) return fail(IGW_PEEK_ERR_INVALID, "H must be in 1..32");
    if (max_steps < 1 || max_steps > 65534) return fail(IGW_PEEK_ERR_INVALID, "max_steps must be in 1..65534");
    if (!__builtin_isfinite(gamma)) return fail(IGW_PEEK_ERR_INVALID, "gamma must be finite");
    if (!aligned(grid, 16) || !aligned(occ, 16) || !aligned(hist, 16) || !aligned(aux, 16) || !aligned(agent, 16) ||
        !aligned(task_target, 16) || !aligned(task_start, 16) || !aligned(task_meta, 16) || !aligned(task_index, 16))
        return fail(IGW_PEEK_ERR_INVALID, "the state and task-table buffers must be 16-byte aligned");
    if (!aligned(reward, 4) || !aligned(ends, 2) || !aligned(change, 2) || !aligned(pose, 4) || !aligned(ret, 4))
        return fail(IGW_PEEK_ERR_INVALID, "reward, pose and ret must be 4-byte, ends and change 2-byte aligned");
    const int32_t chunks = (K + kCand - 1) / kCand;
    const int64_t blocks = (int64_t)n * chunks;
    if (blocks > 0x7fffffffll) return fail(IGW_PEEK_ERR_INVALID, "n * ceil(K / 64) must be below 2^31");
    if (n == 0) return IGW_PEEK_OK;
    p.grid = grid; p.occ = occ; p.hist = hist; p.aux = static_cast<const AuxRec*>(aux); p.agent = static_cast<const AgentRec*>(agent);
    p.task_start = task_start; p.task_meta = static_cast<const TaskMeta*>(task_meta); p.task_index = task_index;
    p.reward = reward; p.ends = ends; p.change = change; p.pose = pose; p.ret = ret;
    p.right_scale = right_placement_scale; p.wrong_scale = wrong_placement_scale; p.gamma = gamma;
    p.K = K; p.H = H; p.chunks = chunks; p.per_env = per_env; p.max_steps = max_steps; p.select_and_place = select_and_place;
    if (fly) hipLaunchKernelGGL(igw_peek_dict_kernel<true>, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(igw_peek_dict_kernel<false>, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_PEEK_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_PEEK_OK;
}

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
        return fail(IGW_PEEK_ERR_INVALID, "movement, camera, inventory and placement must not be NULL");
    if (!aligned(movement, 4) || !aligned(camera, 4) || !aligned(inventory, 4) || !aligned(placement, 4))
        return fail(IGW_PEEK_ERR_INVALID, "movement, camera, inventory and placement must be 4-byte aligned");
    PeekParams p = {};
    p.movement = movement; p.camera = camera; p.inventory = inventory; p.placement = placement;
    return peek_common(true, p, grid, occ, hist, aux, agent, task_target, task_start, task_meta, task_index, n, K, H, per_env,
                       right_placement_scale, wrong_placement_scale, max_steps, select_and_place, gamma, reward, ends, change,
                       pose, ret, stream);
}

int igw_peek_walking_dict(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux,
                          const void* agent, const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                          const uint8_t* task_index, int32_t n, int32_t K, int32_t H, const uint8_t* buttons,
                          const float* camera, int32_t per_env, double right_placement_scale,
                          double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma,
                          float* reward, int16_t* ends, int16_t* change, float* pose, float* ret, void* stream) {
    if (!buttons || !camera) return fail(IGW_PEEK_ERR_INVALID, "buttons and camera must not be NULL");
    if (!aligned(buttons, 8) || !aligned(camera, 4))
        return fail(IGW_PEEK_ERR_INVALID, "buttons must be 8-byte, camera 4-byte aligned");
    PeekParams p = {};
    p.buttons = buttons; p.camera = camera;
    return peek_common(false, p, grid, occ, hist, aux, agent, task_target, task_start, task_meta, task_index, n, K, H, per_env,
                       right_placement_scale, wrong_placement_scale, max_steps, select_and_place, gamma, reward, ends, change,
                       pose, ret, stream);
}

}  // extern "C"
