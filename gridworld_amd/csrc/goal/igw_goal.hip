// igw_goal.hip -- libigw_goal.so: igw_goal (include/igw_goal.h), where the reward wants the target, what is left of it
// and what each of the 18 walking actions would earn on each env's live state, in one launch.
//
// One wavefront owns an env, a block four.  The env's 1 KB histogram row IS the answer to argmax_intersection: lane l
// loads bins 8 l .. 8 l + 7 as one dwordx4, the row maximum is a packed 16-bit maximum and a DPP reduction, the
// alignment the lowest bin that holds it.  An env that is asked for no more reads nothing else but its episode record
// and 16 bytes of task metadata.
//   want / todo: the target row is staged in LDS (69 dwordx4) and every lane builds the 16 bytes of its one or two
//     chunks of the output row from it -- the shifted, rotated read is a byte gather in LDS -- against the grid (and
//     start) chunk it loaded as one dwordx4; both rows leave as dwordx4 stores.
//   gain / ends: the row is parked in LDS once.  Per acting action the wavefront takes the changed cell's level block of
//     the colour index (160 B), votes the cell's old colour out and its new colour in with LDS atomics -- sixteen target
//     cells x four rotations per pass, the arithmetic of the step's histogram update on the level block staged here --
//     takes the maximum, and writes the row back from the registers that still hold it: one LDS copy, no undo pass.
// The colour index's layout, class1 and row_piece_max are igw_vote.h's, the query libraries' one copy.
// Nothing synchronises across wavefronts: a wavefront without an env returns at once.
#include <stdio.h>

#include "../igw_vote.h"
#include "../../../include/igw_goal.h"

namespace {

using namespace igw;

constexpr int kActions = IGW_GOAL_ACTIONS;
static_assert(CHUNKS > WAVE && CHUNKS <= 2 * WAVE, "a lane owns at most two chunks of a grid row");

struct GoalParams {
    const int8_t* grid;
    const uint16_t* hist;
    const AuxRec* aux;
    const AgentRec* agent;
    const int8_t* task_target;
    const int8_t* task_start;
    const TaskMeta* task_meta;
    const uint8_t* task_index;
    const uint8_t* mask;
    const int16_t* look;
    int8_t* align;
    int16_t* fit;
    int8_t* want;
    int8_t* todo;
    float* gain;
    uint8_t* ends;
    double right_scale, wrong_scale;
    int32_t n, max_steps, select_and_place;
};

struct WaveShared {
    alignas(16) uint32_t hist[HIST_ROW / 2];
    alignas(16) uint8_t lvl[kLvlBytes];
    alignas(16) int8_t tgt[STRIDE];
};

// the 16 bytes of chunk c of the `want` row: cell i = 16 c + j reads rotation `rot` of the LDS target at (x + dx, z + dz)
__device__ inline uint4 want_chunk(const int8_t* tgt_s, int c, int dx, int dz, int rot) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int i = 16 * c + j;
        const int y = i / LEVEL, rem = i - y * LEVEL, x = rem / 11, z = rem - x * 11;
        const int X = x + dx, Z = z + dz;
        const bool in = (i < CELLS) & ((unsigned)X <= 10u) & ((unsigned)Z <= 10u);
        // T_rot[X][Z] = T[sx][sz]: the inverse of (x, z) -> (x, z), (z, 10 - x), (10 - x, 10 - z), (10 - z, x)
        const int a = (rot & 1) ? Z : X, b = (rot & 1) ? X : Z;
        const int sx = (rot == 1 || rot == 2) ? 10 - a : a;
        const int sz = rot >= 2 ? 10 - b : b;
        const int v = tgt_s[in ? y * LEVEL + sx * 11 + sz : 0];
        w[j >> 2] |= (in ? (uint32_t)(uint8_t)v : 0u) << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bytewise a - b and "x where x != s, else 0" on packed int8
__device__ inline uint32_t sub_bytes(uint32_t a, uint32_t b) {
    return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ ((a ^ ~b) & 0x80808080u);
}
__device__ inline uint32_t keep_differing(uint32_t x, uint32_t s) {
    const uint32_t d = x ^ s;                                                // a byte is 0 where the two agree
    const uint32_t nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;   // its top bit where they differ
    return x & ((nz >> 7) * 0xffu);
}

__global__ __launch_bounds__(BLOCK) void igw_goal_kernel(const GoalParams p) {
    __shared__ WaveShared sh[WAVES_PER_BLOCK];
    const int lane = __lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
    const int64_t env = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
    if (env >= p.n) return;
    WaveShared& ws = sh[wave];

    // ---- the row, the episode record, the task's bounding boxes
    const uint4 row = gload(reinterpret_cast<const uint4*>(p.hist + env * HIST_ROW) + lane);
    const uint4 auxw = gload(reinterpret_cast<const uint4*>(p.aux + env));
    const int size = (int)((auxw.x >> 16) & 0x7fffu);
    const int cached = (int)(int16_t)(auxw.y & 0xffffu), tsize = (int)(int16_t)(auxw.y >> 16);
    const int64_t task = (int64_t)__builtin_amdgcn_readfirstlane((int)auxw.z);
    const TaskMeta* meta = p.task_meta + task;
    const uint4 bbw = gload(reinterpret_cast<const uint4*>(meta->bbox));

    // ---- align, fit: the row maximum and the lowest bin that holds it
    const int best = wave_max_nonneg(row_piece_max(row));
    int first = 0x7fffffff;
    if (best > 0) {
        const uint32_t w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
        for (int j = 3; j >= 0; j--) {   // descending, so the lowest wins
            if ((int)(w[j] >> 16) == best) first = 8 * lane + 2 * j + 1;
            if ((int)(w[j] & 0xffffu) == best) first = 8 * lane + 2 * j;
        }
    }
    first = wave_min_i32(first);
    int dx = 0, dz = 0, rot = 0;
    if (first < HIST_BINS) {   // bin = r * 121 + (dx - dxlo) * 11 + (dz - dzlo), dxlo = xmax - 10, dzlo = zmax - 10
        rot = first / LEVEL;
        const int rem = first - rot * LEVEL;
        const uint32_t bb = rot == 0 ? bbw.x : rot == 1 ? bbw.y : rot == 2 ? bbw.z : bbw.w;
        dx = rem / 11 + (int)(int8_t)((bb >> 8) & 0xffu) - 10;
        dz = rem % 11 + (int)(int8_t)(bb >> 24) - 10;
    }
    if (lane == 0) {
        if (p.align) gstore(reinterpret_cast<uint32_t*>(p.align) + env, (uint32_t)(uint8_t)dx | (uint32_t)(uint8_t)dz << 8 | (uint32_t)rot << 16);
        if (p.fit)
            gstore(reinterpret_cast<uint2*>(p.fit) + env,
                   make_uint2((uint32_t)best | (uint32_t)(uint16_t)tsize << 16, (uint32_t)size | (uint32_t)(uint16_t)cached << 16));
    }
    const bool rows = p.want != nullptr || p.todo != nullptr, gains = p.gain != nullptr || p.ends != nullptr;
    if (!rows && !gains) return;
    const bool has_start = __builtin_amdgcn_readfirstlane((int)gload(&meta->has_start)) != 0;
    const int8_t* grid_g = p.grid + env * STRIDE;
    const int8_t* start_g = p.task_start + task * STRIDE;

    // ---- want, todo
    if (rows) {
        row_to_lds_wave(ws.tgt, p.task_target + task * STRIDE);
        wave_sync();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int c = lane + k * WAVE;
            if (c < CHUNKS) {
                const uint4 wt = want_chunk(ws.tgt, c, dx, dz, rot);
                if (p.want) gstore(reinterpret_cast<uint4*>(p.want + env * STRIDE) + c, wt);
                if (p.todo) {
                    uint4 s = gload(reinterpret_cast<const uint4*>(grid_g) + c);
                    if (has_start) {
                        const uint4 st = gload(reinterpret_cast<const uint4*>(start_g) + c);
                        s = make_uint4(sub_bytes(s.x, st.x), sub_bytes(s.y, st.y), sub_bytes(s.z, st.z), sub_bytes(s.w, st.w));
                    }
                    gstore(reinterpret_cast<uint4*>(p.todo + env * STRIDE) + c,
                           make_uint4(keep_differing(wt.x, s.x), keep_differing(wt.y, s.y), keep_differing(wt.z, s.z),
                                      keep_differing(wt.w, s.w)));
                }
            }
        }
    }
    if (!gains) return;

    // ---- gain, ends
    reinterpret_cast<uint4*>(ws.hist)[lane] = row;
    const uint4 ag3 = gload(reinterpret_cast<const uint4*>(p.agent + env) + 3);   // inventory, step_no, pack
    const int step_no = (int)(ag3.w & 0xffffu), active = (int)((ag3.w >> 18) & 7u);
    const bool time_up = step_no + 1 == p.max_steps;
    const uint32_t bits = (uint32_t)__ballot(lane < kActions && gload(p.mask + env * kActions + (lane < kActions ? lane : 0)) != 0);
    const int look0 = gload(p.look + 2 * env), look1 = gload(p.look + 2 * env + 1);
    double reward = 0.0 * p.wrong_scale;   // what the step pays an action that leaves the grid alone
    bool done = (cached == tsize) | time_up;
    wave_sync();
    const int q = lane & 3, mi = lane >> 2;
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
        const int a = j < 6 ? 6 + j : 10 + j;   // 6..11, 16, 17
        const bool hotbar = j < 6;
        if (!((bits >> a) & 1u) || (hotbar && !p.select_and_place)) continue;
        const int cell = a == 16 ? look0 : look1;
        if ((unsigned)cell >= (unsigned)CELLS) {   // (a hotbar colour that can be placed where the active one cannot)
            if (lane == a) reward = (double)__builtin_nanf("");
            continue;
        }
        const int g = gload(grid_g + cell), st = has_start ? (int)gload(start_g + cell) : 0;
        const int s0 = g - st, s1 = (a == 16 ? 0 : hotbar ? a - 5 : active) - st;
        const int wrong = (int)(s0 != 0) - (int)(s1 != 0);
        int m = cached;
        if (wrong != 0) {
            const int lvl = cell / LEVEL, rem = cell - lvl * LEVEL, gx = rem / 11, gz = rem - gx * 11;
            if (lane < kLvlBytes / 16)
                reinterpret_cast<uint4*>(ws.lvl)[lane] =
                    gload(reinterpret_cast<const uint4*>(p.task_index + task * IGW_TASK_INDEX_BYTES + lvl * kLvlBytes) + lane);
            wave_sync();
            // the two colour classes' slices of the level's cell list; rotation q's admissible translations
            const uint8_t* blk = ws.lvl;
            const int ka = class1(s0), kb = class1(s1);
            const int oa0 = blk[kLvlOffs - 1 + ka], oa1 = blk[kLvlOffs + ka], ob0 = blk[kLvlOffs - 1 + kb], ob1 = blk[kLvlOffs + kb];
            const int na = ka != 0 ? oa1 - oa0 : 0, nv = na + (kb != 0 ? ob1 - ob0 : 0);
            const int bb = (int)reinterpret_cast<const uint32_t*>(blk)[q];
            const int xmin = (int)(int8_t)(bb & 0xff), dxlo = (int)(int8_t)((bb >> 8) & 0xff) - 10;
            const int zmin = (int)(int8_t)((bb >> 16) & 0xff), dzlo = (int)(int8_t)((bb >> 24) & 0xff) - 10;
            for (int i0 = 0; i0 < nv; i0 += WAVE / 4) {
                const int idx = i0 + mi;
                if (idx < nv) {
                    const bool dec = idx < na;   // a target cell of the old colour stops matching, one of the new starts to
                    const int tc = blk[kLvlCells + (dec ? oa0 + idx : ob0 + (idx - na))];
                    const int tx = tc >> 4, tz = tc & 15;
                    const int bx = (q & 1) ? tz : tx, bz = (q & 1) ? tx : tz;
                    const int rx = q >= 2 ? 10 - bx : bx, rz = (q == 1 || q == 2) ? 10 - bz : bz;
                    const int u = rx - gx - dxlo, v = rz - gz - dzlo;
                    if ((unsigned)u <= (unsigned)(xmin - dxlo) && (unsigned)v <= (unsigned)(zmin - dzlo)) {
                        const int bin = q * LEVEL + u * 11 + v;
                        atomicAdd(&ws.hist[bin >> 1], (dec ? 0xffffffffu : 1u) << (16 * (bin & 1)));
                    }
                }
            }
            wave_sync();
            m = wave_max_nonneg(row_piece_max(reinterpret_cast<const uint4*>(ws.hist)[lane]));
            reinterpret_cast<uint4*>(ws.hist)[lane] = row;   // the live row again
            wave_sync();
        }
        const int right = m - cached;
        if (lane == a) {
            reward = right != 0 ? (double)right * p.right_scale : (double)wrong * p.wrong_scale;
            done = (m == tsize) | time_up;
        }
    }
    if (lane < kActions) {
        if (p.gain) gstore(p.gain + env * kActions + lane, (float)reward);
        if (p.ends) gstore(p.ends + env * kActions + lane, (uint8_t)done);
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_goal: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_GOAL_BUILD_ID
#define IGW_GOAL_BUILD_ID "igw-goal-build-id:unstamped"
#endif

extern "C" {

int igw_goal_version(void) { return IGW_GOAL_VERSION; }
// (the string carries a marker so that goal.py can read the id of a library file without loading it)
const char* igw_goal_build_id(void) { return &IGW_GOAL_BUILD_ID[sizeof("igw-goal-build-id:") - 1]; }
const char* igw_goal_last_error(void) { return g_err; }

int igw_goal(const int8_t* grid, const uint16_t* hist, const void* aux, const void* agent, const int8_t* task_target,
             const int8_t* task_start, const void* task_meta, const uint8_t* task_index, int32_t n,
             double right_placement_scale, double wrong_placement_scale, int32_t max_steps, int32_t select_and_place,
             const uint8_t* mask, const int16_t* look, int8_t* align, int16_t* fit, int8_t* want, int8_t* todo,
             float* gain, uint8_t* ends, void* stream) {
    if (!grid || !hist || !aux || !agent || !task_target || !task_start || !task_meta || !task_index)
        return fail(IGW_GOAL_ERR_INVALID, "grid, hist, aux, agent and the task-table buffers must not be NULL");
    if (n < 0) return fail(IGW_GOAL_ERR_INVALID, "n must be >= 0");
    if (!aligned(grid, 16) || !aligned(hist, 16) || !aligned(aux, 16) || !aligned(agent, 16) || !aligned(task_target, 16) ||
        !aligned(task_start, 16) || !aligned(task_meta, 16) || !aligned(task_index, 16))
        return fail(IGW_GOAL_ERR_INVALID, "the state and task-table buffers must be 16-byte aligned");
    if (!aligned(align, 4) || !aligned(fit, 8) || !aligned(want, 16) || !aligned(todo, 16) || !aligned(gain, 4) || !aligned(look, 2))
        return fail(IGW_GOAL_ERR_INVALID, "align must be 4-byte, fit 8-byte, want and todo 16-byte, gain 4-byte, look 2-byte aligned");
    if (gain || ends) {
        if (!mask || !look) return fail(IGW_GOAL_ERR_INVALID, "gain and ends need mask and look (igw_action_mask)");
        if (max_steps < 1 || max_steps > 65534) return fail(IGW_GOAL_ERR_INVALID, "max_steps must be in 1..65534");
    }
    if (n == 0) return IGW_GOAL_OK;
    GoalParams p;
    p.grid = grid; p.hist = hist; p.aux = static_cast<const AuxRec*>(aux); p.agent = static_cast<const AgentRec*>(agent);
    p.task_target = task_target; p.task_start = task_start; p.task_meta = static_cast<const TaskMeta*>(task_meta);
    p.task_index = task_index; p.mask = mask; p.look = look;
    p.align = align; p.fit = fit; p.want = want; p.todo = todo; p.gain = gain; p.ends = ends;
    p.right_scale = right_placement_scale; p.wrong_scale = wrong_placement_scale;
    p.n = n; p.max_steps = max_steps; p.select_and_place = select_and_place;
    const unsigned blocks = (unsigned)(((int64_t)n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
    hipLaunchKernelGGL(igw_goal_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_GOAL_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_GOAL_OK;
}

}  // extern "C"
