// igw_worth.hip -- libigw_worth.so: igw_worth (include/igw_worth.h), what the step would pay for every single-cell edit
// of each env's live state -- a break of every block, a place of each of the six colours into every empty cell -- and
// the best-paid edit among the ones the caller allows, in one launch.
//
// One wavefront owns an env, a block four; nothing synchronises across wavefronts.  The env's histogram row (1 KB), its
// task's colour index (1,440 B), its grid row and -- where the task has one -- its start row go to LDS once.  The row
// maximum M and the number of bins that hold it are taken once per env (a packed 16-bit maximum and a DPP reduction, a
// count and a butterfly sum).
//   An edit changes one cell's synthetic value between 0 and one colour v, so it only adds that colour's votes or only
//   removes them (with both values non-zero the step does not recount and the edit is paid from the cached maximum).
//   Most edits touch no bin: a place of colour k into an untouched cell on a level where no target cell has k's colour
//   class is paid M - cached whatever the cell.  Per plane the whole row is first staged with that one word where the
//   cell is empty and -1 elsewhere, EIGHT cells per lane (the grid bytes as one 8-byte LDS read, the zero bytes found
//   with integer arithmetic, one dwordx4 written to the LDS staging row); the levels that do hold such a target cell
//   (one ballot over the colour index per env; every level for the breaks and for a task with a starting grid, whose
//   cells have values of their own) are then worked out a LANE per cell: the lane walks the level's target cells of
//   v's colour class (a slice of the colour index) and the four rotations, the arithmetic of the step's histogram
//   update with a lane per cell (the index's layout, class1, row_piece_max and wave_sum_i32 are igw_vote.h's, the query
//   libraries' one copy).
//     adding:    m' = max(M, max over the touched admissible bins of h + 1): no copy of the row;
//     removing:  the touched bins are distinct, so the maximum falls -- to exactly M - 1, every bin that held M now
//                holds M - 1 and no other held more -- if and only if every bin that holds M is touched: the lane counts
//                its touched bins at M against the env's count.  No rescan, no LDS atomics.
//   The staged row leaves as 138 whole dwordx4 stores; the 15 pad words are staged as -1 with the rest.
//   best: every lane keeps the best candidate of the edits it owned (reward as binary64, then the lowest plane * 2048
//   + cell; the quiet cells of a chunk offer their lowest), the wavefront reduces with a butterfly, lane 0 stores the
//   16 bytes.
// Vector stores only; every loop is static or bounded by the 121 cells of a level times four rotations.
#include <stdio.h>

#include "../igw_vote.h"
#include "../../../include/igw_worth.h"

namespace {

using namespace igw;

constexpr int kPlanes = IGW_WORTH_PLANES;
constexpr int kIndexChunks = IGW_TASK_INDEX_BYTES / 16;
constexpr int kWordChunks = STRIDE * 2 / 16;       // 138 dwordx4 per plane row of int16 words
constexpr int kNoEdit = 0x7fffffff;
static_assert(IGW_WORTH_ROW == STRIDE && IGW_WORTH_CELLS == CELLS, "a plane has the layout of a grid row");
static_assert(kIndexChunks <= 2 * WAVE && kWordChunks <= 3 * WAVE && STRIDE % 8 == 0, "rows in dwordx4 per lane");

struct WorthParams {
    const int8_t* grid;
    const uint16_t* hist;
    const AuxRec* aux;
    const AgentRec* agent;
    const int8_t* task_start;
    const TaskMeta* task_meta;
    const uint8_t* task_index;
    const uint8_t* allow;
    int16_t* word;
    int32_t* best;
    double right_scale, wrong_scale;
    int32_t n, max_steps, stocked;
};

struct WaveShared {
    alignas(16) uint16_t hist[HIST_ROW];
    alignas(16) uint8_t index[IGW_TASK_INDEX_BYTES];
    alignas(16) int8_t grid[STRIDE];
    alignas(16) int8_t start[STRIDE];
    alignas(16) int16_t stage[STRIDE];
};

// bit j: byte j of x is 0
__device__ inline uint32_t zero_bytes(uint32_t x) {
    const uint32_t z = (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
    return (z | z >> 7 | z >> 14 | z >> 21) & 0xfu;
}

__global__ __launch_bounds__(BLOCK) void igw_worth_kernel(const WorthParams p) {
    __shared__ WaveShared sh[WAVES_PER_BLOCK];
    const int lane = __lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
    const int64_t env = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
    if (env >= p.n) return;
    WaveShared& ws = sh[wave];

    // ---- the row, the episode and agent records, the task's rows
    const uint4 row = gload(reinterpret_cast<const uint4*>(p.hist + env * HIST_ROW) + lane);
    const uint4 auxw = gload(reinterpret_cast<const uint4*>(p.aux + env));
    const int cached = (int)(int16_t)(auxw.y & 0xffffu), tsize = (int)(int16_t)(auxw.y >> 16);
    const int64_t task = (int64_t)__builtin_amdgcn_readfirstlane((int)auxw.z);
    const TaskMeta* meta = p.task_meta + task;
    const bool has_start = __builtin_amdgcn_readfirstlane((int)gload(&meta->has_start)) != 0;
    const uint4 ag3 = gload(reinterpret_cast<const uint4*>(p.agent + env) + 3);   // inventory, step_no, pack
    const bool time_up = (int)(ag3.w & 0xffffu) + 1 == p.max_steps;
    reinterpret_cast<uint4*>(ws.hist)[lane] = row;
    row_to_lds_wave(ws.grid, p.grid + env * STRIDE);
    if (has_start) row_to_lds_wave(ws.start, p.task_start + task * STRIDE);
    for (int c = lane; c < kIndexChunks; c += WAVE)
        reinterpret_cast<uint4*>(ws.index)[c] = gload(reinterpret_cast<const uint4*>(p.task_index + task * IGW_TASK_INDEX_BYTES) + c);

    // ---- the row maximum and the number of bins that hold it
    const int M = wave_max_nonneg(row_piece_max(row));
    int at_max = 0;
    {
        const uint32_t w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
        for (int j = 0; j < 4; j++) at_max += (int)((int)(w[j] & 0xffffu) == M) + (int)((int)(w[j] >> 16) == M);
    }
    const int n_max = wave_sum_i32(at_max);
    wave_sync();
    // the four rotations' bounding boxes (xmin, xmax, zmin, zmax), from the colour index's copy: held in vector registers
    uint32_t bbox[4];
#pragma unroll
    for (int q = 0; q < 4; q++) bbox[q] = reinterpret_cast<const uint32_t*>(ws.index)[q];

    // ---- what most edits share: a place into an untouched cell on a level without a target cell of the colour's class
    // touches no bin, so it is paid M - cached whatever the cell (wrong = -1)
    const int gap = M - cached;
    const int quiet_word = (gap & 0xfff) | (int)((M == tsize) | time_up) << 14;
    // bit (k - 1) * 9 + y: level y holds a target cell of colour k's class (k = 1..6)
    const int bk = lane / 9 + 1 + 7, by = lane % 9;   // class1(k) = k + 7
    const uint64_t held = __ballot(lane < 54 && ws.index[by * kLvlBytes + kLvlOffs - 1 + bk] < ws.index[by * kLvlBytes + kLvlOffs + bk]);

    const uint8_t* allow_g = p.allow ? p.allow + env * (2 * STRIDE) : nullptr;
    const bool want_best = p.best != nullptr;
    double best_reward = 0.0;
    int best_edit = kNoEdit, best_word = -1, candidates = 0;
    auto offer = [&](double reward, int edit, int w) {   // (lanes do not meet their edits in order)
        if (best_edit == kNoEdit || reward > best_reward || (reward == best_reward && edit < best_edit)) {
            best_reward = reward;
            best_edit = edit;
            best_word = w;
        }
    };

#pragma unroll 1
    for (int plane = 0; plane < kPlanes; plane++) {
        bool open = want_best;   // may the edits of this plane be candidates?
        if (plane > 0 && p.stocked) {
            const uint32_t pair = plane <= 2 ? ag3.x : plane <= 4 ? ag3.y : ag3.z;
            open = open && ((plane & 1) ? inv_lo(pair) : inv_hi(pair)) > 0;
        }
        // the levels whose cells are worked out one by one: all of them for the breaks and where cells have a start value
        const uint32_t busy = (plane == 0 || has_start) ? 0x1ffu : (uint32_t)(held >> ((plane - 1) * 9)) & 0x1ffu;

        // ---- the whole row, eight cells per lane: the quiet word where the cell is empty, -1 elsewhere and in the pad
        for (int c = lane; c < kWordChunks; c += WAVE) {
            const uint2 gb = reinterpret_cast<const uint2*>(ws.grid)[c];
            const int nvalid = min(max(CELLS - 8 * c, 0), 8);
            const uint32_t fill = plane == 0 ? 0u : (zero_bytes(gb.x) | zero_bytes(gb.y) << 4) & ((1u << nvalid) - 1u);
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                h[j] = (((fill >> (2 * j)) & 1u) ? (uint32_t)quiet_word : 0xffffu) |
                       (((fill >> (2 * j + 1)) & 1u) ? (uint32_t)quiet_word : 0xffffu) << 16;
            reinterpret_cast<uint4*>(ws.stage)[c] = make_uint4(h[0], h[1], h[2], h[3]);
            if (open && fill != 0u) {   // the candidates among them: the cells of the quiet levels that the gate lets through
                const int l0 = (8 * c) / LEVEL, b = (l0 + 1) * LEVEL - 8 * c;   // cells j < b of the chunk lie on level l0
                const uint32_t low = b >= 8 ? 0xffu : (1u << b) - 1u;
                uint32_t cand = fill & ((((busy >> l0) & 1u) ? 0u : low) | (((busy >> (l0 + 1)) & 1u) ? 0u : (low ^ 0xffu)));
                if (allow_g && cand != 0u) {
                    const uint2 ab = gload(reinterpret_cast<const uint2*>(allow_g + STRIDE) + c);
                    cand &= ~(zero_bytes(ab.x) | zero_bytes(ab.y) << 4);
                }
                if (cand != 0u) {
                    candidates += __popc(cand);
                    offer(gap != 0 ? (double)gap * p.right_scale : -1.0 * p.wrong_scale, plane * 2048 + 8 * c + (__ffs((int)cand) - 1),
                          quiet_word);
                }
            }
        }
        wave_sync();

        // ---- the busy levels, a lane per cell
#pragma unroll 1
        for (uint32_t left = busy; left != 0u; left &= left - 1u) {
            const int lvl = __ffs((int)left) - 1;
            const uint8_t* blk = ws.index + lvl * kLvlBytes;
#pragma unroll 1
            for (int r = lane; r < LEVEL; r += WAVE) {
                const int cell = lvl * LEVEL + r, gx = r / 11, gz = r - gx * 11;
                int w = -1;
                const int g = ws.grid[cell], st = has_start ? (int)ws.start[cell] : 0;
                if ((plane == 0) == (g != 0)) {
                    const int s0 = plane == 0 ? g - st : -st, s1 = plane - st;   // (a break leaves block id 0 = plane)
                    const int wrong = (int)(s0 != 0) - (int)(s1 != 0);
                    int m = cached;
                    if (wrong != 0) {
                        const bool add = s0 == 0;
                        const int k = class1(add ? s1 : s0);
                        const int i0 = blk[kLvlOffs - 1 + k], i1 = k != 0 ? min((int)blk[kLvlOffs + k], LEVEL) : 0;
                        int top = M, hit = 0;
                        for (int i = i0; i < i1; i++) {
                            const int tc = blk[kLvlCells + i];
                            const int tx = tc >> 4, tz = tc & 15;
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                const int bx = (q & 1) ? tz : tx, bz = (q & 1) ? tx : tz;
                                const int rx = q >= 2 ? 10 - bx : bx, rz = (q == 1 || q == 2) ? 10 - bz : bz;
                                // rotation q's admissible translations, as the step's histogram update reads them
                                const int bb = (int)bbox[q];
                                const int xmin = (int)(int8_t)(bb & 0xff), dxlo = (int)(int8_t)((bb >> 8) & 0xff) - 10;
                                const int zmin = (int)(int8_t)((bb >> 16) & 0xff), dzlo = (int)(int8_t)((bb >> 24) & 0xff) - 10;
                                const int u = rx - gx - dxlo, v = rz - gz - dzlo;
                                if ((unsigned)u <= (unsigned)(xmin - dxlo) && (unsigned)v <= (unsigned)(zmin - dzlo)) {
                                    const int h = ws.hist[q * LEVEL + u * 11 + v];
                                    top = max(top, h + 1);
                                    hit += (int)(h == M);
                                }
                            }
                        }
                        m = add ? top : (M > 0 && hit == n_max) ? M - 1 : M;
                    }
                    const int right = m - cached;
                    const bool done = (m == tsize) | time_up;
                    w = (right & 0xfff) | (wrong + 1) << 12 | (int)done << 14;
                    if (open && (!allow_g || gload(allow_g + (plane == 0 ? 0 : STRIDE) + cell) != 0)) {
                        candidates++;
                        offer(right != 0 ? (double)right * p.right_scale : (double)wrong * p.wrong_scale, plane * 2048 + cell, w);
                    }
                }
                ws.stage[cell] = (int16_t)w;
            }
        }
        if (p.word) {
            wave_sync();
            uint4* dst = reinterpret_cast<uint4*>(p.word + (env * kPlanes + plane) * STRIDE);
            for (int c = lane; c < kWordChunks; c += WAVE) gstore(dst + c, reinterpret_cast<const uint4*>(ws.stage)[c]);
        }
        wave_sync();
    }

    if (want_best) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double r = __shfl_xor(best_reward, o, 64);
            const int e = __shfl_xor(best_edit, o, 64), w = __shfl_xor(best_word, o, 64);
            if (e != kNoEdit && (best_edit == kNoEdit || r > best_reward || (r == best_reward && e < best_edit))) {
                best_reward = r;
                best_edit = e;
                best_word = w;
            }
        }
        const int total = wave_sum_i32(candidates);
        if (lane == 0) {
            const bool any = best_edit != kNoEdit;
            gstore(reinterpret_cast<uint4*>(p.best) + env,
                   make_uint4((uint32_t)(any ? best_edit >> 11 : -1), (uint32_t)(any ? best_edit & 2047 : -1),
                              (uint32_t)(any ? best_word : -1), (uint32_t)total));
        }
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_worth: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_WORTH_BUILD_ID
#define IGW_WORTH_BUILD_ID "igw-worth-build-id:unstamped"
#endif

extern "C" {

int igw_worth_version(void) { return IGW_WORTH_VERSION; }
// (the string carries a marker so that worth.py can read the id of a library file without loading it)
const char* igw_worth_build_id(void) { return &IGW_WORTH_BUILD_ID[sizeof("igw-worth-build-id:") - 1]; }
const char* igw_worth_last_error(void) { return g_err; }

int igw_worth(const int8_t* grid, const uint16_t* hist, const void* aux, const void* agent, const int8_t* task_target,
              const int8_t* task_start, const void* task_meta, const uint8_t* task_index, int32_t n, int32_t max_steps,
              const uint8_t* allow, int32_t stocked, double right_scale, double wrong_scale, int16_t* word,
              int32_t* best, void* stream) {
    if (!grid || !hist || !aux || !agent || !task_target || !task_start || !task_meta || !task_index)
        return fail(IGW_WORTH_ERR_INVALID, "grid, hist, aux, agent and the task-table buffers must not be NULL");
    if (!word && !best) return fail(IGW_WORTH_ERR_INVALID, "word and best are both NULL: nothing to compute");
    if (n < 0) return fail(IGW_WORTH_ERR_INVALID, "n must be >= 0");
    if (!aligned(grid, 16) || !aligned(hist, 16) || !aligned(aux, 16) || !aligned(agent, 16) || !aligned(task_target, 16) ||
        !aligned(task_start, 16) || !aligned(task_meta, 16) || !aligned(task_index, 16))
        return fail(IGW_WORTH_ERR_INVALID, "the state and task-table buffers must be 16-byte aligned");
    if (!aligned(word, 16) || !aligned(best, 16) || !aligned(allow, 16))
        return fail(IGW_WORTH_ERR_INVALID, "word, best and allow must be 16-byte aligned");
    if (max_steps < 1 || max_steps > 65534) return fail(IGW_WORTH_ERR_INVALID, "max_steps must be in 1..65534");
    if (n == 0) return IGW_WORTH_OK;
    WorthParams p;
    p.grid = grid; p.hist = hist; p.aux = static_cast<const AuxRec*>(aux); p.agent = static_cast<const AgentRec*>(agent);
    p.task_start = task_start; p.task_meta = static_cast<const TaskMeta*>(task_meta); p.task_index = task_index;
    p.allow = allow; p.word = word; p.best = best;
    p.right_scale = right_scale; p.wrong_scale = wrong_scale;
    p.n = n; p.max_steps = max_steps; p.stocked = stocked;
    const unsigned blocks = (unsigned)(((int64_t)n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
    hipLaunchKernelGGL(igw_worth_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_WORTH_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_WORTH_OK;
}

}  // extern "C"
