// igw_relabel.hip -- libigw_relabel.so: igw_relabel (include/igw_relabel.h), the reward, done and cached max_int of every
// step of E logged episodes under G other targets each (hindsight relabelling), from the log's change words alone, in
// one launch that reads no env state and writes nothing but its answers.
//
// One wavefront owns a pair (episode, goal), a block the four goals 4c .. 4c + 3 of ONE episode: the episode's starting
// row and its change words -- 256 records at a time, the u16 at byte 40 of each -- are staged once per block and shared
// by its wavefronts.  Per wavefront in LDS: the synthetic target (goal - start), the episode's grid as the walk has it,
// the target's colour index (the task table's layout, include/igw.h, built here by a counting sort per level) and the
// 4 x 11 x 11 vote histogram (the step's row: 16-bit counts, two per word).
//   A goal given as an entry (`at`) is rebuilt first: the block walks the change words once, every wavefront applying
//   the ones below its own entry to its copy of the starting row.
//   The scoring walks the CHANGES, not the steps: of every 64 records (a lane each) a ballot keeps the ones that changed
//   a cell; per change the wavefront votes with LDS atomics (vote_change of igw_vote.h, the query libraries' one copy of
//   the step's histogram update: the target cells of the
//   cell's level and old colour lose a vote per rotation and admissible translation, those of the new colour gain one)
//   and retakes the row maximum only when the block count of grid - start moved (a packed 16-bit maximum per lane and a
//   DPP reduction); a cell recoloured in place votes but leaves the cached maximum as it is, as the step does.  The lanes
//   at and behind the change take the new cached value, so the steps between two changes cost nothing: every lane then
//   forms its own step's reward and done and stores them, 64 steps per store instruction.
//   ret: gamma's powers come from one multiplication per step (the recurrence's own), a lane's term is g * reward, and
//   the sum takes the non-zero terms in step order (ret + 0.0 is ret: ret is never -0.0).
// Vector stores only.  Every loop is bounded by L, by the 64 lanes of a ballot or by the 121 cells of a level.
#include <stdio.h>

#include "../igw_vote.h"
#include "../../../include/igw_relabel.h"

namespace {

using namespace igw;

constexpr int kChunk = BLOCK;                      // records staged per round: one per thread
constexpr int kSubs = kChunk / WAVE;
constexpr int kChangeOffset = 40;                  // the u16 `change` of a trajectory record
static_assert(IGW_RELABEL_ROW == STRIDE && IGW_RELABEL_CELLS == CELLS && IGW_RELABEL_RECORD == IGW_TRAJ_BYTES, "layouts of include/igw.h");
static_assert(CELLS <= 0x7ff, "a cell fits the low 11 bits of a change");

struct RelabelParams {
    const uint8_t* records;
    const int64_t* first;
    const int32_t* length;
    const int8_t* start;
    const int8_t* targets;
    const int32_t* at;
    float* reward;
    uint8_t* done;
    int16_t* progress;
    int32_t* end;
    float* ret;
    int16_t* tsize;
    int8_t* target;
    double right_scale, wrong_scale, gamma;
    int64_t n_records;
    int32_t E, G, L, gchunks, max_steps;
};

struct WaveShared {
    alignas(16) int8_t tgt[STRIDE];                   // the synthetic target: goal - start
    alignas(16) int8_t grid[STRIDE];                  // the goal while it is built, then the episode's grid as walked
    alignas(16) uint32_t hist[HIST_ROW / 2];          // votes of grid - start against tgt
    alignas(16) uint8_t index[IGW_TASK_INDEX_BYTES];  // colour index of tgt
};
struct Shared {
    alignas(16) int8_t start[STRIDE];
    alignas(16) uint16_t chg[kChunk];
    WaveShared w[WAVES_PER_BLOCK];
};

__device__ inline double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__device__ inline int pack_bbox(int xmin, int xmax, int zmin, int zmax) {
    return (xmin & 0xff) | ((xmax & 0xff) << 8) | ((zmin & 0xff) << 16) | ((zmax & 0xff) << 24);
}

// Size, bounding box and the four rotations' boxes of the synthetic target (Task.__init__, tasks/task.py:52-72 as the
// box rule of igw_kernels.hip: admissible translations of rotation r are dx in [xmax - 10, xmin], dz in [zmax - 10,
// zmin]; an empty target has the box (10, 0, 10, 0)).  Returns the number of non-zero cells.
__device__ inline int target_boxes(const int8_t* tgt_s, int* bb4) {
    const int lane = __lane_id();
    int xmin = 10, xmax = 0, zmin = 10, zmax = 0, cnt = 0;
    for (int c = lane; c < CELLS; c += WAVE) {
        if (tgt_s[c] != 0) {
            const int r = c % LEVEL, x = r / 11, z = r - x * 11;
            xmin = min(xmin, x); xmax = max(xmax, x);
            zmin = min(zmin, z); zmax = max(zmax, z);
            cnt++;
        }
    }
    cnt = wave_sum_i32(cnt);
    xmin = wave_min_i32(xmin); xmax = wave_max_i32(xmax);
    zmin = wave_min_i32(zmin); zmax = wave_max_i32(zmax);
    if (cnt == 0) {
        bb4[0] = bb4[1] = bb4[2] = bb4[3] = pack_bbox(10, 0, 10, 0);
        return 0;
    }
    bb4[0] = pack_bbox(xmin, xmax, zmin, zmax);
    bb4[1] = pack_bbox(zmin, zmax, 10 - xmax, 10 - xmin);
    bb4[2] = pack_bbox(10 - xmax, 10 - xmin, 10 - zmax, 10 - zmin);
    bb4[3] = pack_bbox(10 - zmax, 10 - zmin, xmin, xmax);
    return cnt;
}

// The colour index of the synthetic target in LDS (build_level_index_wave of igw_kernels.hip, written in place): per y
// level the four boxes, offs[15] and the level's target cells sorted by colour class -- a counting sort by the whole
// wavefront, two cells per lane.
__device__ inline int index_class(int c) { return (c == 0 || c < -7 || c > 7) ? -1 : (c < 0 ? c + 7 : c + 6); }
__device__ inline void build_index(const int8_t* tgt_s, const int* bb4, uint8_t* index_s) {
    const int lane = __lane_id();
    const int c0 = lane, c1 = lane + 64;
    const bool v1 = c1 < LEVEL;
    const uint32_t p0 = (uint32_t)((c0 / 11) << 4 | (c0 % 11)), p1 = (uint32_t)((c1 / 11) << 4 | (c1 % 11));
    for (int y = 0; y < IGW_GRID_Y; y++) {
        uint8_t* blk = index_s + y * kLvlBytes;
        const int k0 = index_class(tgt_s[y * LEVEL + c0]), k1 = v1 ? index_class(tgt_s[y * LEVEL + c1]) : -1;
        if (lane < kLvlBytes / 16)
            reinterpret_cast<uint4*>(blk)[lane] = lane == 0 ? make_uint4((uint32_t)bb4[0], (uint32_t)bb4[1], (uint32_t)bb4[2], (uint32_t)bb4[3])
                                                             : make_uint4(0, 0, 0, 0);
        wave_sync();
        if (__ballot(k0 >= 0 || k1 >= 0)) {   // (most levels of most targets are empty: all offsets stay 0)
            int off = 0;
            for (int k = 0; k < 14; k++) {
                const uint64_t m0 = __ballot(k0 == k), m1 = __ballot(k1 == k);
                const int n0 = __builtin_popcountll(m0);
                if (lane == 0) blk[kLvlOffs + k] = (uint8_t)off;
                if (k0 == k) blk[kLvlCells + off + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u))] = (uint8_t)p0;
                if (k1 == k) blk[kLvlCells + off + n0 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u))] = (uint8_t)p1;
                off += n0 + __builtin_popcountll(m1);
            }
            if (lane == 0) blk[kLvlOffs + 14] = blk[kLvlOffs + 15] = (uint8_t)off;   // (offs[15] = offs[14]: the empty slice class1() clamps to)
        }
        wave_sync();
    }
}

// A 16-byte piece (chunk c) of a grid row with the block ids above `hi` and the 15 pad bytes behind cell 1088 read as 0
__device__ inline uint32_t keep_ids(uint32_t w, uint32_t hi) {
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = (w >> (8 * j)) & 0xffu;
        r |= (b <= hi ? b : 0u) << (8 * j);
    }
    return r;
}
__device__ inline uint4 clean_chunk(const uint4& v, int c, uint32_t hi) {
    const bool last = c == CHUNKS - 1;   // cells 1088 .. 1103: one cell, fifteen pad bytes
    return make_uint4(keep_ids(v.x, hi) & (last ? 0xffu : 0xffffffffu), last ? 0u : keep_ids(v.y, hi), last ? 0u : keep_ids(v.z, hi),
                      last ? 0u : keep_ids(v.w, hi));
}
static_assert(CELLS == 16 * (CHUNKS - 1) + 1, "the last chunk of a row holds one cell");

// +0 in steps [from, L) of a pair's per-step outputs
__device__ inline void pad_steps(const RelabelParams& p, int64_t off, int64_t from) {
    for (int64_t j = from + __lane_id(); j < p.L; j += WAVE) {
        if (p.reward) gstore(p.reward + off + j, 0.0f);
        if (p.done) gstore(p.done + off + j, (uint8_t)0);
        if (p.progress) gstore(p.progress + off + j, (int16_t)0);
    }
}

__global__ __launch_bounds__(BLOCK) void igw_relabel_kernel(const RelabelParams p) {
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x, lane = __lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t bid = (int64_t)blockIdx.x;
    const int64_t e = bid / p.gchunks;
    const int g = (int)(bid - e * p.gchunks) * WAVES_PER_BLOCK + wave;
    const bool active = g < p.G;                      // (a wavefront without a goal keeps the block's barriers company)
    const int64_t pair = e * p.G + (active ? g : 0);
    const int64_t off = pair * p.L;
    const int64_t first_v = gload(p.first + e);
    const int64_t first = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(first_v >> 32)) << 32) |
                                    (uint32_t)__builtin_amdgcn_readfirstlane((int)first_v));
    const int len = __builtin_amdgcn_readfirstlane(clampi(gload(p.length + e), 0, p.L));
    WaveShared& ws = sh.w[wave];

    if (first < 0 || first > p.n_records - len) {     // the episode is not in the buffer: padding only (block-uniform)
        if (active) {
            pad_steps(p, off, 0);
            if (p.target)
                for (int c = lane; c < CHUNKS; c += WAVE) gstore(reinterpret_cast<uint4*>(p.target + pair * STRIDE) + c, make_uint4(0, 0, 0, 0));
            if (lane == 0) {
                if (p.end) gstore(p.end + pair, 0);
                if (p.ret) gstore(p.ret + pair, 0.0f);
                if (p.tsize) gstore(p.tsize + pair, (int16_t)0);
            }
        }
        return;
    }

    // ---- the starting row, once per block (a cell outside 0..6 reads as empty, as in the task table)
    if (tid < CHUNKS)
        reinterpret_cast<uint4*>(sh.start)[tid] = clean_chunk(gload(reinterpret_cast<const uint4*>(p.start + e * STRIDE) + tid), tid, 6u);
    const uint8_t* rec_g = p.records + first * IGW_TRAJ_BYTES + kChangeOffset;
    const auto stage = [&](int base) {                // the change words of records base .. base + 255 of the episode
        const int j = base + tid;
        sh.chg[tid] = j < len ? gload(reinterpret_cast<const uint16_t*>(rec_g + (int64_t)j * IGW_TRAJ_BYTES)) : (uint16_t)0xffffu;
    };
    __syncthreads();

    // ---- the goal grid
    if (p.at == nullptr) {
        if (active) {
            const uint4* tg = reinterpret_cast<const uint4*>(p.targets + pair * STRIDE);
            for (int c = lane; c < CHUNKS; c += WAVE) reinterpret_cast<uint4*>(ws.grid)[c] = clean_chunk(gload(tg + c), c, 7u);
        }
    } else {
        const int a = __builtin_amdgcn_readfirstlane(active ? clampi(gload(p.at + pair), 0, len) : 0);
        for (int c = lane; c < CHUNKS; c += WAVE) reinterpret_cast<uint4*>(ws.grid)[c] = reinterpret_cast<const uint4*>(sh.start)[c];
        wave_sync();
        for (int base = 0; base < len; base += kChunk) {
            stage(base);
            __syncthreads();
            for (int sub = 0; sub < kSubs; sub++) {
                const int t0 = base + sub * WAVE;
                if (t0 >= a) break;
                const int w = sh.chg[sub * WAVE + lane];
                uint64_t mask = __ballot(t0 + lane < a && w != 0xffff && (w & 0x7ff) < CELLS);
                while (mask != 0) {                   // in step order: a cell may change more than once
                    const int b = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int wv = __builtin_amdgcn_readlane(w, b);
                    if (lane == 0) ws.grid[wv & 0x7ff] = (int8_t)((wv >> 11) & 7);
                }
            }
            __syncthreads();
        }
    }
    wave_sync();

    // ---- the synthetic target, its size, boxes and colour index; the walk starts from the starting row
    int tsize = 0;
    if (active) {
        if (p.target)
            for (int c = lane; c < CHUNKS; c += WAVE)
                gstore(reinterpret_cast<uint4*>(p.target + pair * STRIDE) + c, reinterpret_cast<const uint4*>(ws.grid)[c]);
        for (int c = lane; c < STRIDE; c += WAVE) {
            const int st = sh.start[c];
            ws.tgt[c] = (int8_t)(ws.grid[c] - st);
            ws.grid[c] = (int8_t)st;
        }
        reinterpret_cast<uint4*>(ws.hist)[lane] = make_uint4(0, 0, 0, 0);
        wave_sync();
        int bb4[4];
        tsize = target_boxes(ws.tgt, bb4);
        build_index(ws.tgt, bb4, ws.index);
    }

    // ---- the walk
    int cached = 0, end = 0;
    double ret = 0.0, gpow = 1.0;
    for (int base = 0; base < len; base += kChunk) {
        stage(base);
        __syncthreads();
        if (active) {
            for (int sub = 0; sub < kSubs; sub++) {
                const int t0 = base + sub * WAVE;
                if (t0 >= len) break;
                const int j = t0 + lane;              // this lane's record; its step number is j + 1
                const bool valid = j < len;
                const int w = sh.chg[sub * WAVE + lane];
                uint64_t mask = __ballot(valid && w != 0xffff && (w & 0x7ff) < CELLS);
                int mi_l = cached, wrong_l = 0, right_l = 0;
                while (mask != 0) {
                    const int b = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int wv = __builtin_amdgcn_readlane(w, b);
                    const int cell = wv & 0x7ff, col = (wv >> 11) & 7;
                    const int st = sh.start[cell];
                    const int s0 = (int)ws.grid[cell] - st, s1 = col - st;
                    if (lane == 0) ws.grid[cell] = (int8_t)col;
                    int now = cached;
                    if (s0 != s1) {
                        vote_change(ws.hist, ws.index, cell, s0, s1);
                        const int wrong = (int)(s0 != 0) - (int)(s1 != 0);
                        if (wrong != 0) {             // the block count moved: maximal_intersection is taken again
                            wave_sync();
                            now = wave_max_nonneg(row_piece_max(reinterpret_cast<const uint4*>(ws.hist)[lane]));
                        }
                        if (lane == b) {
                            wrong_l = wrong;
                            right_l = now - cached;
                        }
                    }
                    if (lane >= b) mi_l = now;
                    cached = now;
                    wave_sync();
                }
                const bool dn = valid && ((mi_l == tsize) | (j + 1 == p.max_steps));
                const double rw = right_l == 0 ? (double)wrong_l * p.wrong_scale : (double)right_l * p.right_scale;
                const bool ended = end != 0;          // before this round
                const uint64_t dmask = __ballot(dn);
                if (!ended && dmask != 0) end = t0 + __builtin_ctzll(dmask) + 1;
                if (p.ret && !ended) {
                    double my_g = 1.0;
                    const int nk = min(WAVE, len - t0);
                    for (int k = 0; k < nk; k++) {    // gamma's powers by the recurrence's own multiplications
                        my_g = lane == k ? gpow : my_g;
                        gpow = gpow * p.gamma;
                    }
                    const double term = my_g * rw;
                    uint64_t cmask = __ballot(valid && (end == 0 || j + 1 <= end) && !(term == 0.0));
                    while (cmask != 0) {
                        const int b = __builtin_ctzll(cmask);
                        cmask &= cmask - 1;
                        ret = ret + readlane_f64(term, b);
                    }
                }
                if (j < p.L) {                        // (lanes behind the episode's last step write padding)
                    if (p.reward) gstore(p.reward + off + j, valid ? (float)rw : 0.0f);
                    if (p.done) gstore(p.done + off + j, (uint8_t)dn);
                    if (p.progress) gstore(p.progress + off + j, (int16_t)(valid ? mi_l : 0));
                }
            }
        }
        __syncthreads();
    }
    if (active) {
        pad_steps(p, off, ((int64_t)len + WAVE - 1) / WAVE * WAVE);
        if (lane == 0) {
            if (p.end) gstore(p.end + pair, end);
            if (p.ret) gstore(p.ret + pair, (float)ret);
            if (p.tsize) gstore(p.tsize + pair, (int16_t)tsize);
        }
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_relabel: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_RELABEL_BUILD_ID
#define IGW_RELABEL_BUILD_ID "igw-relabel-build-id:unstamped"
#endif

extern "C" {

int igw_relabel_version(void) { return IGW_RELABEL_VERSION; }
// (the string carries a marker so that relabel.py can read the id of a library file without loading it)
const char* igw_relabel_build_id(void) { return &IGW_RELABEL_BUILD_ID[sizeof("igw-relabel-build-id:") - 1]; }
const char* igw_relabel_last_error(void) { return g_err; }

int igw_relabel(const void* records, int64_t n_records, const int64_t* first, const int32_t* length,
                const int8_t* start_grid, const int8_t* targets, const int32_t* at, int32_t E, int32_t G, int32_t L,
                double right_placement_scale, double wrong_placement_scale, int32_t max_steps, double gamma,
                float* reward, uint8_t* done, int16_t* progress, int32_t* end, float* ret, int16_t* target_size,
                int8_t* target, void* stream) {
    if (!records || !first || !length || !start_grid)
        return fail(IGW_RELABEL_ERR_INVALID, "records, first, length and start_grid must not be NULL");
    if ((targets != nullptr) == (at != nullptr))
        return fail(IGW_RELABEL_ERR_INVALID, "exactly one of targets and at must be given");
    if (!reward && !done && !progress && !end && !ret && !target_size && !target)
        return fail(IGW_RELABEL_ERR_INVALID, "at least one output must not be NULL");
    if (E < 0 || n_records < 0) return fail(IGW_RELABEL_ERR_INVALID, "E and n_records must be >= 0");
    if (G < 1 || G > IGW_RELABEL_MAX_G) return fail(IGW_RELABEL_ERR_INVALID, "G must be in 1..256");
    if (L < 1) return fail(IGW_RELABEL_ERR_INVALID, "L must be >= 1");
    if ((int64_t)E * G > 0 && (int64_t)L > ((1ll << 40) - 1) / ((int64_t)E * G))
        return fail(IGW_RELABEL_ERR_INVALID, "E * G * L must be below 2^40");
    if (max_steps < 1 || max_steps > 65534) return fail(IGW_RELABEL_ERR_INVALID, "max_steps must be in 1..65534");
    if (!__builtin_isfinite(gamma)) return fail(IGW_RELABEL_ERR_INVALID, "gamma must be finite");
    if (!aligned(start_grid, 16) || !aligned(targets, 16) || !aligned(target, 16))
        return fail(IGW_RELABEL_ERR_INVALID, "start_grid, targets and target must be 16-byte aligned");
    if (!aligned(first, 8) || !aligned(records, 4) || !aligned(length, 4) || !aligned(at, 4) || !aligned(reward, 4) ||
        !aligned(end, 4) || !aligned(ret, 4) || !aligned(progress, 2) || !aligned(target_size, 2))
        return fail(IGW_RELABEL_ERR_INVALID, "first must be 8-byte, records, length, at, reward, end and ret 4-byte, progress and target_size 2-byte aligned");
    if (E == 0) return IGW_RELABEL_OK;
    RelabelParams p;
    p.records = static_cast<const uint8_t*>(records); p.first = first; p.length = length; p.start = start_grid;
    p.targets = targets; p.at = at;
    p.reward = reward; p.done = done; p.progress = progress; p.end = end; p.ret = ret; p.tsize = target_size; p.target = target;
    p.right_scale = right_placement_scale; p.wrong_scale = wrong_placement_scale; p.gamma = gamma;
    p.n_records = n_records;
    p.E = E; p.G = G; p.L = L; p.gchunks = (G + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK; p.max_steps = max_steps;
    const int64_t blocks = (int64_t)E * p.gchunks;   // E < 2^31 and gchunks <= 64: the product is checked, not assumed
    if (blocks > 0x7fffffffll) return fail(IGW_RELABEL_ERR_INVALID, "E * ceil(G / 4) must be below 2^31");
    hipLaunchKernelGGL(igw_relabel_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(IGW_RELABEL_ERR_HIP, "launch failed: ", hipGetErrorString(err));
    return IGW_RELABEL_OK;
}

}  // extern "C"
