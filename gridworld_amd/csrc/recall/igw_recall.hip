// igw_recall.hip -- libigw_recall.so: igw_recall (include/igw_recall.h), the voxel observation before and after one
// logged step for B sampled (episode, step) pairs, rebuilt from the log's change words and f32 poses in one launch: the
// front of the relabel query (the walk over the change words) feeding the back of the voxel observation (the staged
// planes and the 16-byte streaming stores).  No env state is read, nothing but the outputs is written.
//
// One workgroup of 256 lanes per sample (e, t).
//   rebuild  The episode's 1104-byte starting row goes to LDS (69 dwordx4, a cell outside 0..6 as 0), the goal row beside
//            it (bytes, at any alignment).  The change words of records 0 .. lo - 1, lo = max(0, t - K), are read a lane
//            per record, 256 at a time (the u16 at byte 40 of each 64-byte record); the first wavefront keeps the
//            non-empty ones with a ballot and applies them in record order, so a cell changed twice ends as the later
//            word says.  The K + 1 entries lo .. t that the two stacks hold are then visited in order: each applies its
//            own word (at most 8 of them, kept in LDS), is staged once and written to every slot of obs and next_obs that
//            shows it.
//   stage    The pose is the reset pose in binary64 for entry 0 and the record's f32 agentPos widened for the others,
//            handed to every lane through LDS.  The channel table and the staging loop are csrc/igw_voxel_table.h and
//            igw_voxel_stage.h, statements included in the kernel body and shared with the voxel observation; a plane's
//            value at a world cell is the rebuilt grid's or the goal row's, both in LDS.
//   write    The element, the frame of a pose and the writer of a slot at the absolute 16-byte boundaries are
//            csrc/igw_voxel.h's, shared with the voxel observation too, where the stage / write story is told; the
//            stores are non-temporal.
//   A barrier separates the restaging of the planes from the previous entry's last reads of them.
// A padding sample writes the value of bit 0 to both of its runs, zeros to its record and 0 to its valid byte.
// Vector stores in plain C++ only.  Every loop is bounded by L, by the 64 lanes of a ballot or by the spec.
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "../../../include/igw_recall.h"
#include "../igw_voxel.h"

namespace {

using namespace voxel;

static_assert(IGW_RECALL_U8 == kU8 && IGW_RECALL_F16 == kF16 && IGW_RECALL_BF16 == kBF16 && IGW_RECALL_F32 == kF32, "element types");
static_assert(IGW_RECALL_ONEHOT == kOneHot && IGW_RECALL_OCC == kOcc, "encodings");
static_assert(IGW_RECALL_LEVELS == kLevels && IGW_RECALL_MAX_RADIUS == kMaxRadius && IGW_RECALL_MAX_PLANES == kMaxSources, "limits");
constexpr int kWave = 64;
constexpr int kRow = IGW_RECALL_ROW;
constexpr int kCells = IGW_RECALL_CELLS;
constexpr int kRecord = IGW_RECALL_RECORD;
constexpr int kChunks = kRow / 16;                               // 69 dwordx4 of a grid row
constexpr int kPlanes = kMaxSources + 1;                         // the spec's planes and the agent's
constexpr int kChangeOffset = 40;                                // the u16 `change` of a trajectory record
constexpr int kNone = 0xffff;
static_assert(kCells == 16 * (kChunks - 1) + 1, "the last chunk of a row holds one cell");
static_assert(kCells <= 0x7ff, "a cell fits the low 11 bits of a change");

struct RecallParams {
    void* obs;
    void* next_obs;
    const uint8_t* records;
    const double* init_pose;
    const int64_t* first;
    const int32_t* length;
    const int8_t* start;
    const int32_t* episode;
    const int32_t* step;
    const int8_t* goal;
    const int64_t* goal_index;
    uint8_t* record;
    uint8_t* valid;
    int64_t n_records, goal_stride, n_goal_rows;
    float scale, bias;
    int32_t E, L;
    uint32_t planes;            // two bits per plane: bit 2k its source, bit 2k + 1 its encoding
    int32_t nplanes, agent_plane, ego, R, dtype, stack, channels;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// A value every lane loaded from the same address, as the scalar it is
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    return (int64_t)(((uint64_t)(uint32_t)uniform((int)(v >> 32)) << 32) | (uint32_t)uniform((int)v));
}

// `n` elements of the value v0 from `base` on: a padding sample's run.
template <typename E>
__device__ __forceinline__ void fill_run(E* base, int n, E v0) {
    constexpr int P = 16 / (int)sizeof(E);
    const int tid = threadIdx.x;
    const Cut<E> cut(base, n);
    uint32_t w = v0;
    if constexpr (sizeof(E) == 1) w *= 0x01010101u;
    if constexpr (sizeof(E) == 2) w *= 0x00010001u;
    const u32x4 v{w, w, w, w};
#pragma unroll 1
    for (int p = tid; p < cut.pieces; p += kThreads) store16<true>(base + cut.head + p * P, v);
    const int edge = cut.head + (n - cut.tail);
    if (tid < edge) base[tid < cut.head ? tid : cut.tail + (tid - cut.head)] = v0;
}

// What a sample is, the same in every lane: its episode, its step, where its records lie, and whether it is padding.
struct Sample {
    int64_t e, first, goal_row;
    int t;
    bool pad;
};

template <int kDtype>
__device__ __forceinline__ void emit_padding(const RecallParams& p, int64_t b, int P9) {
    using E = typename Elem<kDtype>::E;
    const int n = p.stack * p.channels * P9;   // <= 8 * 25 * 3,969
    const E v0 = elem_value<kDtype>(0u, p.scale, p.bias);
    if (p.obs) fill_run<E>(static_cast<E*>(p.obs) + b * n, n, v0);
    if (p.next_obs) fill_run<E>(static_cast<E*>(p.next_obs) + b * n, n, v0);
}

// Entry s of sample (e, t), staged in `pl`, into the slots of obs and next_obs that show it.
template <int kDtype>
__device__ __forceinline__ void emit_entry(const RecallParams& p, int64_t b, int t, int s, const Planes& pl) {
    using E = typename Elem<kDtype>::E;
    const E v0 = elem_value<kDtype>(0u, p.scale, p.bias), v1 = elem_value<kDtype>(1u, p.scale, p.bias);
    const int K = p.stack, L = p.channels * pl.P9;
    E* obs = p.obs ? static_cast<E*>(p.obs) + b * K * (int64_t)L : nullptr;
    E* next = p.next_obs ? static_cast<E*>(p.next_obs) + b * K * (int64_t)L : nullptr;
#pragma unroll 1
    for (int j = 0; j < K; j++) {   // (block-uniform conditions)
        if (obs && max(0, t - K + j) == s) write_slot<kDtype, true>(obs + (int64_t)j * L, L, pl, v0, v1);
        if (next && max(0, t - K + 1 + j) == s) write_slot<kDtype, true>(next + (int64_t)j * L, L, pl, v0, v1);
    }
}

__device__ __forceinline__ int source_of(uint32_t planes, int k) { return (int)((planes >> (2 * k)) & 1u); }
__device__ __forceinline__ int encoding_of(uint32_t planes, int k) { return (int)((planes >> (2 * k + 1)) & 1u); }
static_assert(IGW_RECALL_GOAL == 1 && IGW_RECALL_OCC == 1, "a plane's source and encoding are a bit each");

// What igw_voxel_table.h and igw_voxel_stage.h take from this kernel: a plane's value is the rebuilt grid's or the goal
// row's, both in LDS.
#define VOXEL_PLANES p.nplanes
#define VOXEL_AGENT p.agent_plane
#define VOXEL_ENCODING(k) encoding_of(p.planes, k)
#define VOXEL_EGO p.ego
#define VOXEL_GUARD_CELL 1
#define VOXEL_READ(k, c, v) const int v = source_of(p.planes, k) == IGW_RECALL_GOAL ? (int)goal_row[c] : (int)grid[c];

// One kernel per element type: the type decides the stores, and four of them in one kernel cost scalar registers.
template <int kDtype>
__global__ __launch_bounds__(kThreads) void igw_recall_kernel(const RecallParams p) {
    __shared__ uint8_t cells[kPlanes * kMaxPlane];
    __shared__ alignas(16) uint8_t grid[kRow];
    __shared__ int8_t goal_row[kRow];
    __shared__ uint16_t chg[kThreads];
    __shared__ uint16_t own_word[IGW_RECALL_MAX_STACK];
    __shared__ double pose_s[4];
    __shared__ uint8_t ch_plane[kTable], ch_match[kTable];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = uniform(tid / kWave);
    const int64_t b = blockIdx.x;
    const int R = p.R, S = p.ego ? 2 * R + 1 : 11, SS = S * S, P9 = kLevels * SS;
    const int K = p.stack;

    // ---- the sample: nothing read from the device is trusted
    Sample sm;
    sm.e = uniform(p.episode[b]);
    sm.t = uniform(p.step[b]);
    sm.first = 0;
    sm.goal_row = 0;
    sm.pad = sm.e < 0 || sm.e >= p.E;
    if (!sm.pad) {
        sm.first = uniform64(p.first[sm.e]);
        const int len = uniform(clampi(p.length[sm.e], 0, p.L));
        sm.pad = sm.t < 1 || sm.t > len || sm.first < 0 || sm.first > p.n_records - len;
        if (p.goal) {
            sm.goal_row = p.goal_index ? uniform64(p.goal_index[b]) : sm.e;
            sm.pad = sm.pad || sm.goal_row < 0 || sm.goal_row >= p.n_goal_rows;
        }
    }
    if (sm.pad) {   // (block-uniform)
        emit_padding<kDtype>(p, b, P9);
        if (p.record && tid < kRecord) p.record[b * kRecord + tid] = 0;
        if (p.valid && tid == 0) p.valid[b] = 0;
        return;
    }
    const int t = sm.t, lo = max(0, t - K);           // the stacks hold entries lo .. t
    const uint8_t* rec_g = p.records + sm.first * kRecord;
    if (p.record && tid < kRecord) p.record[b * kRecord + tid] = rec_g[(int64_t)(t - 1) * kRecord + tid];
    if (p.valid && tid == 0) p.valid[b] = 1;

    // ---- channel -> (plane, test); the starting row, the goal row, the entries' own words
#include "../igw_voxel_table.h"
    if (tid < kChunks) {
        u32x4 v = reinterpret_cast<const u32x4*>(p.start + sm.e * kRow)[tid];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t c = (w[k] >> (8 * j)) & 0xffu;
                r |= (c <= 6u ? c : 0u) << (8 * j);
            }
            w[k] = r;
        }
        if (tid == kChunks - 1) {   // cell 1088 and fifteen pad bytes
            w[0] &= 0xffu;
            w[1] = w[2] = w[3] = 0u;
        }
        reinterpret_cast<u32x4*>(grid)[tid] = u32x4{w[0], w[1], w[2], w[3]};
    }
    if (p.goal) {
        const int8_t* g = p.goal + sm.goal_row * p.goal_stride;
        for (int c = tid; c < kCells; c += kThreads) goal_row[c] = g[c];
    }
    if (tid < IGW_RECALL_MAX_STACK)   // the word of record lo + tid makes entry lo + tid + 1
        own_word[tid] = lo + tid < t ? *reinterpret_cast<const uint16_t*>(rec_g + (int64_t)(lo + tid) * kRecord + kChangeOffset)
                                     : (uint16_t)kNone;

    // ---- entry lo: the words of records 0 .. lo - 1 in record order
#pragma unroll 1
    for (int base = 0; base < lo; base += kThreads) {
        const int j = base + tid;
        chg[tid] = j < lo ? *reinterpret_cast<const uint16_t*>(rec_g + (int64_t)j * kRecord + kChangeOffset) : (uint16_t)kNone;
        __syncthreads();
        if (wave == 0) {
            for (int sub = 0; sub < kThreads / kWave; sub++) {
                if (base + sub * kWave >= lo) break;
                const int w = chg[sub * kWave + lane];
                uint64_t mask = __ballot(w != kNone && (w & 0x7ff) < kCells);
                while (mask != 0) {                   // in record order: a cell may change more than once
                    const int bit = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int wv = __builtin_amdgcn_readlane(w, bit);
                    if (lane == 0) grid[wv & 0x7ff] = (uint8_t)((wv >> 11) & 7);
                }
            }
        }
        __syncthreads();
    }

    const Planes pl{cells, ch_plane, ch_match, P9};
#pragma unroll 1
    for (int s = lo; s <= t; s++) {
        if (s > lo && tid == 0) {
            const int w = own_word[s - lo - 1];
            if (w != kNone && (w & 0x7ff) < kCells) grid[w & 0x7ff] = (uint8_t)((w >> 11) & 7);
        }
        if (tid < 4) {     // x, y, z, yaw through LDS: what every lane derives from them then lives in vector registers
            pose_s[tid] = s == 0 ? p.init_pose[(int64_t)sm.e * 5 + tid]
                                 : (double)reinterpret_cast<const float*>(rec_g + (int64_t)(s - 1) * kRecord)[tid == 3 ? 4 : tid];
        }
        __syncthreads();   // the grid is entry s's; the previous entry's planes and pose have been read

        const Frame fr(pose_s[0], pose_s[1], pose_s[2], pose_s[3]);
#include "../igw_voxel_stage.h"
        __syncthreads();

        emit_entry<kDtype>(p, b, t, s, pl);
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_recall: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_RECALL_BUILD_ID
#define IGW_RECALL_BUILD_ID "igw-recall-build-id:unstamped"
#endif

static_assert(sizeof(igw_recall_spec) == IGW_RECALL_SPEC_BYTES, "igw_recall_spec layout");

extern "C" {

int igw_recall_version(void) { return IGW_RECALL_VERSION; }
// (the string carries a marker so that recall.py can read the id of a library file without loading it)
const char* igw_recall_build_id(void) { return &IGW_RECALL_BUILD_ID[sizeof("igw-recall-build-id:") - 1]; }
const char* igw_recall_last_error(void) { return g_err; }

int igw_recall(const void* records, int64_t n_records, const int64_t* first, const int32_t* length,
               const int8_t* start_grid, const double* init_pose, int32_t E, int32_t L, const int32_t* episode,
               const int32_t* step, int32_t B, const int8_t* goal, int64_t goal_stride, int64_t n_goal_rows,
               const int64_t* goal_index, const igw_recall_spec* spec, void* obs, void* next_obs, uint8_t* record,
               uint8_t* valid, void* stream) {
    if (!spec) return fail(IGW_RECALL_ERR_INVALID, "spec must not be NULL");
    if (!records || !first || !length || !start_grid || !init_pose)
        return fail(IGW_RECALL_ERR_INVALID, "records, first, length, start_grid and init_pose must not be NULL");
    if (!episode || !step) return fail(IGW_RECALL_ERR_INVALID, "episode and step must not be NULL");
    if (!obs && !next_obs && !record && !valid) return fail(IGW_RECALL_ERR_INVALID, "at least one output must not be NULL");
    if (B < 0 || E < 0 || n_records < 0) return fail(IGW_RECALL_ERR_INVALID, "B, E and n_records must be >= 0");
    if (L < 1) return fail(IGW_RECALL_ERR_INVALID, "L must be >= 1");
    if (spec->num_planes < 1 || spec->num_planes > IGW_RECALL_MAX_PLANES)
        return fail(IGW_RECALL_ERR_INVALID, "num_planes must be in 1..4");
    int channels = spec->agent_plane ? 1 : 0;
    bool goal_plane = false;
    for (int s = 0; s < spec->num_planes; s++) {
        const igw_recall_plane& pl = spec->planes[s];
        if (pl.source != IGW_RECALL_GRID && pl.source != IGW_RECALL_GOAL)
            return fail(IGW_RECALL_ERR_INVALID, "a plane's source must be IGW_RECALL_GRID or IGW_RECALL_GOAL");
        if (pl.encoding != IGW_RECALL_ONEHOT && pl.encoding != IGW_RECALL_OCC)
            return fail(IGW_RECALL_ERR_INVALID, "a plane's encoding must be IGW_RECALL_ONEHOT or IGW_RECALL_OCC");
        goal_plane = goal_plane || pl.source == IGW_RECALL_GOAL;
        channels += pl.encoding == IGW_RECALL_ONEHOT ? 6 : 1;
    }
    if (goal_plane && !goal) return fail(IGW_RECALL_ERR_INVALID, "a goal plane needs goal");
    if (goal && goal_stride < IGW_RECALL_CELLS) return fail(IGW_RECALL_ERR_INVALID, "goal_stride must be >= 1089");
    if (goal && n_goal_rows < 0) return fail(IGW_RECALL_ERR_INVALID, "n_goal_rows must be >= 0");
    if (spec->frame != IGW_RECALL_WORLD && spec->frame != IGW_RECALL_EGO)
        return fail(IGW_RECALL_ERR_INVALID, "frame must be IGW_RECALL_WORLD or IGW_RECALL_EGO");
    if (spec->frame == IGW_RECALL_EGO && (spec->radius < 1 || spec->radius > IGW_RECALL_MAX_RADIUS))
        return fail(IGW_RECALL_ERR_INVALID, "radius must be in 1..10");
    if (spec->dtype < IGW_RECALL_U8 || spec->dtype > IGW_RECALL_F32)
        return fail(IGW_RECALL_ERR_INVALID, "dtype must be an IGW_RECALL_U8 / F16 / BF16 / F32");
    if (spec->stack < 1 || spec->stack > IGW_RECALL_MAX_STACK) return fail(IGW_RECALL_ERR_INVALID, "stack must be in 1..8");
    if (!__builtin_isfinite(spec->scale) || !__builtin_isfinite(spec->bias))
        return fail(IGW_RECALL_ERR_INVALID, "scale and bias must be finite");
    if (spec->dtype == IGW_RECALL_U8 && (spec->scale != 1.0f || spec->bias != 0.0f))
        return fail(IGW_RECALL_ERR_INVALID, "IGW_RECALL_U8 takes scale 1 and bias 0");
    if (!aligned(start_grid, 16)) return fail(IGW_RECALL_ERR_INVALID, "start_grid must be 16-byte aligned");
    if (!aligned(first, 8) || !aligned(init_pose, 8) || !aligned(goal_index, 8) || !aligned(records, 4) ||
        !aligned(length, 4) || !aligned(episode, 4) || !aligned(step, 4))
        return fail(IGW_RECALL_ERR_INVALID, "first, init_pose and goal_index must be 8-byte, records, length, episode and step 4-byte aligned");
    const uintptr_t size = spec->dtype == IGW_RECALL_U8 ? 1 : spec->dtype == IGW_RECALL_F32 ? 4 : 2;
    if (!aligned(obs, size) || !aligned(next_obs, size))
        return fail(IGW_RECALL_ERR_INVALID, "obs and next_obs must be aligned to their element size");
    const int64_t blocks = B;   // one workgroup per sample
    if (blocks > 0x7fffffffll) return fail(IGW_RECALL_ERR_INVALID, "B must be below 2^31");
    if (B == 0) return IGW_RECALL_OK;
    RecallParams p;
    p.records = static_cast<const uint8_t*>(records); p.first = first; p.length = length; p.start = start_grid;
    p.init_pose = init_pose; p.episode = episode; p.step = step; p.goal = goal; p.goal_index = goal ? goal_index : nullptr;
    p.obs = obs; p.next_obs = next_obs; p.record = record; p.valid = valid;
    p.n_records = n_records; p.goal_stride = goal_stride; p.n_goal_rows = n_goal_rows;
    p.scale = spec->scale; p.bias = spec->bias;
    p.E = E; p.L = L;
    p.planes = 0;
    for (int s = 0; s < spec->num_planes; s++)
        p.planes |= ((uint32_t)spec->planes[s].source | (uint32_t)spec->planes[s].encoding << 1) << (2 * s);
    p.nplanes = spec->num_planes;
    p.agent_plane = spec->agent_plane ? 1 : 0;
    p.ego = spec->frame == IGW_RECALL_EGO;
    p.R = p.ego ? spec->radius : 5;
    p.dtype = spec->dtype;
    p.stack = spec->stack;
    p.channels = channels;
    const dim3 grid((unsigned)blocks), block(kThreads);
    switch (p.dtype) {
        case IGW_RECALL_U8: hipLaunchKernelGGL(igw_recall_kernel<IGW_RECALL_U8>, grid, block, 0, (hipStream_t)stream, p); break;
        case IGW_RECALL_F16: hipLaunchKernelGGL(igw_recall_kernel<IGW_RECALL_F16>, grid, block, 0, (hipStream_t)stream, p); break;
        case IGW_RECALL_BF16: hipLaunchKernelGGL(igw_recall_kernel<IGW_RECALL_BF16>, grid, block, 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(igw_recall_kernel<IGW_RECALL_F32>, grid, block, 0, (hipStream_t)stream, p); break;
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(IGW_RECALL_ERR_HIP, "launch failed: ", hipGetErrorString(err));
    return IGW_RECALL_OK;
}

}  // extern "C"
