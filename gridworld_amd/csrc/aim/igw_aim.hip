// igw_aim.hip -- libigw_aim.so: igw_aim (include/igw_aim.h), which grid cells a place or a break can reach from each
// env's live state by turning the camera alone, and the cheapest turn that gets there, in one launch.
//
// One workgroup of 256 lanes owns an env.  It stages the env's 192-byte occupancy row in LDS behind the constant prefix
// and suffix hit_test expects, evaluates the step's own trig (sincos_deg<true> over the same table, -ffp-contract=off)
// ONCE per lattice angle -- at most 72 yaw and 73 pitch values, one lane each -- and lists the directions of the window
// row by row: a row is one dj, its slots the di of the diamond |di| + |dj| <= max_turns, rows whose pitch does not exist
// are empty.  Slot s of that list goes to lane s % 256 of round s / 256, so the 64 rays of a wavefront are neighbours in
// di at one or two dj: they stop at similar samples, and hit_test<1> of igw_device.h (compiled here unchanged) leaves
// its loop when every lane of the wavefront has its answer.  A small max_turns walks only its diamond.  Every lane folds
// its ray's two cells into the two 1104-word planes in LDS with an unsigned atomic minimum of the direction's code; the
// planes start as all ones (= -1, which the 15 pad words keep), and the block stores each as 276 dwordx4.
#include <stdio.h>

#include "../igw_device.h"
#include "../../../include/igw_aim.h"

namespace {

using namespace igw;

constexpr int kRow = IGW_AIM_ROW;
constexpr int kHalf = 36;                  // di = -36..35, dj = -36..36
constexpr int kYaw = 2 * kHalf;            // 72 yaw angles
constexpr int kPitch = 2 * kHalf + 1;      // 73 pitch angles
static_assert(kRow % 4 == 0 && kRow >= IGW_AIM_CELLS && IGW_AIM_CELLS == CELLS, "a plane is whole dwordx4 and holds every cell");
static_assert(kYaw + kPitch <= BLOCK && OCC_PITCH <= BLOCK, "one lane per lattice angle, one per occupancy word");
static_assert(IGW_AIM_MAX_TURNS == 2 * kHalf, "the window is 36 turns either way in yaw and in pitch");

struct Shared {
    alignas(16) uint32_t occ[OCC_PITCH];
    alignas(16) uint32_t plane[2][kRow];   // [0] place, [1] break: the smallest code per cell
    double sc[kYaw + kPitch][2];           // (sin, cos) of yaw_d - 90 for di = -36..35, then of pitch_d for dj = -36..36
    int start[kPitch + 1];                 // first slot of each listed row; [rows] = the number of slots
};

// the slots of row dj: the di of the diamond, clipped to -36..35; none where the pitch does not exist
__device__ inline int row_first(int rem) { return max(-kHalf, -rem); }
__device__ inline int row_width(double pitch, int dj, int max_turns) {
    const double pd = pitch + 5.0 * (double)dj;
    if (!((pd >= -90.0) & (pd <= 90.0))) return 0;
    const int rem = max_turns - abs(dj);
    return min(kHalf - 1, rem) - row_first(rem) + 1;
}

__global__ __launch_bounds__(BLOCK) void igw_aim_kernel(const AgentRec* __restrict__ agent, const uint32_t* __restrict__ occ,
                                                        int32_t* __restrict__ place, int32_t* __restrict__ brk,
                                                        int32_t max_turns) {
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x;
    const int64_t env = (int64_t)blockIdx.x;
    const AgentRec r = agent[env];   // every lane the same 64 bytes

    // ---- the occupancy row: words 0..15 and 64..71 constant (occ_const_word), 16..63 the env's
    if (tid < OCC_PITCH) {
        const bool var = (tid >= OCC_VAR0) & (tid < OCC_VAR0 + OCC_WORDS);
        sh.occ[tid] = var ? occ[env * OCC_WORDS + (tid - OCC_VAR0)] : occ_const_word(tid);
    }
    for (int i = tid; i < 2 * kRow; i += BLOCK) (&sh.plane[0][0])[i] = 0xffffffffu;

    // ---- the lattice angles the window uses, one lane each (get_sight_vector, core/world.py:312-318: the yaw enters as
    // yaw - 90)
    if (tid < kYaw + kPitch) {
        const bool is_yaw = tid < kYaw;
        const int d = (is_yaw ? tid : tid - kYaw) - kHalf;
        if (abs(d) <= max_turns) {
            TrigCtx trig;
            // sincos_deg<true> reads lut[2 * k] = cos and lut[2 * k + 1] = sin of entry k < IGW_LUT_N: the host table's layout
            static_assert(sizeof(IGW_TRIG_LUT_HOST) == sizeof(double) * 2 * IGW_LUT_N, "the trig table is IGW_LUT_N (cos, sin) pairs of doubles");
            trig.lut = &IGW_TRIG_LUT_HOST[0][0];   // a const table with a constant initialiser: constant memory of this code object
            const double turned = (is_yaw ? r.yaw : r.pitch) + 5.0 * (double)d;
            double s, c;
            sincos_deg<true>(trig, is_yaw ? turned - 90.0 : turned, s, c);
            sh.sc[tid][0] = s;
            sh.sc[tid][1] = c;
        }
    }

    // ---- the list of directions: rows dj = -span..span, lane t sums the widths of the rows in front of row t
    const int span = min(max_turns, kHalf), rows = 2 * span + 1;
    if (tid <= rows) {
        int first = 0;
        for (int j = 0; j < tid; j++) first += row_width(r.pitch, j - span, max_turns);
        sh.start[tid] = first;
    }
    __syncthreads();
    const int total = sh.start[rows];

    const Grp<1> G;
    const double x = r.x, z = r.z;
    const double y = r.y - 1.0 + PAD;   // y - (PLAYER_HEIGHT - 1) + Agent.PAD
    for (int base = 0; base < total; base += BLOCK) {
        const int s = base + tid;
        if (s < total) {
            // the last row that starts at or before slot s (an empty row shares its start with the next one)
            int row = 0;
#pragma unroll
            for (int bit = 64; bit > 0; bit >>= 1) {
                const int probe = row + bit;
                if (probe < rows && sh.start[probe] <= s) row = probe;
            }
            const int dj = row - span;
            const int di = row_first(max_turns - abs(dj)) + (s - sh.start[row]);
            const double sy = sh.sc[di + kHalf][0], cy = sh.sc[di + kHalf][1];
            const double sp = sh.sc[kYaw + dj + kHalf][0], cp = sh.sc[kYaw + dj + kHalf][1];
            const double vx = cy * cp, vy = sp, vz = sy * cp;
            const Hit h = hit_test<1>(G, sh.occ, r.x, r.y, r.z, vx, vy, vz);

            // the predicates of place_or_remove_block (world_act_post), at the current position
            const double bx = (double)h.px - 0.5, by = (double)h.py, bz = (double)h.pz - 0.5;
            const bool overlap = (bx <= x) & (x <= bx + 1.0) & (bz <= z) & (z <= bz + 1.0) &
                                 (((by <= y) & (y <= by + 1.0)) | ((by <= (y + 1.0)) & ((y + 1.0) <= by + 1.0)));
            const bool free_cell = h.hit & h.have_prev & build_zone_i(h.px, h.py, h.pz) & !overlap;
            // (a block that is not the ground stands in the build zone; the test keeps the index inside the plane)
            const bool hit_block = h.hit & (h.by != -2) & build_zone_i(h.bx, h.by, h.bz);
            const uint32_t code = (uint32_t)(abs(di) + abs(dj)) << 16 | (uint32_t)(dj + kHalf) << 8 | (uint32_t)(di + kHalf);
            if (free_cell) atomicMin(&sh.plane[0][cell_of(h.px, h.py, h.pz)], code);
            if (hit_block) atomicMin(&sh.plane[1][cell_of(h.bx, h.by, h.bz)], code);
        }
    }
    __syncthreads();

    // ---- the two rows, 4,416 bytes each, as whole dwordx4
#pragma unroll
    for (int p = 0; p < 2; p++) {
        int32_t* const out = p == 0 ? place : brk;
        if (!out) continue;
        vu4* const dst = reinterpret_cast<vu4*>(out + env * kRow);
        const uint4* const src = reinterpret_cast<const uint4*>(sh.plane[p]);
        for (int i = tid; i < kRow / 4; i += BLOCK) {
            const uint4 v = src[i];
            gstore(dst + i, vu4{v.x, v.y, v.z, v.w});
        }
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_aim: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_AIM_BUILD_ID
#define IGW_AIM_BUILD_ID "igw-aim-build-id:unstamped"
#endif

extern "C" {

int igw_aim_version(void) { return IGW_AIM_VERSION; }
// (the string carries a marker so that aim.py can read the id of a library file without loading it)
const char* igw_aim_build_id(void) { return &IGW_AIM_BUILD_ID[sizeof("igw-aim-build-id:") - 1]; }
const char* igw_aim_last_error(void) { return g_err; }

int igw_aim(const void* agent, const uint32_t* occ, int32_t n, int32_t max_turns, int32_t* place, int32_t* brk,
            void* stream) {
    if (!agent || !occ) return fail(IGW_AIM_ERR_INVALID, "agent and occ must not be NULL");
    if (!place && !brk) return fail(IGW_AIM_ERR_INVALID, "place and brk must not both be NULL");
    if (n < 0) return fail(IGW_AIM_ERR_INVALID, "n must be >= 0");
    if (max_turns < 0 || max_turns > IGW_AIM_MAX_TURNS) return fail(IGW_AIM_ERR_INVALID, "max_turns must be 0..72");
    if (!aligned(agent, 16) || !aligned(occ, 16) || !aligned(place, 16) || !aligned(brk, 16))
        return fail(IGW_AIM_ERR_INVALID, "agent, occ, place and brk must be 16-byte aligned");
    if (n == 0) return IGW_AIM_OK;
    hipLaunchKernelGGL(igw_aim_kernel, dim3((unsigned)n), dim3(BLOCK), 0, (hipStream_t)stream,
                       static_cast<const AgentRec*>(agent), occ, place, brk, max_turns);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_AIM_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_AIM_OK;
}

}  // extern "C"
