// igw_query.hip -- libigw_query.so: igw_action_mask (include/igw_query.h), which of the 18 walking actions would act on
// each env's live state, in one launch.
//
// The layout is the step kernel's at four lanes per env: a quad owns an env, a wavefront sixteen, a block sixty-four.
// The quad stages the env's 192-byte occupancy row in LDS behind the constant prefix hit_test expects, builds the sight
// vector with the step's own trig (sincos_deg<true> over the same table, -ffp-contract=off) and marches the ray ONCE with
// hit_test<4> of igw_device.h, compiled here unchanged: no Discrete(18) action turns the camera and places or breaks, so
// this is the ray the next step marches whichever of the eight place / break actions it is given.  What is left are
// seven inventory tests, the overlap / build-zone predicate of place_or_remove_block and three scalar tests on the
// agent record.  The 18 bytes of an env are assembled in LDS and a full wavefront stores its 288 bytes as 72 dwords.
// Nothing synchronises across wavefronts: a wavefront that has no env returns at once.
#include <stdio.h>

#include "../igw_device.h"
#include "../../../include/igw_query.h"

namespace {

using namespace igw;

constexpr int kActions = IGW_QUERY_ACTIONS;
constexpr int kEnvsPerWave = WAVE / 4;
constexpr int kMaskWords = kEnvsPerWave * kActions / 4;   // 72 dwords = 288 B of mask per wavefront
constexpr int kMarchWords = WAVE * 10;                    // hit_test<4>'s scratch: ten rounds of one key per lane
static_assert(kEnvsPerWave * kActions % 4 == 0 && kActions % 2 == 0, "a wavefront's mask is whole dwords, an env's whole shorts");

struct WaveShared {
    alignas(16) uint32_t occ[kEnvsPerWave * OCC_PITCH];
    uint32_t march[kMarchWords];
    alignas(4) uint16_t mask[kEnvsPerWave * kActions / 2];
};

// the k-th set bit of m (k < popcount(m), m < 2^18)
__device__ inline int nth_set_bit(uint32_t m, int k) {
#pragma unroll
    for (int j = 0; j < kActions - 1; j++) m = j < k ? m & (m - 1) : m;
    return __builtin_ctz(m);
}

__global__ __launch_bounds__(BLOCK) void igw_action_mask_kernel(const AgentRec* __restrict__ agent,
                                                                const uint32_t* __restrict__ occ, uint8_t* __restrict__ mask,
                                                                int16_t* __restrict__ look, int32_t* __restrict__ actions,
                                                                int32_t n, int32_t select_and_place, uint64_t seed, uint64_t t,
                                                                int64_t env_offset) {
    __shared__ WaveShared sh[WAVES_PER_BLOCK];
    const Grp<4> G;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
    const int64_t env0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + wave) * kEnvsPerWave;   // the wavefront's first env
    if (env0 >= n) return;
    WaveShared& ws = sh[wave];
    const int valid = (int)min((int64_t)kEnvsPerWave, (int64_t)n - env0);
    const bool live = G.g < valid;
    const int64_t env = env0 + (live ? G.g : 0);   // a quad without an env redoes the wavefront's first and stores nothing

    // ---- loads: the agent record (every lane of the quad the same 64 bytes) and the quad's share of the occupancy row
    const AgentRec r = agent[env];
    const uint4* row_g = reinterpret_cast<const uint4*>(occ + env * OCC_WORDS);
    uint32_t* occ_s = ws.occ + G.g * OCC_PITCH;
    uint4 v[3];
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = row_g[G.gl + 4 * i];
    {
        // the constant words (occ_const_word): words 0..9 zero, word 10 the first bits of the ground plane, 11..15 ones,
        // 64..71 zero; lane q of the quad writes the 16-byte piece q of the prefix and, q < 2, of the suffix
        static_assert(occ_const_word(0) == 0u && occ_const_word(9) == 0u && occ_const_word(11) == 0xffffffffu &&
                      occ_const_word(15) == 0xffffffffu && occ_const_word(OCC_VAR0 + OCC_WORDS) == 0u, "constant words of the LDS occupancy row");
        static_assert(OCC_VAR0 == 16 && OCC_WORDS == 48 && OCC_PITCH == 72, "the row is staged as 4 + 12 + 2 pieces of 16 bytes");
        const int q = G.gl;
        const uint32_t is3 = 0u - (uint32_t)(q == 3), ge2 = 0u - (uint32_t)(q >= 2);
        *reinterpret_cast<uint4*>(occ_s + 4 * q) = make_uint4(is3, is3, is3 | (ge2 & occ_const_word(10)), ge2);
        if (q < 2) *reinterpret_cast<uint4*>(occ_s + OCC_VAR0 + OCC_WORDS + 4 * q) = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) *reinterpret_cast<uint4*>(occ_s + OCC_VAR0 + 4 * (G.gl + 4 * i)) = v[i];

    // ---- the sight vector (get_sight_vector, core/world.py:312-318) as world_act_pre builds it: lane 0 of the quad
    // evaluates the pitch, lane 1 yaw - 90, the pairs are exchanged
    TrigCtx trig;
    // sincos_deg<true> reads lut[2 * k] = cos and lut[2 * k + 1] = sin of entry k < IGW_LUT_N: the host table's layout
    static_assert(sizeof(IGW_TRIG_LUT_HOST) == sizeof(double) * 2 * IGW_LUT_N, "the trig table is IGW_LUT_N (cos, sin) pairs of doubles");
    trig.lut = &IGW_TRIG_LUT_HOST[0][0];   // a const table with a constant initialiser: constant memory of this code object
    double sv, cv;
    sincos_deg<true>(trig, G.gl == 1 ? r.yaw - 90.0 : r.pitch, sv, cv);
    const double sp = dpp_quad<QUAD_BCAST0>(sv), cp = dpp_quad<QUAD_BCAST0>(cv);
    const double sy = dpp_quad<QUAD_BCAST1>(sv), cy = dpp_quad<QUAD_BCAST1>(cv);
    const double vx = cy * cp, vy = sp, vz = sy * cp;
    wave_sync();   // the rows are written by the lanes that read them, of this wavefront
    const Hit h = hit_test<4>(G, occ_s, r.x, r.y, r.z, vx, vy, vz, false, ws.march);

    // ---- the predicates of place_or_remove_block (world_act_post), at the current position
    const double x = r.x, z = r.z;
    const double y = r.y - 1.0 + PAD;   // y - (PLAYER_HEIGHT - 1) + Agent.PAD
    const double bx = (double)h.px - 0.5, by = (double)h.py, bz = (double)h.pz - 0.5;
    const bool overlap = (bx <= x) & (x <= bx + 1.0) & (bz <= z) & (z <= bz + 1.0) &
                         (((by <= y) & (y <= by + 1.0)) | ((by <= (y + 1.0)) & ((y + 1.0) <= by + 1.0)));
    const bool free_cell = h.hit & h.have_prev & build_zone_i(h.px, h.py, h.pz) & !overlap;
    const bool brk = h.hit & (h.by != -2);
    uint32_t iw[4];
    __builtin_memcpy(iw, &r.inv[0], 16);
    const int active = (int)((iw[3] >> 18) & 7u);
    uint32_t have = 0;   // bit k: inventory[k] > 0
#pragma unroll
    for (int k = 0; k < 6; k++) have |= (uint32_t)(inv_pick(iw[0], iw[1], iw[2], k) > 0) << k;
    const uint32_t act_bit = (unsigned)(active - 1) < 6u ? 1u << (active - 1) : 0u;
    const bool place = free_cell & ((have & act_bit) != 0);
    const uint32_t hotbar = select_and_place ? (free_cell ? have : 0u) : (0x3fu & ~act_bit);
    const uint32_t bits = 0x301fu                                 // no-op, the four moves, the two yaw actions
                          | (uint32_t)(r.vy == 0.0) << 5          // jump: movement, core/world.py:344-356
                          | hotbar << 6
                          | (uint32_t)(r.pitch > -90.0) << 14 | (uint32_t)(r.pitch < 90.0) << 15   // move_camera's clamp
                          | (uint32_t)brk << 16 | (uint32_t)place << 17;

    if (look && live && G.gl < 2) {
        const int cell = G.gl == 0 ? (brk ? cell_of(h.bx, h.by, h.bz) : -1) : (place ? cell_of(h.px, h.py, h.pz) : -1);
        gstore(look + 2 * env + G.gl, (int16_t)cell);
    }
    if (actions && live && G.gl == 0) {
        const uint64_t e = (uint64_t)(env_offset + env);
        const uint64_t hsh = splitmix64(seed ^ splitmix64(e * 0x9E3779B1ull + t * 0x100000001B3ull + 0x6d61736bull));
        gstore(actions + env, nth_set_bit(bits, rng_below((uint32_t)(hsh >> 32), __builtin_popcount(bits))));
    }

    // ---- the mask: an env's 18 bytes as nine shorts in LDS (lane q of the quad writes shorts q, q + 4, q + 8), then the
    // wavefront's 288 bytes as dwords; byte by byte where the wavefront is not full or `mask` is not dword-aligned
#pragma unroll
    for (int s = G.gl; s < kActions / 2; s += 4)
        ws.mask[G.g * (kActions / 2) + s] = (uint16_t)(((bits >> (2 * s)) & 1u) | (((bits >> (2 * s + 1)) & 1u) << 8));
    wave_sync();
    uint8_t* dst = mask + env0 * kActions;
    if (valid == kEnvsPerWave && (reinterpret_cast<uintptr_t>(mask) & 3) == 0) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(ws.mask);
        gstore(reinterpret_cast<uint32_t*>(dst) + G.lane, src[G.lane]);
        if (G.lane < kMaskWords - WAVE) gstore(reinterpret_cast<uint32_t*>(dst) + WAVE + G.lane, src[WAVE + G.lane]);
    } else {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(ws.mask);
        for (int b = G.lane; b < valid * kActions; b += WAVE) gstore(dst + b, src[b]);
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_action_mask: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_QUERY_BUILD_ID
#define IGW_QUERY_BUILD_ID "igw-query-build-id:unstamped"
#endif

extern "C" {

int igw_query_version(void) { return IGW_QUERY_VERSION; }
// (the string carries a marker so that query.py can read the id of a library file without loading it)
const char* igw_query_build_id(void) { return &IGW_QUERY_BUILD_ID[sizeof("igw-query-build-id:") - 1]; }
const char* igw_query_last_error(void) { return g_err; }

int igw_action_mask(const void* agent, const uint32_t* occ, int32_t n, int32_t select_and_place, uint8_t* mask,
                    int16_t* look, int32_t* actions, uint64_t seed, uint64_t t, int64_t env_offset, void* stream) {
    if (!agent || !occ || !mask) return fail(IGW_QUERY_ERR_INVALID, "agent, occ and mask must not be NULL");
    if (n < 0) return fail(IGW_QUERY_ERR_INVALID, "n must be >= 0");
    if (!aligned(agent, 16) || !aligned(occ, 16) || !aligned(look, 2) || !aligned(actions, 4))
        return fail(IGW_QUERY_ERR_INVALID, "agent and occ must be 16-byte, look 2-byte, actions 4-byte aligned");
    if (n == 0) return IGW_QUERY_OK;
    const int64_t waves = ((int64_t)n + kEnvsPerWave - 1) / kEnvsPerWave;
    const unsigned blocks = (unsigned)((waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
    hipLaunchKernelGGL(igw_action_mask_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                       static_cast<const AgentRec*>(agent), occ, mask, look, actions, n, select_and_place, seed, t, env_offset);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_QUERY_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_QUERY_OK;
}

}  // extern "C"
