// igw_vox.hip -- libigw_vox.so: igw_vox_obs (include/igw_vox.h), the state as the tensor a policy network reads:
// channel-first one-hot / occupancy planes of up to four grids and the agent's body, in the world's or the agent's
// frame, in u8 / f16 / bf16 / f32, stacked over the last K calls -- one launch, a pure streaming writer.
//
// One workgroup of 256 lanes per env.
//   stage   Pose, head cell, heading quadrant and window are computed by every lane from the env's agent record (the
//           same values in all of them: no exchange).  Each lane then walks output cells o = (y, u, w) of the S x S
//           window, maps them to the world cell they show and leaves one byte per source in LDS, ALREADY in the output
//           frame: for a one-hot source 0 (empty, or outside the grid), 1..6 (the colour), 7 (any other non-zero sum), for
//           an occupancy source [v != 0]; the agent's body is a plane of the second kind.  A small table says which
//           plane a channel reads and which code it compares with, so every element is one byte load and one compare.
//   write   An env's run of stack * C * 9 * S * S elements starts wherever the runs before it end, so neither the run
//           nor its slots are 16-byte aligned in general.  Every slot is cut at the ABSOLUTE 16-byte boundaries: a lane
//           assembles a whole 16-byte piece (16 u8, 8 half, 4 f32 elements) from the LDS planes and stores it with one
//           16-byte store, so a wave instruction writes 1 KiB of contiguous lines; the up to 15 bytes in front of the
//           first boundary and behind the last go element by element.
//   shift   Slot k takes slot k + 1 piece by piece: the destination pieces are the aligned ones, the source is read at
//           whatever alignment it has (a 16-byte load at element alignment).  Pieces of two slots do not coincide, so a
//           barrier separates slot k's copy from the write of slot k + 1: everything read from a slot has arrived
//           (the stores before the barrier consumed it) before any lane writes that slot.
// Loop bounds depend on the spec only; nothing is allocated, nothing synchronises across workgroups.
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "../../../include/igw_vox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLevels = IGW_VOX_LEVELS;
constexpr int kMaxSide = 2 * IGW_VOX_MAX_RADIUS + 1;
constexpr int kMaxPlane = kLevels * kMaxSide * kMaxSide;      // cells of the largest window: 3,969
constexpr int kPlanes = IGW_VOX_MAX_SOURCES + 1;               // the sources' and the agent's
constexpr int kTable = 32;                                     // >= 4 * 6 + 1 channels, and one behind the last
constexpr int kOther = 7;                                      // a non-zero value outside 1..6

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct VoxParams {
    igw_vox_source src[IGW_VOX_MAX_SOURCES];
    const uint8_t* agent;
    const uint8_t* aux;
    void* data;
    const uint8_t* restart;
    int64_t restart_stride;
    float scale, bias;
    int nsrc, agent_plane, ego, R, dtype, stack, fill, channels;
};

template <int kDtype> struct Elem { using E = uint16_t; };
template <> struct Elem<IGW_VOX_U8> { using E = uint8_t; };
template <> struct Elem<IGW_VOX_F32> { using E = uint32_t; };

// b = 0 / 1 as the bits of an element: u8 as it is; the float types from (float)b * scale, then + bias (two roundings:
// the library is built with -ffp-contract=off), f16 / bf16 rounded to nearest-even from that f32.
template <int kDtype>
__device__ __forceinline__ typename Elem<kDtype>::E value(uint32_t b, float scale, float bias) {
    if constexpr (kDtype == IGW_VOX_U8) {
        return (uint8_t)b;
    } else {
        float f = (float)b * scale;
        f = f + bias;
        const uint32_t u = __float_as_uint(f);
        if constexpr (kDtype == IGW_VOX_F32) {
            return u;
        } else if constexpr (kDtype == IGW_VOX_F16) {
            const _Float16 h = (_Float16)f;
            return __builtin_bit_cast(uint16_t, h);
        } else {   // (scale and bias are finite, so f is no NaN unless inf - inf: kept a quiet NaN)
            if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
            return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    }
}

// Which 16-byte stores are non-temporal: 1 = those of the new planes (the default: what won the A/B of
// profiles/LAB_NOTEBOOK.md), 0 = none, 2 = those of the shift too (the A/B's other arms).
#ifndef IGW_VOX_NT_STORES
#define IGW_VOX_NT_STORES 1
#endif

template <bool kNew>
__device__ __forceinline__ void store16(void* p, u32x4 v) {
    if constexpr (IGW_VOX_NT_STORES >= (kNew ? 1 : 2)) {
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    } else {
        *reinterpret_cast<u32x4*>(p) = v;
    }
}

// rint(v) as an int, clamped to +-64: a centre that far out sees only cells outside the grid, as any farther one does
__device__ __forceinline__ int cell_of(double v) {
    const double r = __builtin_rint(v);
    return (int)__builtin_fmin(__builtin_fmax(r, -64.0), 64.0);
}

// How a slot of L elements at `base` is cut at the absolute 16-byte boundaries: `head` elements in front of the first,
// `pieces` whole 16-byte pieces, and the rest from `tail` on.
template <typename E> struct Cut {
    int head, pieces, tail;
    __device__ __forceinline__ Cut(const E* base, int L) {
        constexpr int P = 16 / (int)sizeof(E);
        const unsigned lead = (16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u;
        head = min(L, (int)(lead / sizeof(E)));
        pieces = (L - head) / P;
        tail = head + pieces * P;
    }
};

struct Planes {
    const uint8_t* cells;      // [kPlanes][kMaxPlane] bytes in LDS
    const uint8_t* ch_plane;   // [kTable]
    const uint8_t* ch_match;   // [kTable]: the channel is [code == it]
    int P9;                    // cells of one channel: 9 * S * S
};

// The new planes into one slot.
template <int kDtype>
__device__ __forceinline__ void write_new(typename Elem<kDtype>::E* base, int L, const Planes& pl,
                                          typename Elem<kDtype>::E v0, typename Elem<kDtype>::E v1) {
    using E = typename Elem<kDtype>::E;
    constexpr int P = 16 / (int)sizeof(E);
    const int tid = threadIdx.x;
    const Cut<E> cut(base, L);
    const int rounds = (L / P + kThreads) / kThreads;   // >= pieces / kThreads, from the spec alone
#pragma unroll 1
    for (int it = 0; it < rounds; it++) {
        const int p = tid + it * kThreads;
        if (p >= cut.pieces) continue;
        const int e0 = cut.head + p * P;
        const int ch = e0 / pl.P9, o = e0 - ch * pl.P9;
        // A piece lies in one channel or straddles two (a channel has an odd number of cells): its first `own`
        // elements are channel ch's from cell o on, the others channel ch + 1's from cell 0 on (behind the last
        // channel the table still answers, and no piece reaches there).  No branch, no carried cell counter.
        const int own = pl.P9 - o;
        const int at1 = (int)pl.ch_plane[ch] * kMaxPlane + o, at2 = (int)pl.ch_plane[ch + 1] * kMaxPlane - own;
        const uint32_t m1 = pl.ch_match[ch], m2 = pl.ch_match[ch + 1];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < P; j++) {
            const bool next = j >= own;
            const uint32_t code = pl.cells[(next ? at2 : at1) + j];
            const uint32_t e = code == (next ? m2 : m1) ? v1 : v0;
            w[j * (int)sizeof(E) / 4] |= e << (8 * ((j * (int)sizeof(E)) & 3));
        }
        store16<true>(base + e0, u32x4{w[0], w[1], w[2], w[3]});
    }
    const int edge = cut.head + (L - cut.tail);   // < 2 * P
    if (tid < edge) {
        const int e = tid < cut.head ? tid : cut.tail + (tid - cut.head);
        const int ch = e / pl.P9, o = e - ch * pl.P9;
        base[e] = pl.cells[(int)pl.ch_plane[ch] * kMaxPlane + o] == pl.ch_match[ch] ? v1 : v0;
    }
}

// Slot k takes slot k + 1 (L elements further on).
template <typename E>
__device__ __forceinline__ void shift_down(E* dst, int L) {
    constexpr int P = 16 / (int)sizeof(E);
    const int tid = threadIdx.x;
    const E* src = dst + L;
    const Cut<E> cut(dst, L);
    const int rounds = (L / P + kThreads) / kThreads;
#pragma unroll 1
    for (int it = 0; it < rounds; it++) {
        const int p = tid + it * kThreads;
        if (p >= cut.pieces) continue;
        const int e0 = cut.head + p * P;
        u32x4 v;
        __builtin_memcpy(&v, src + e0, 16);   // (aligned to the element only)
        store16<false>(dst + e0, v);
    }
    const int edge = cut.head + (L - cut.tail);
    if (tid < edge) {
        const int e = tid < cut.head ? tid : cut.tail + (tid - cut.head);
        dst[e] = src[e];
    }
}

template <int kDtype>
__device__ __forceinline__ void emit(const VoxParams& p, int64_t env, const Planes& pl) {
    using E = typename Elem<kDtype>::E;
    const E v0 = value<kDtype>(0u, p.scale, p.bias), v1 = value<kDtype>(1u, p.scale, p.bias);
    const int K = p.stack, L = p.channels * pl.P9;
    E* run = static_cast<E*>(p.data) + env * K * (int64_t)L;
    const bool all = p.fill != 0 || (p.restart != nullptr && p.restart[env * p.restart_stride] != 0);
    if (all) {
        for (int k = 0; k < K; k++) write_new<kDtype>(run + (int64_t)k * L, L, pl, v0, v1);
    } else {
        for (int k = 0; k + 1 < K; k++) {
            shift_down<E>(run + (int64_t)k * L, L);
            __syncthreads();
        }
        write_new<kDtype>(run + (int64_t)(K - 1) * L, L, pl, v0, v1);
    }
}

__global__ __launch_bounds__(kThreads) void igw_vox_kernel(const VoxParams p) {
    __shared__ uint8_t cells[kPlanes * kMaxPlane];
    __shared__ uint8_t ch_plane[kTable], ch_match[kTable];
    const int tid = threadIdx.x;
    const int64_t env = blockIdx.x;
    const int R = p.R, S = p.ego ? 2 * R + 1 : 11, SS = S * S, P9 = kLevels * SS;

    const double* pose = reinterpret_cast<const double*>(p.agent + env * 64);
    const int hx = cell_of(pose[0]) + 5, hy = cell_of(pose[1]) + 1, hz = cell_of(pose[2]) + 5;
    const double f = __builtin_floor((pose[3] + 45.0) / 90.0);
    const int q = (int)(f - 4.0 * __builtin_floor(f / 4.0)) & 3;
    const int fx = (q == 1) - (q == 3), fz = (q == 2) - (q == 0), rx = (q == 0) - (q == 2), rz = (q == 1) - (q == 3);
    const int64_t task = *reinterpret_cast<const int32_t*>(p.aux + env * 16 + 8);

    if (tid < kTable) {   // channel -> (plane, test)
        int plane = 0, match = 0, first = 0;
#pragma unroll
        for (int s = 0; s < IGW_VOX_MAX_SOURCES; s++) {
            if (s < p.nsrc) {
                const int count = p.src[s].encoding == IGW_VOX_ONEHOT ? 6 : 1;
                if (tid >= first && tid < first + count) {
                    plane = s;
                    match = p.src[s].encoding == IGW_VOX_ONEHOT ? tid - first + 1 : 1;
                }
                first += count;
            }
        }
        if (p.agent_plane && tid == first) {
            plane = p.nsrc;
            match = 1;
        }
        ch_plane[tid] = (uint8_t)plane;
        ch_match[tid] = (uint8_t)match;
    }
#pragma unroll 1
    for (int o = tid; o < P9; o += kThreads) {
        const int y = o / SS, rem = o - y * SS, u = rem / S, w = rem - u * S;
        int x = u, z = w;
        if (p.ego) {
            const int s = R - u, t = w - R;
            x = hx + s * fx + t * rx;
            z = hz + s * fz + t * rz;
        }
        const bool inside = (unsigned)x < 11u && (unsigned)z < 11u;
        const int c = y * 121 + x * 11 + z;
#pragma unroll
        for (int s = 0; s < IGW_VOX_MAX_SOURCES; s++) {
            if (s < p.nsrc) {
                int code = 0;
                if (inside) {
                    const int64_t at = (p.src[s].by_task ? task : env) * p.src[s].row_stride + c;
                    int v = p.src[s].rows[at];
                    if (p.src[s].add) v += p.src[s].add[at];
                    code = p.src[s].encoding == IGW_VOX_OCC ? v != 0 : v >= 1 && v <= 6 ? v : v != 0 ? kOther : 0;
                }
                cells[s * kMaxPlane + o] = (uint8_t)code;
            }
        }
        if (p.agent_plane) cells[p.nsrc * kMaxPlane + o] = (uint8_t)(inside && x == hx && z == hz && (y == hy || y == hy - 1));
    }
    __syncthreads();

    const Planes pl{cells, ch_plane, ch_match, P9};
    switch (p.dtype) {   // block-uniform
        case IGW_VOX_U8: emit<IGW_VOX_U8>(p, env, pl); break;
        case IGW_VOX_F16: emit<IGW_VOX_F16>(p, env, pl); break;
        case IGW_VOX_BF16: emit<IGW_VOX_BF16>(p, env, pl); break;
        default: emit<IGW_VOX_F32>(p, env, pl); break;
    }
}

thread_local char g_err[256] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_vox_obs: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#ifndef IGW_VOX_BUILD_ID
#define IGW_VOX_BUILD_ID "igw-vox-build-id:unstamped"
#endif

static_assert(sizeof(igw_vox_spec) == IGW_VOX_SPEC_BYTES, "igw_vox_spec layout");

extern "C" {

int igw_vox_version(void) { return IGW_VOX_VERSION; }
// (the string carries a marker so that vox.py can read the id of a library file without loading it)
const char* igw_vox_build_id(void) { return &IGW_VOX_BUILD_ID[sizeof("igw-vox-build-id:") - 1]; }
const char* igw_vox_last_error(void) { return g_err; }

int igw_vox_obs(const void* agent, const void* aux, int32_t n, const igw_vox_spec* spec, void* stream) {
    if (!spec) return fail(IGW_VOX_ERR_INVALID, "spec must not be NULL");
    if (!agent || !aux) return fail(IGW_VOX_ERR_INVALID, "agent and aux must not be NULL");
    if (n < 0) return fail(IGW_VOX_ERR_INVALID, "n must be >= 0");
    if (!aligned(agent, 8) || !aligned(aux, 4)) return fail(IGW_VOX_ERR_INVALID, "agent must be 8-byte, aux 4-byte aligned");
    if (spec->num_sources < 1 || spec->num_sources > IGW_VOX_MAX_SOURCES)
        return fail(IGW_VOX_ERR_INVALID, "num_sources must be in 1..4");
    int channels = spec->agent_plane ? 1 : 0;
    for (int s = 0; s < spec->num_sources; s++) {
        const igw_vox_source& src = spec->sources[s];
        if (!src.rows) return fail(IGW_VOX_ERR_INVALID, "a source's rows must not be NULL");
        if (src.row_stride < IGW_VOX_CELLS) return fail(IGW_VOX_ERR_INVALID, "a source's row_stride must be >= 1089");
        if (src.encoding != IGW_VOX_ONEHOT && src.encoding != IGW_VOX_OCC)
            return fail(IGW_VOX_ERR_INVALID, "a source's encoding must be IGW_VOX_ONEHOT or IGW_VOX_OCC");
        channels += src.encoding == IGW_VOX_ONEHOT ? 6 : 1;
    }
    if (spec->frame != IGW_VOX_WORLD && spec->frame != IGW_VOX_EGO)
        return fail(IGW_VOX_ERR_INVALID, "frame must be IGW_VOX_WORLD or IGW_VOX_EGO");
    if (spec->frame == IGW_VOX_EGO && (spec->radius < 1 || spec->radius > IGW_VOX_MAX_RADIUS))
        return fail(IGW_VOX_ERR_INVALID, "radius must be in 1..10");
    if (spec->dtype < IGW_VOX_U8 || spec->dtype > IGW_VOX_F32) return fail(IGW_VOX_ERR_INVALID, "dtype must be an IGW_VOX_U8 / F16 / BF16 / F32");
    if (spec->stack < 1 || spec->stack > IGW_VOX_MAX_STACK) return fail(IGW_VOX_ERR_INVALID, "stack must be in 1..8");
    if (!__builtin_isfinite(spec->scale) || !__builtin_isfinite(spec->bias))
        return fail(IGW_VOX_ERR_INVALID, "scale and bias must be finite");
    if (spec->dtype == IGW_VOX_U8 && (spec->scale != 1.0f || spec->bias != 0.0f))
        return fail(IGW_VOX_ERR_INVALID, "IGW_VOX_U8 takes scale 1 and bias 0");
    if (spec->restart && spec->restart_stride < 1) return fail(IGW_VOX_ERR_INVALID, "restart_stride must be >= 1");
    const int64_t blocks = n;   // one workgroup per env
    if (blocks > 0x7fffffffll) return fail(IGW_VOX_ERR_INVALID, "n must be below 2^31");
    if (n == 0) return IGW_VOX_OK;
    if (!spec->data) return fail(IGW_VOX_ERR_INVALID, "data must not be NULL");
    const uintptr_t size = spec->dtype == IGW_VOX_U8 ? 1 : spec->dtype == IGW_VOX_F32 ? 4 : 2;
    if (!aligned(spec->data, size)) return fail(IGW_VOX_ERR_INVALID, "data must be aligned to its element size");
    VoxParams p;
    for (int s = 0; s < IGW_VOX_MAX_SOURCES; s++) p.src[s] = s < spec->num_sources ? spec->sources[s] : igw_vox_source{};
    p.agent = static_cast<const uint8_t*>(agent);
    p.aux = static_cast<const uint8_t*>(aux);
    p.data = spec->data;
    p.restart = spec->restart;
    p.restart_stride = spec->restart_stride;
    p.scale = spec->scale;
    p.bias = spec->bias;
    p.nsrc = spec->num_sources;
    p.agent_plane = spec->agent_plane ? 1 : 0;
    p.ego = spec->frame == IGW_VOX_EGO;
    p.R = p.ego ? spec->radius : 5;
    p.dtype = spec->dtype;
    p.stack = spec->stack;
    p.fill = spec->fill;
    p.channels = channels;
    hipLaunchKernelGGL(igw_vox_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_VOX_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_VOX_OK;
}

}  // extern "C"
