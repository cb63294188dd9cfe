// igw_vox.hip -- libigw_vox.so: igw_vox_obs (include/igw_vox.h), the state as the tensor a policy network reads:
// channel-first one-hot / occupancy planes of up to four grids and the agent's body, in the world's or the agent's
// frame, in u8 / f16 / bf16 / f32, stacked over the last K calls -- one launch, a pure streaming writer.
//
// One workgroup of 256 lanes per env.  The element, the frame of a pose and the writer of a slot at the absolute 16-byte
// boundaries are csrc/igw_voxel.h's, shared with the recall query, where the stage / write story is told; this file's own:
//   stage   The channel table and the staging loop are csrc/igw_voxel_table.h and igw_voxel_stage.h, statements
//           included in the kernel body; a plane's value is read from the source's row of this env or of its task
//           (by_task), plus the row to add where there is one: global loads, for cells inside the grid only.
//   run     An env's run of stack * C * 9 * S * S elements starts wherever the runs before it end.  A restarted env
//           (or fill) takes the new planes in every slot; any other shifts its slots down and takes them in the last.
//   shift   Slot k takes slot k + 1 piece by piece: the destination pieces are the aligned ones, the source is read at
//           whatever alignment it has (a 16-byte load at element alignment).  Pieces of two slots do not coincide, so a
//           barrier separates slot k's copy from the write of slot k + 1: everything read from a slot has arrived
//           (the stores before the barrier consumed it) before any lane writes that slot.
// Loop bounds depend on the spec only; nothing is allocated, nothing synchronises across workgroups.
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "../../../include/igw_vox.h"
#include "../igw_voxel.h"

namespace {

using namespace voxel;

static_assert(IGW_VOX_U8 == kU8 && IGW_VOX_F16 == kF16 && IGW_VOX_BF16 == kBF16 && IGW_VOX_F32 == kF32, "element types");
static_assert(IGW_VOX_ONEHOT == kOneHot && IGW_VOX_OCC == kOcc, "encodings");
static_assert(IGW_VOX_LEVELS == kLevels && IGW_VOX_MAX_RADIUS == kMaxRadius && IGW_VOX_MAX_SOURCES == kMaxSources, "limits");
constexpr int kPlanes = kMaxSources + 1;                       // the sources' and the agent's

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

// Which 16-byte stores are non-temporal: 1 = those of the new planes (the default: what won the A/B of
// profiles/LAB_NOTEBOOK.md), 0 = none, 2 = those of the shift too (the A/B's other arms).
#ifndef IGW_VOX_NT_STORES
#define IGW_VOX_NT_STORES 1
#endif

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
        store16<IGW_VOX_NT_STORES >= 2>(dst + e0, v);
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
    const E v0 = elem_value<kDtype>(0u, p.scale, p.bias), v1 = elem_value<kDtype>(1u, p.scale, p.bias);
    const int K = p.stack, L = p.channels * pl.P9;
    E* run = static_cast<E*>(p.data) + env * K * (int64_t)L;
    const bool all = p.fill != 0 || (p.restart != nullptr && p.restart[env * p.restart_stride] != 0);
    if (all) {
        for (int k = 0; k < K; k++) write_slot<kDtype, IGW_VOX_NT_STORES >= 1>(run + (int64_t)k * L, L, pl, v0, v1);
    } else {
        for (int k = 0; k + 1 < K; k++) {
            shift_down<E>(run + (int64_t)k * L, L);
            __syncthreads();
        }
        write_slot<kDtype, IGW_VOX_NT_STORES >= 1>(run + (int64_t)(K - 1) * L, L, pl, v0, v1);
    }
}

// What igw_voxel_table.h and igw_voxel_stage.h take from this kernel: a plane's value is the source's row of this env or
// of its task, plus the row to add where there is one.
#define VOXEL_PLANES p.nsrc
#define VOXEL_AGENT p.agent_plane
#define VOXEL_ENCODING(k) p.src[k].encoding
#define VOXEL_EGO p.ego
#define VOXEL_GUARD_CELL 0
#define VOXEL_READ(k, c, v)                                                                  \
    const int64_t at = (p.src[k].by_task ? task : env) * p.src[k].row_stride + (c);          \
    int v = p.src[k].rows[at];                                                               \
    if (p.src[k].add) v += p.src[k].add[at];

__global__ __launch_bounds__(kThreads) void igw_vox_kernel(const VoxParams p) {
    __shared__ uint8_t cells[kPlanes * kMaxPlane];
    __shared__ uint8_t ch_plane[kTable], ch_match[kTable];
    const int tid = threadIdx.x;
    const int64_t env = blockIdx.x;
    const int R = p.R, S = p.ego ? 2 * R + 1 : 11, SS = S * S, P9 = kLevels * SS;

    const double* pose = reinterpret_cast<const double*>(p.agent + env * 64);
    const Frame fr(pose[0], pose[1], pose[2], pose[3]);
    const int64_t task = *reinterpret_cast<const int32_t*>(p.aux + env * 16 + 8);

#include "../igw_voxel_table.h"
#include "../igw_voxel_stage.h"
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
