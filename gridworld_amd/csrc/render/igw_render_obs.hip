// igw_render_obs.hip -- libigw_render_obs.so: igw_render_pov_obs (include/igw_render_obs.h), the first-person frame of
// igw_render_pov together with the observation a policy network reads, in one launch.
//
// The kernel is the plain pov kernel of igw_render.hip -- the same prologue and the one ray caster, render_frame() of
// igw_render_frame.h, compiled here unchanged -- followed by the observation stage (igw_render_obs_stage.h), which
// reads the chunk's colours where render_frame() left them staged in LDS.  It is a library of its own so that
// libigw_render.so, its sources and its build id stay what they were.
#include <stdio.h>

#include "igw_render_obs_stage.h"

namespace {

constexpr int kAgentBytes = 64;        // include/igw.h: IGW_AGENT_BYTES

// render_frame() always flushes its staging to `out`.  A call without a frame (out == NULL) aims that flush at a slot
// of this sink instead: kSinkSlots chunk-sized slots shared by the blocks in flight (what lands there is never read;
// blocks that share a slot overwrite one another).  It stays cache-resident, so the flush costs no more than the frame.
constexpr int kSinkSlots = 2048;
__device__ uint4 g_sink[kSinkSlots * (kChunk * 3 / 16)];

// Block (env, chunk): the pov kernel's body with C = 3, then the observation of the same chunk.
__global__ __launch_bounds__(kThreads) void igw_obs_pov_kernel(const uint8_t* __restrict__ agent,
                                                           const int8_t* __restrict__ grid,
                                                           const uint32_t* __restrict__ occ, ObsOut ob,
                                                           const uint32_t* __restrict__ atlas, int side,
                                                           uint8_t* __restrict__ out, int W, int H) {
    const int tid = threadIdx.x;
    const int64_t env = blockIdx.x;
    if (tid < kGridStride / 16)
        s_grid4[tid] = reinterpret_cast<const uint4*>(grid + env * kGridStride)[tid];
    else if (tid >= 128 && tid < 128 + kOccWords / 4)
        s_occ4[tid - 128] = reinterpret_cast<const uint4*>(occ + env * kOccWords)[tid - 128];
    const double* pose = reinterpret_cast<const double*>(agent + env * kAgentBytes);
    const int wh = W * H, c0 = blockIdx.y * kChunk;
    uint8_t* dst = out;
    int64_t frame = env;
    if (!out) {   // block-uniform: render_frame() stores at dst + (frame * wh + c0) * 3
        const unsigned slot = (blockIdx.x * gridDim.y + blockIdx.y) % (unsigned)kSinkSlots;
        dst = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(g_sink) + (uintptr_t)slot * (kChunk * 3) -
                                         (uintptr_t)c0 * 3);
        frame = 0;
    }
    render_frame<false>(pose, lds_occ(), lds_grid(), s_stage4, atlas, side, dst, frame, W, H, 3);
    // every thread is past the barrier that published the staged colours, and nothing writes them again
    ob.store(reinterpret_cast<const uint8_t*>(s_stage4), env, wh, c0, min(kChunk, wh - c0));
}

thread_local char g_err[512] = "";

int fail(int code, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "igw_render_pov_obs: %s%s", what, detail);
    return code;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

bool have_device() {
    static int seen = 0;   // once a device was seen it stays (the count is not re-queried per frame)
    if (!seen) {
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1) return false;
        seen = 1;
    }
    return true;
}

}  // namespace

#ifndef IGW_RENDER_OBS_BUILD_ID
#define IGW_RENDER_OBS_BUILD_ID "igw-render-obs-build-id:unstamped"
#endif

static_assert(sizeof(igw_render_obs) == IGW_RENDER_OBS_BYTES, "include/igw_render_obs.h: IGW_RENDER_OBS_BYTES");

extern "C" {

// (the string carries a marker so that render.py can read the id of a library file without loading it)
const char* igw_render_obs_build_id(void) { return &IGW_RENDER_OBS_BUILD_ID[sizeof("igw-render-obs-build-id:") - 1]; }
const char* igw_render_obs_last_error(void) { return g_err; }

// The checks come in igw_render_pov's order: an invalid argument (-1) before a missing device (-2) before the no-op
// of n == 0.
int igw_render_pov_obs(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                       int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, const igw_render_obs* obs,
                       void* stream) {
    if (!obs) return fail(IGW_RENDER_ERR_INVALID, "obs is NULL");
    if (n < 0) return fail(IGW_RENDER_ERR_INVALID, "n must be >= 0");
    if (n > 0 && (!agent || !grid || !occ || !atlas)) return fail(IGW_RENDER_ERR_INVALID, "null buffer");
    if (!aligned(agent, 8) || !aligned(grid, 16) || !aligned(occ, 16) || !aligned(atlas, 4))
        return fail(IGW_RENDER_ERR_INVALID, "agent must be 8-byte, grid and occ 16-byte, atlas 4-byte aligned");
    if (obs->dtype < IGW_OBS_U8 || obs->dtype > IGW_OBS_F32)
        return fail(IGW_RENDER_ERR_INVALID, "obs.dtype must be an IGW_OBS_*");
    if (obs->stack < 1 || obs->stack > IGW_RENDER_MAX_STACK)
        return fail(IGW_RENDER_ERR_INVALID, "obs.stack must be in 1..8");
    if (!isfinite(obs->scale) || !isfinite(obs->bias))
        return fail(IGW_RENDER_ERR_INVALID, "obs.scale and obs.bias must be finite");
    if (obs->dtype == IGW_OBS_U8 && (obs->scale != 1.f || obs->bias != 0.f))
        return fail(IGW_RENDER_ERR_INVALID, "IGW_OBS_U8 takes scale 1 and bias 0");
    if (n > 0 && !obs->data) return fail(IGW_RENDER_ERR_INVALID, "obs.data is NULL");
    if (!aligned(obs->data, obs->dtype == IGW_OBS_U8 ? 1 : obs->dtype == IGW_OBS_F32 ? 4 : 2))
        return fail(IGW_RENDER_ERR_INVALID, "obs.data must be aligned to its element size");
    if (obs->restart && obs->restart_stride < 1)
        return fail(IGW_RENDER_ERR_INVALID, "obs.restart_stride must be >= 1");
    if (width < 1 || width > IGW_RENDER_MAX_SIDE || height < 1 || height > IGW_RENDER_MAX_SIDE)
        return fail(IGW_RENDER_ERR_INVALID, "width and height must be in 1..1024");
    if (atlas_side < 8 || atlas_side > IGW_RENDER_MAX_ATLAS || atlas_side % 8)
        return fail(IGW_RENDER_ERR_INVALID, "atlas_side must be a multiple of 8 in 8..256");
    if (!have_device())
        return fail(IGW_RENDER_ERR_NO_DEVICE, "no HIP device available (the renderer has no CPU fallback)");
    if (n == 0) return IGW_RENDER_OK;
    const ObsOut ob{obs->data, obs->restart, obs->restart_stride, obs->scale, obs->bias,
                    obs->dtype, obs->gray != 0, obs->stack, obs->fill != 0};
    const int chunks = (width * height + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(igw_obs_pov_kernel, dim3((unsigned)n, (unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(agent), grid, occ, ob, reinterpret_cast<const uint32_t*>(atlas),
                       (int)atlas_side, out, (int)width, (int)height);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_RENDER_ERR_HIP, "launch failed: ", hipGetErrorString(e));
    return IGW_RENDER_OK;
}

}  // extern "C"
