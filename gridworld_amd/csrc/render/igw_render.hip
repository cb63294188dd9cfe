// igw_render.hip -- batched first-person frames of the IGLU gridworld on gfx950 (include/igw_render.h).
//
// One ray per pixel against the scene of gridworld/render.py: a 3-D DDA over the env's occupancy bitmap inside the
// build-zone box, then the ground plane analytically.  The contract (scene, camera, culling, near / far limits,
// texture mapping) is DESIGN.md, section "First-person frames"; tests/pov_model.py is an independent brute-force
// model of it that the GPU tests compare against.
//
// Layout: block (env, chunk) renders up to kChunk consecutive pixels of one env's frame.  The env's occupancy bitmap
// and grid go to LDS once per block, the camera basis is built once per block in f64 (like the pose it comes from)
// and rounded to f32; every pixel then works in f32 relative to an integer origin next to the eye (all cell and
// ground-quad boundaries are exact half-integers there).  Colours are staged in LDS and leave as 16-byte stores.
// The _aux entries also write per-pixel depth, label and surface planes from the same launch (igw_render_frame.h).
#include <stdio.h>

#include "igw_render_frame.h"

namespace {

constexpr int kAgentBytes = 64;        // include/igw.h: IGW_AGENT_BYTES
constexpr int kTrajBytes = 64;         // include/igw.h: IGW_TRAJ_BYTES

// Every kernel comes in two variants of one body: the plain one (the colour frame alone: render_frame<false>, no
// trace of the planes in its code) and the _aux one (igw_render.h: igw_render_aux; render_frame<true>, `out` may be
// NULL).  The body, prologue included, is a __device__ function template; the kernels only choose the variant.
template <bool kAux>
__device__ __forceinline__ void pov_block(const uint8_t* __restrict__ agent, const int8_t* __restrict__ grid,
                                          const uint32_t* __restrict__ occ, Planes pl,
                                          const uint32_t* __restrict__ atlas, int side, uint8_t* __restrict__ out,
                                          int W, int H, int C) {
    const int tid = threadIdx.x;
    const int64_t env = blockIdx.x;
    if (tid < kGridStride / 16)
        s_grid4[tid] = reinterpret_cast<const uint4*>(grid + env * kGridStride)[tid];
    else if (tid >= 128 && tid < 128 + kOccWords / 4)
        s_occ4[tid - 128] = reinterpret_cast<const uint4*>(occ + env * kOccWords)[tid - 128];
    const double* pose = reinterpret_cast<const double*>(agent + env * kAgentBytes);
    render_frame<kAux>(pose, lds_occ(), lds_grid(), s_stage4, atlas, side, out, env, W, H, C, pl);
}

__global__ __launch_bounds__(kThreads) void igw_render_pov_kernel(const uint8_t* __restrict__ agent,
                                                              const int8_t* __restrict__ grid,
                                                              const uint32_t* __restrict__ occ,
                                                              const uint32_t* __restrict__ atlas, int side,
                                                              uint8_t* __restrict__ out, int W, int H, int C) {
    pov_block<false>(agent, grid, occ, Planes{}, atlas, side, out, W, H, C);
}

__global__ __launch_bounds__(kThreads) void igw_aux_pov_kernel(const uint8_t* __restrict__ agent,
                                                           const int8_t* __restrict__ grid,
                                                           const uint32_t* __restrict__ occ, Planes pl,
                                                           const uint32_t* __restrict__ atlas, int side,
                                                           uint8_t* __restrict__ out, int W, int H, int C) {
    pov_block<true>(agent, grid, occ, pl, atlas, side, out, W, H, C);
}

// Block (episode e, entry t, chunk): frame t of episode e, rebuilt from the episode log (igw_render.h:
// igw_render_episodes).  The grid is the start grid with the last change of every cell among records 0..t-1 applied:
// one strided pass over the records keeps, per cell, max(record << 3 | colour) in an LDS table (the staging area,
// free until the pixels are shaded); the occupancy bitmap is then derived from the grid (build_occ).
template <bool kAux>
__device__ __forceinline__ void episodes_block(
    const uint8_t* __restrict__ records, int64_t n_records, const int64_t* __restrict__ first,
    const int32_t* __restrict__ length, const int64_t* __restrict__ frame0, const int8_t* __restrict__ start_grid,
    const double* __restrict__ init_pose, int max_length, int64_t n_frames, Planes pl,
    const uint32_t* __restrict__ atlas, int side, uint8_t* __restrict__ out, int W, int H, int C) {
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x / (unsigned)(max_length + 1);
    const int t = (int)(blockIdx.x - e * (max_length + 1));
    // device-side values are not trusted: the length is clamped, an episode outside the buffers is not drawn
    const int len = min(max(length[e], 0), max_length);
    const int64_t r0 = first[e], f0 = frame0[e];
    if (t > len || r0 < 0 || r0 > n_records - len || f0 < 0 || f0 > n_frames - (len + 1)) return;

    int* s_last = reinterpret_cast<int*>(s_stage4);
    int8_t* s_grid = lds_grid();
    if (tid < kGridStride / 16) s_grid4[tid] = reinterpret_cast<const uint4*>(start_grid + e * kGridStride)[tid];
    for (int c = tid; c < kCells; c += kThreads) s_last[c] = -1;
    // entry 0: the reset pose (f64, task_meta order x, y, z, yaw, pitch); entry t: the f32 agentPos of record t-1
    // (x, y, z, pitch, yaw) widened to f64
    double pose[5];
    if (t == 0) {
        for (int k = 0; k < 5; k++) pose[k] = init_pose[5 * e + k];
    } else {
        const float* p = reinterpret_cast<const float*>(records + (r0 + t - 1) * kTrajBytes);
        pose[0] = p[0]; pose[1] = p[1]; pose[2] = p[2]; pose[3] = p[4]; pose[4] = p[3];
    }
    __syncthreads();
    const uint8_t* rec = records + r0 * kTrajBytes;
    for (int k = tid; k < t; k += kThreads) {
        const uint32_t ch = *reinterpret_cast<const uint16_t*>(rec + (int64_t)k * kTrajBytes + 40);
        const uint32_t cell = ch & 0x7ffu;
        if (ch != 0xffffu && cell < (uint32_t)kCells) atomicMax(&s_last[cell], (k << 3) | (int)((ch >> 11) & 7u));
    }
    __syncthreads();
    for (int c = tid; c < kCells; c += kThreads) {
        const int w = s_last[c];
        if (w >= 0) s_grid[c] = (int8_t)(w & 7);
    }
    build_occ(s_grid, lds_occ());
    render_frame<kAux>(pose, lds_occ(), s_grid, s_stage4, atlas, side, out, f0 + t, W, H, C, pl);
}

__global__ __launch_bounds__(kThreads) void igw_render_episodes_kernel(
    const uint8_t* __restrict__ records, int64_t n_records, const int64_t* __restrict__ first,
    const int32_t* __restrict__ length, const int64_t* __restrict__ frame0, const int8_t* __restrict__ start_grid,
    const double* __restrict__ init_pose, int max_length, int64_t n_frames, const uint32_t* __restrict__ atlas,
    int side, uint8_t* __restrict__ out, int W, int H, int C) {
    episodes_block<false>(records, n_records, first, length, frame0, start_grid, init_pose, max_length, n_frames,
                          Planes{}, atlas, side, out, W, H, C);
}

__global__ __launch_bounds__(kThreads) void igw_aux_episodes_kernel(
    const uint8_t* __restrict__ records, int64_t n_records, const int64_t* __restrict__ first,
    const int32_t* __restrict__ length, const int64_t* __restrict__ frame0, const int8_t* __restrict__ start_grid,
    const double* __restrict__ init_pose, int max_length, int64_t n_frames, Planes pl,
    const uint32_t* __restrict__ atlas, int side, uint8_t* __restrict__ out, int W, int H, int C) {
    episodes_block<true>(records, n_records, first, length, frame0, start_grid, init_pose, max_length, n_frames, pl,
                         atlas, side, out, W, H, C);
}

// Block (view v, chunk): grid view_grid[v] (or v) seen from pose[v] (igw_render.h: igw_render_views).  The caller has
// only grids, at any row stride, so the block copies the view's 1,089 cells to LDS itself (16-byte loads where the
// rows are aligned, bytes otherwise) and derives the occupancy bitmap there (build_occ).
template <bool kAux>
__device__ __forceinline__ void views_block(const int8_t* __restrict__ grids, int64_t grid_stride, int n_grids,
                                            const int32_t* __restrict__ view_grid, const double* __restrict__ pose,
                                            Planes pl, const uint32_t* __restrict__ atlas, int side,
                                            uint8_t* __restrict__ out, int W, int H, int C) {
    const int tid = threadIdx.x;
    const int64_t v = blockIdx.x;
    // device-side values are not trusted: a view of a row outside the grids is not drawn
    const int64_t row = view_grid ? (int64_t)view_grid[v] : v;
    if (row < 0 || row >= n_grids) return;

    int8_t* s_grid = lds_grid();
    const int8_t* g = grids + row * grid_stride;
    if (((reinterpret_cast<uintptr_t>(grids) | (uintptr_t)grid_stride) & 15) == 0) {
        // aligned rows have a stride >= 1104: the 15 bytes past the cells belong to the row
        if (tid < kGridStride / 16) s_grid4[tid] = reinterpret_cast<const uint4*>(g)[tid];
    } else {
        for (int c = tid; c < kCells; c += kThreads) s_grid[c] = g[c];
    }
    build_occ(s_grid, lds_occ());
    render_frame<kAux>(pose + 5 * v, lds_occ(), s_grid, s_stage4, atlas, side, out, v, W, H, C, pl);
}

__global__ __launch_bounds__(kThreads) void igw_render_views_kernel(
    const int8_t* __restrict__ grids, int64_t grid_stride, int n_grids, const int32_t* __restrict__ view_grid,
    const double* __restrict__ pose, const uint32_t* __restrict__ atlas, int side, uint8_t* __restrict__ out, int W,
    int H, int C) {
    views_block<false>(grids, grid_stride, n_grids, view_grid, pose, Planes{}, atlas, side, out, W, H, C);
}

__global__ __launch_bounds__(kThreads) void igw_aux_views_kernel(
    const int8_t* __restrict__ grids, int64_t grid_stride, int n_grids, const int32_t* __restrict__ view_grid,
    const double* __restrict__ pose, Planes pl, const uint32_t* __restrict__ atlas, int side,
    uint8_t* __restrict__ out, int W, int H, int C) {
    views_block<true>(grids, grid_stride, n_grids, view_grid, pose, pl, atlas, side, out, W, H, C);
}

thread_local char g_err[512] = "";

int fail(int code, const char* entry, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s: %s%s", entry, what, detail);
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

// What every entry point does once its own arguments (counts, nulls, alignments, ranges) are in order: the checks of
// the frame's shape and the atlas, the device, the empty launch, and the launch of `count` x chunks blocks of
// kernel(own..., atlas, side, out, W, H, C).  An invalid argument (-1) comes before a missing device (-2), which
// comes before the no-op of count == 0.
template <typename... Params, typename... Own>
int launch(const char* entry, void (*kernel)(Params...), int64_t count, const uint8_t* atlas, int32_t atlas_side,
           uint8_t* out, int32_t width, int32_t height, int32_t channels, void* stream, Own... own) {
    if (channels != 3 && channels != 4) return fail(IGW_RENDER_ERR_INVALID, entry, "channels must be 3 or 4");
    if (width < 1 || width > IGW_RENDER_MAX_SIDE || height < 1 || height > IGW_RENDER_MAX_SIDE)
        return fail(IGW_RENDER_ERR_INVALID, entry, "width and height must be in 1..1024");
    if (atlas_side < 8 || atlas_side > IGW_RENDER_MAX_ATLAS || atlas_side % 8)
        return fail(IGW_RENDER_ERR_INVALID, entry, "atlas_side must be a multiple of 8 in 8..256");
    if (!have_device())
        return fail(IGW_RENDER_ERR_NO_DEVICE, entry, "no HIP device available (the renderer has no CPU fallback)");
    if (count == 0) return IGW_RENDER_OK;
    const int chunks = (width * height + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(kernel, dim3((unsigned)count, (unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, own...,
                       reinterpret_cast<const uint32_t*>(atlas), (int)atlas_side, out, (int)width, (int)height,
                       (int)channels);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_RENDER_ERR_HIP, entry, "launch failed: ", hipGetErrorString(e));
    return IGW_RENDER_OK;
}

// The planes of an _aux entry, read on the host at call time (aux == NULL: none).
Planes planes_of(const igw_render_aux* aux) {
    return aux ? Planes{aux->depth, aux->label, aux->surface} : Planes{nullptr, nullptr, nullptr};
}

// What an entry's frame and planes must satisfy (`pl` == NULL: the plain entry, whose `out` is checked with its other
// buffers): something to write, and planes aligned for their element stores.  Returns 0 or the failure.
int check_outputs(const char* entry, const uint8_t* out, const Planes* pl) {
    if (!pl) return 0;
    if (!out && !pl->depth && !pl->label && !pl->surface)
        return fail(IGW_RENDER_ERR_INVALID, entry, "nothing to write: out and every plane are NULL");
    if (!aligned(pl->depth, 4) || !aligned(pl->surface, 2))
        return fail(IGW_RENDER_ERR_INVALID, entry, "depth must be 4-byte, surface 2-byte aligned");
    return 0;
}

// The three pairs of entry points: the plain entry passes pl == NULL (its `out` is required, its kernel the plain
// one), the _aux entry its planes (any of `out` and the planes may be NULL, but not all).
int pov_entry(const char* entry, const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n,
              const uint8_t* atlas, int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, int32_t channels,
              const Planes* pl, void* stream) {
    if (n < 0) return fail(IGW_RENDER_ERR_INVALID, entry, "n must be >= 0");
    if (n > 0 && (!agent || !grid || !occ || !atlas || (!pl && !out)))
        return fail(IGW_RENDER_ERR_INVALID, entry, "null buffer");
    if (!aligned(agent, 8) || !aligned(grid, 16) || !aligned(occ, 16) || !aligned(atlas, 4))
        return fail(IGW_RENDER_ERR_INVALID, entry, "agent must be 8-byte, grid and occ 16-byte, atlas 4-byte "
                                                   "aligned");
    if (const int rc = check_outputs(entry, out, pl)) return rc;
    if (pl)
        return launch(entry, igw_aux_pov_kernel, n, atlas, atlas_side, out, width, height, channels, stream,
                      static_cast<const uint8_t*>(agent), grid, occ, *pl);
    return launch(entry, igw_render_pov_kernel, n, atlas, atlas_side, out, width, height, channels, stream,
                  static_cast<const uint8_t*>(agent), grid, occ);
}

int episodes_entry(const char* entry, const uint8_t* records, int64_t n_records, const int64_t* first,
                   const int32_t* length, const int64_t* frame0, const int8_t* start_grid, const double* init_pose,
                   int32_t m, int32_t max_length, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                   int64_t n_frames, int32_t width, int32_t height, int32_t channels, const Planes* pl, void* stream) {
    if (m < 0) return fail(IGW_RENDER_ERR_INVALID, entry, "m must be >= 0");
    if (max_length < 0 || max_length > IGW_RENDER_MAX_EPISODE)
        return fail(IGW_RENDER_ERR_INVALID, entry, "max_length must be in 0..2^24");
    if ((int64_t)m * (max_length + 1) > INT32_MAX)
        return fail(IGW_RENDER_ERR_INVALID, entry, "m * (max_length + 1) must be < 2^31");
    if (n_records < 0 || n_frames < 0)
        return fail(IGW_RENDER_ERR_INVALID, entry, "n_records and n_frames must be >= 0");
    if (m > 0 && (!records || !first || !length || !frame0 || !start_grid || !init_pose || !atlas || (!pl && !out)))
        return fail(IGW_RENDER_ERR_INVALID, entry, "null buffer");
    if (!aligned(records, 16) || !aligned(first, 8) || !aligned(length, 4) || !aligned(frame0, 8) ||
        !aligned(start_grid, 16) || !aligned(init_pose, 8) || !aligned(atlas, 4))
        return fail(IGW_RENDER_ERR_INVALID, entry, "records and start_grid must be 16-byte, first, frame0 and "
                                                   "init_pose 8-byte, length and atlas 4-byte aligned");
    if (const int rc = check_outputs(entry, out, pl)) return rc;
    const int64_t blocks = (int64_t)m * (max_length + 1);
    if (pl)
        return launch(entry, igw_aux_episodes_kernel, blocks, atlas, atlas_side, out, width, height, channels, stream,
                      records, n_records, first, length, frame0, start_grid, init_pose, (int)max_length, n_frames, *pl);
    return launch(entry, igw_render_episodes_kernel, blocks, atlas, atlas_side, out, width, height, channels, stream,
                  records, n_records, first, length, frame0, start_grid, init_pose, (int)max_length, n_frames);
}

int views_entry(const char* entry, const int8_t* grids, int64_t grid_stride, int32_t n_grids, const int32_t* view_grid,
                const double* pose, int32_t m, const uint8_t* atlas, int32_t atlas_side, uint8_t* out, int32_t width,
                int32_t height, int32_t channels, const Planes* pl, void* stream) {
    if (m < 0 || n_grids < 0) return fail(IGW_RENDER_ERR_INVALID, entry, "m and n_grids must be >= 0");
    if (grid_stride < kCells) return fail(IGW_RENDER_ERR_INVALID, entry, "grid_stride must be >= 1089");
    if (!view_grid && n_grids < m)
        return fail(IGW_RENDER_ERR_INVALID, entry, "without view_grid, view v shows row v: n_grids must be >= m");
    if (m > 0 && (!grids || !pose || !atlas || (!pl && !out))) return fail(IGW_RENDER_ERR_INVALID, entry, "null buffer");
    if (!aligned(view_grid, 4) || !aligned(pose, 8) || !aligned(atlas, 4))
        return fail(IGW_RENDER_ERR_INVALID, entry, "pose must be 8-byte, view_grid and atlas 4-byte aligned");
    if (const int rc = check_outputs(entry, out, pl)) return rc;
    if (pl)
        return launch(entry, igw_aux_views_kernel, m, atlas, atlas_side, out, width, height, channels, stream, grids,
                      grid_stride, (int)n_grids, view_grid, pose, *pl);
    return launch(entry, igw_render_views_kernel, m, atlas, atlas_side, out, width, height, channels, stream, grids,
                  grid_stride, (int)n_grids, view_grid, pose);
}

}  // namespace

#ifndef IGW_RENDER_BUILD_ID
#define IGW_RENDER_BUILD_ID "igw-render-build-id:unstamped"
#endif

extern "C" {

int igw_render_version(void) { return IGW_RENDER_VERSION; }
// (the string carries a marker so that render.py can read the id of a library file without loading it)
const char* igw_render_build_id(void) { return &IGW_RENDER_BUILD_ID[sizeof("igw-render-build-id:") - 1]; }
const char* igw_render_last_error(void) { return g_err; }

int igw_render_pov(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                   int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, int32_t channels, void* stream) {
    return pov_entry(__func__, agent, grid, occ, n, atlas, atlas_side, out, width, height, channels, nullptr, stream);
}

int igw_render_pov_aux(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                       int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, int32_t channels,
                       const igw_render_aux* aux, void* stream) {
    const Planes pl = planes_of(aux);
    return pov_entry(__func__, agent, grid, occ, n, atlas, atlas_side, out, width, height, channels, &pl, stream);
}

int igw_render_episodes(const uint8_t* records, int64_t n_records, const int64_t* first, const int32_t* length,
                        const int64_t* frame0, const int8_t* start_grid, const double* init_pose, int32_t m,
                        int32_t max_length, const uint8_t* atlas, int32_t atlas_side, uint8_t* out, int64_t n_frames,
                        int32_t width, int32_t height, int32_t channels, void* stream) {
    return episodes_entry(__func__, records, n_records, first, length, frame0, start_grid, init_pose, m, max_length,
                          atlas, atlas_side, out, n_frames, width, height, channels, nullptr, stream);
}

int igw_render_episodes_aux(const uint8_t* records, int64_t n_records, const int64_t* first, const int32_t* length,
                            const int64_t* frame0, const int8_t* start_grid, const double* init_pose, int32_t m,
                            int32_t max_length, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                            int64_t n_frames, int32_t width, int32_t height, int32_t channels,
                            const igw_render_aux* aux, void* stream) {
    const Planes pl = planes_of(aux);
    return episodes_entry(__func__, records, n_records, first, length, frame0, start_grid, init_pose, m, max_length,
                          atlas, atlas_side, out, n_frames, width, height, channels, &pl, stream);
}

int igw_render_views(const int8_t* grids, int64_t grid_stride, int32_t n_grids, const int32_t* view_grid,
                     const double* pose, int32_t m, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                     int32_t width, int32_t height, int32_t channels, void* stream) {
    return views_entry(__func__, grids, grid_stride, n_grids, view_grid, pose, m, atlas, atlas_side, out, width,
                       height, channels, nullptr, stream);
}

int igw_render_views_aux(const int8_t* grids, int64_t grid_stride, int32_t n_grids, const int32_t* view_grid,
                         const double* pose, int32_t m, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                         int32_t width, int32_t height, int32_t channels, const igw_render_aux* aux, void* stream) {
    const Planes pl = planes_of(aux);
    return views_entry(__func__, grids, grid_stride, n_grids, view_grid, pose, m, atlas, atlas_side, out, width,
                       height, channels, &pl, stream);
}

}  // extern "C"
