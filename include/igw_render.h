/*
 * igw_render.h -- C ABI of the batched first-person renderer (libigw_render.so).
 *
 * The reference's default observation `obs['pov']` (gridworld/render.py, gridworld/env.py:258, 300): the 64 x 64 RGB
 * image the pyglet/OpenGL Renderer draws of the agent's view.  This library ray-casts the same scene for N envs in
 * one launch, straight from the state buffers of the step path (include/igw.h documents their layouts): it READS
 * them and is not part of the step path (libigw_hip.so neither links nor knows it).
 *
 * The scene, camera, texture mapping and colours are specified in DESIGN.md, section "First-person frames"; in short:
 * every occupied cell of the 9 x 11 x 11 grid is a unit cube with all six faces, the ground is the top face of 37 x 37
 * unit quads at y = -1.5, the camera is gluPerspective(90, W/H, 0.1, 30) at the agent's eye with back faces culled,
 * and a pixel is either the clear colour (128, 176, 255, 255) or one atlas texel (GL_NEAREST, no lighting).
 *
 * Plain device pointers; the call is asynchronous on `stream` (hipStream_t as void*, NULL = default stream), never
 * allocates, never synchronises, and returns 0 or a negative igw_render_status (igw_render_last_error() gives the
 * message).  Buffers may be slices of a larger batch or pinned, device-mapped host memory.
 */
#ifndef IGW_RENDER_H
#define IGW_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_RENDER_VERSION 1
#define IGW_RENDER_MAX_SIDE 1024      /* largest frame width / height */
#define IGW_RENDER_MAX_ATLAS 256      /* largest atlas side (texels); the side is a multiple of 8 */
#define IGW_RENDER_CLEAR_RGBA 0xFFFFB080u  /* (128, 176, 255, 255) as little-endian RGBA bytes */

enum igw_render_status {
    IGW_RENDER_OK = 0,
    IGW_RENDER_ERR_INVALID = -1,   /* bad argument */
    IGW_RENDER_ERR_NO_DEVICE = -2, /* no usable HIP device (there is no CPU fallback) */
    IGW_RENDER_ERR_HIP = -3        /* a HIP call failed */
};

int igw_render_version(void);
/* sha256 prefix of the renderer's sources and flags (gridworld_amd/render.py: source_hash) */
const char* igw_render_build_id(void);
const char* igw_render_last_error(void);

/*
 * Renders the current state of n envs into out [n][height][width][channels] uint8 (row 0 = top image row).
 *   agent  [n][64] B   agent records (include/igw.h): f64 x, y, z at 0, yaw at 24, pitch at 32 (degrees)
 *   grid   [n][1104] i8 world grids [y+1][x+5][z+5] (block ids 1..6 = BLUE, GREEN, RED, ORANGE, PURPLE, YELLOW)
 *   occ    [n][48] u32 occupancy bitmaps kept in sync with grid (include/igw.h: IGW_OCC_WORDS)
 *   atlas  [atlas_side][atlas_side][4] uint8 RGBA, row 0 = top image row (as an image file stores it)
 *   channels 3 (RGB) or 4 (RGBA); 1 <= width, height <= IGW_RENDER_MAX_SIDE; atlas_side a multiple of 8, <= 256.
 * n == 0 is a no-op.  Frames are written with 64-bit offsets (65,536 envs x 64 x 64 x 3 = 805 MB).
 */
int igw_render_pov(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                   int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, int32_t channels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
