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
#define IGW_RENDER_HAS_AUX 1          /* the _aux entries and igw_render_aux below exist (an addition to version 1) */
#define IGW_RENDER_MAX_SIDE 1024      /* largest frame width / height */
#define IGW_RENDER_MAX_ATLAS 256      /* largest atlas side (texels); the side is a multiple of 8 */
#define IGW_RENDER_CLEAR_RGBA 0xFFFFB080u  /* (128, 176, 255, 255) as little-endian RGBA bytes */
#define IGW_RENDER_MAX_EPISODE (1 << 24)  /* largest max_length of igw_render_episodes */

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

/*
 * Renders every entry of m logged episodes from the episode log of the step path (include/igw.h:
 * igw_set_trajectory_log), in one launch.  Episode e has length[e] + 1 frames, written to out[frame0[e] + t]
 * ([n_frames][height][width][channels] uint8) for t = 0 .. length[e]:
 *   t = 0   the reset state: start_grid[e] seen from init_pose[e] (f64);
 *   t >= 1  the state after step t: start_grid[e] with the `change` of records[first[e]] .. records[first[e] + t - 1]
 *           applied in order, seen from the f32 agentPos of records[first[e] + t - 1] widened to f64 (agentPos is
 *           x, y, z, pitch, yaw: the angles are swapped against init_pose).
 * Frame t is bit-identical to what igw_render_pov draws for an agent record holding that pose and that grid.
 *   records    [n_records][IGW_TRAJ_BYTES] the log (16-byte aligned); an episode's records are consecutive
 *   first      [m] i64  index in records of the episode's first record
 *   length     [m] i32  steps recorded; clamped to 0 .. max_length on the device
 *   frame0     [m] i64  index in out of the episode's entry 0
 *   start_grid [m][1104] i8 grid the reset wrote (the task row's starting grid, include/igw.h: task_start)
 *   init_pose  [m][5] f64  x, y, z, yaw, pitch of the reset (task_meta bytes 0..39)
 * Every array is a device array and is read on the device only: the call never reads it on the host, never
 * allocates, never synchronises.  Device-side values are not trusted: a change to a cell >= 1089 is ignored, and an
 * episode whose records [first, first + length) or frames [frame0, frame0 + length] fall outside n_records / n_frames
 * is not drawn.  Frames of entries past length[e] are not written.  0 <= max_length <= IGW_RENDER_MAX_EPISODE and
 * m * (max_length + 1) < 2^31; atlas, size and channels as for igw_render_pov.  m == 0 is a no-op.
 */
int igw_render_episodes(const uint8_t* records, int64_t n_records, const int64_t* first, const int32_t* length,
                        const int64_t* frame0, const int8_t* start_grid, const double* init_pose, int32_t m,
                        int32_t max_length, const uint8_t* atlas, int32_t atlas_side, uint8_t* out, int64_t n_frames,
                        int32_t width, int32_t height, int32_t channels, void* stream);

/*
 * Renders m views into out [m][height][width][channels] uint8, in one launch: view v shows grid view_grid[v] from
 * pose[v].  Neither the camera nor the scene is tied to an env: any grid from any pose (the reference's
 * gridworld/visualizer.py), e.g. goal images, spectator cameras of a running batch, orbits of one structure.
 *   grids      [n_grids] rows of int8 cells [y+1][x+5][z+5], row r starting at grids + r * grid_stride elements
 *              (grid_stride >= 1089: 1089 for a dense [G, 9, 11, 11] array, 1104 for the step path's grid_buf,
 *              task_target and task_start of include/igw.h, which are read in place).  A cell is occupied iff it is
 *              not 0; ids outside 1..6 are drawn as the nearer of 1 and 6, as by igw_render_pov.  No alignment is
 *              required; rows whose base and stride are multiples of 16 bytes are fetched with 16-byte loads.
 *   view_grid  [m] i32 row of each view, or NULL: view v shows row v (then n_grids >= m)
 *   pose       [m][5] f64 x, y, z, yaw, pitch (degrees; the order of an agent record and of init_pose)
 * The occupancy bitmap is derived from the grid on the device, so there is no occupancy input.  For a grid with ids
 * 0..6, view v is bit-identical to what igw_render_pov draws for an agent record holding pose[v] over that grid with
 * its matching bitmap (the same per-block body).  The eye may be anywhere: outside the build zone, beyond the ground,
 * below it (then the ground is not drawn: it has a top face only); surfaces beyond depth 30 are clipped as always.
 * Every array is a device array and is read on the device only: the call never reads it on the host, never
 * allocates, never synchronises.  Device-side values are not trusted: a view whose view_grid[v] is outside
 * [0, n_grids) is not drawn (its frame is left unwritten).  Atlas, size and channels as for igw_render_pov.
 * m == 0 is a no-op.  Frames are written with 64-bit offsets.
 */
int igw_render_views(const int8_t* grids, int64_t grid_stride, int32_t n_grids, const int32_t* view_grid,
                     const double* pose, int32_t m, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                     int32_t width, int32_t height, int32_t channels, void* stream);

/*
 * Planes: what the ray caster knows about a pixel beside its colour, written by the same launch that draws the frame.
 * Each plane is [n][height][width] over the frames of its entry (row 0 = top image row), indexed like `out` with
 * 64-bit offsets, and follows the colour's visibility contract ("First-person frames": the first face
 * entered with 0.1 <= t <= 30, else the ground from above within +-18.5, else sky):
 *   depth   f32  the ray parameter t of the visible surface = its eye-space depth; +inf for sky.  4-byte aligned.
 *   label   u8   0 sky, 1..6 the block's colour BLUE..YELLOW (an id outside 1..6 as the nearer of 1 and 6, like the
 *                colour), 7 WHITE ground, 8 GREY ground.
 *   surface i16  sky: -1.  Block: face * 1089 + cell, face 0..5 = top, bottom, left, right, front, back (the side
 *                the ray enters through), cell = (y+1)*121 + (x+5)*11 + (z+5) of world (x, y, z), the grid's own
 *                index.  Ground: 6 * 1089 + (qx + 18) * 37 + (qz + 18) for the quad centred at (qx, qz).
 *                2-byte aligned.
 * A pose the colour path treats as seeing nothing (not finite, or beyond 1e4) gives sky in all three.
 * Every pointer is a device pointer or NULL (plane not wanted: no store is issued for it).  The struct itself is host
 * memory, read during the call; the kernel receives the three pointers by value.
 */
typedef struct igw_render_aux {
    float* depth;
    uint8_t* label;
    int16_t* surface;
} igw_render_aux;

/*
 * igw_render_pov / igw_render_episodes / igw_render_views with planes: the arguments of the sibling, plus `aux` in
 * front of `stream` (NULL = no planes).  The frame is byte-identical to the sibling's, and the planes do not depend
 * on whether `out` is given.  Here `out` may be NULL (planes only: no texel is fetched, no colour stored); at least
 * one of `out` and the three planes must not be NULL (IGW_RENDER_ERR_INVALID otherwise).  The planes follow the frame
 * indexing of their entry: env i for pov; frame0[e] + t within n_frames for episodes, entries past length[e] left
 * unwritten; view v for views, an undrawn view left unwritten.  Everything else (checks, device-side clamps, n == 0,
 * asynchrony) is the sibling's.
 */
int igw_render_pov_aux(const void* agent, const int8_t* grid, const uint32_t* occ, int32_t n, const uint8_t* atlas,
                       int32_t atlas_side, uint8_t* out, int32_t width, int32_t height, int32_t channels,
                       const igw_render_aux* aux, void* stream);
int igw_render_episodes_aux(const uint8_t* records, int64_t n_records, const int64_t* first, const int32_t* length,
                            const int64_t* frame0, const int8_t* start_grid, const double* init_pose, int32_t m,
                            int32_t max_length, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                            int64_t n_frames, int32_t width, int32_t height, int32_t channels,
                            const igw_render_aux* aux, void* stream);
int igw_render_views_aux(const int8_t* grids, int64_t grid_stride, int32_t n_grids, const int32_t* view_grid,
                         const double* pose, int32_t m, const uint8_t* atlas, int32_t atlas_side, uint8_t* out,
                         int32_t width, int32_t height, int32_t channels, const igw_render_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif
