/*
 * igw_vox.h -- C ABI of the voxel observation of the vector-state path (libigw_vox.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (grid rows, agent and episode records, the task
 * table) and the goal query's rows (include/igw_goal.h) and writes only its output; libigw_hip.so and the other
 * libraries, their sources and their build ids stay what they were.  Every pointer but the spec is a device pointer
 * (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on it, never allocate and never
 * synchronise.
 */
#ifndef IGW_VOX_H_ABI
#define IGW_VOX_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_VOX_VERSION 1
#define IGW_VOX_MAX_SOURCES 4
#define IGW_VOX_MAX_STACK 8
#define IGW_VOX_MAX_RADIUS 10
#define IGW_VOX_CELLS 1089             /* 9 * 11 * 11; cell c = y * 121 + x * 11 + z */
#define IGW_VOX_LEVELS 9
#define IGW_VOX_SPEC_BYTES 192         /* sizeof(igw_vox_spec) */

enum igw_vox_status {
    IGW_VOX_OK = 0,
    IGW_VOX_ERR_INVALID = -1,          /* bad argument */
    IGW_VOX_ERR_HIP = -3               /* a HIP call failed (no usable device included) */
};
enum { IGW_VOX_ONEHOT = 0, IGW_VOX_OCC = 1 };                     /* igw_vox_source.encoding */
enum { IGW_VOX_WORLD = 0, IGW_VOX_EGO = 1 };                      /* igw_vox_spec.frame */
enum { IGW_VOX_U8 = 0, IGW_VOX_F16 = 1, IGW_VOX_BF16 = 2, IGW_VOX_F32 = 3 };   /* igw_vox_spec.dtype (= IGW_OBS_*) */

int igw_vox_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/vox.py: LIBRARY.source_hash) */
const char* igw_vox_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_vox_last_error(void);

/*
 * One grid of colour ids per env.  Env i reads row r = by_task ? aux[i].task : i (the int32 at offset 8 of the 16-byte
 * episode record); the value of cell c is v = rows[r * row_stride + c] + (add ? add[r * row_stride + c] : 0), summed
 * as int.  row_stride >= 1089 bytes; no alignment is required of rows / add (the 1104-byte state rows and a contiguous
 * [n][9][11][11] array both work).  `add` makes the user's target of the task table's synthetic one: task_target +
 * task_start by task row (include/igw.h).
 *   IGW_VOX_ONEHOT  6 channels, channel k = [v == k + 1]; a value outside 1..6 sets none
 *   IGW_VOX_OCC     1 channel, [v != 0]
 */
typedef struct igw_vox_source {
    const int8_t* rows;
    const int8_t* add;              /* NULL, or rows of the same stride and indexing added cell by cell */
    int64_t       row_stride;       /* bytes */
    int32_t       by_task;          /* != 0: the row is the env's task row */
    int32_t       encoding;         /* IGW_VOX_ONEHOT / IGW_VOX_OCC */
} igw_vox_source;

/*
 * The observation: data [n][stack][C][9][S][S] elements of `dtype`, indexed with 64-bit offsets.  C = the sources'
 * channels in their order, then one agent channel if agent_plane; S = 11 (IGW_VOX_WORLD) or 2 * radius + 1
 * (IGW_VOX_EGO, radius 1..10).
 *
 * Agent channel: with the binary64 pose of the 64-byte agent record (x, y, z, yaw at offsets 0 / 8 / 16 / 24) the head
 * cell is (hx, hy, hz) = (rint(x) + 5, rint(y) + 1, rint(z) + 5), rint = round-half-even; the channel is 1 at the head
 * cell and at (hx, hy - 1, hz) where those lie inside 0..10 x 0..8 x 0..10.
 *
 * WORLD: plane[y][x][z] is the bit of cell (y, x, z).  EGO: the level y is kept; the x / z window is centred on the head
 * cell and turned by the heading quadrant q = floor((yaw + 45.0) / 90.0) mod 4 (binary64, non-negative result; yaw in
 * degrees): output [y][u][w] reads world cell (y, hx + a, hz + b) with s = R - u cells ahead, t = w - R cells to the
 * right and (a, b) = s * f_q + t * r_q, f_0..3 = (0,-1), (1,0), (0,1), (-1,0), r_0..3 = (1,0), (0,1), (-1,0), (0,-1).
 * A world cell outside the grid reads 0 in every channel, the agent channel included.
 *
 * Element: b in {0, 1}.  IGW_VOX_U8 stores b (scale 1, bias 0 required); IGW_VOX_F32 (float)b * scale, then + bias,
 * two f32 operations that are never fused; IGW_VOX_F16 / IGW_VOX_BF16 that f32 value rounded to nearest-even.
 *
 * Stack and restart: include/igw_render_obs.h's rule.  Slot stack - 1 holds the planes of this call, slot 0 the
 * oldest.  If `fill` is set or env i restarts (restart != NULL and restart[i * restart_stride] != 0, a device byte per
 * env at any stride in bytes: 64 for the `done` byte of the step's output records, 1 for a mask) every slot becomes the
 * new planes; otherwise slot k takes the old slot k + 1 (in place) and slot stack - 1 the new planes.  With stack == 1
 * `data` is never read.  `data` need only be aligned to its element size.
 * The struct itself is host memory, read during the call; its values reach the kernel by value.
 */
typedef struct igw_vox_spec {
    igw_vox_source sources[IGW_VOX_MAX_SOURCES];
    int32_t        num_sources;     /* 1..4 */
    int32_t        agent_plane;     /* 0 / 1 */
    int32_t        frame;           /* IGW_VOX_WORLD / IGW_VOX_EGO */
    int32_t        radius;          /* R, 1..10 (EGO only) */
    int32_t        dtype;           /* IGW_VOX_U8 / F16 / BF16 / F32 */
    int32_t        stack;           /* K, 1..8 */
    int32_t        fill;            /* != 0: every env restarts its stack in this call */
    int32_t        reserved;
    float          scale, bias;
    void*          data;
    const uint8_t* restart;         /* NULL, or env i restarts iff restart[i * restart_stride] != 0 */
    int64_t        restart_stride;  /* bytes */
} igw_vox_spec;

/*
 * Writes the observation of envs [0, n): agent [n] 64-byte records (8-byte aligned), aux [n] 16-byte records (4-byte
 * aligned).  Nothing outside data[0 .. n * stack * C * 9 * S * S) is written; no state buffer is.  n == 0 is a no-op.
 * Returns IGW_VOX_OK; IGW_VOX_ERR_INVALID for a NULL agent, aux, spec or data (n > 0), n < 0, 0 or more than 4
 * sources, a NULL rows, a row_stride < 1089, an unknown encoding, frame or dtype, a radius outside 1..10 with EGO, a
 * stack outside 1..8, a scale or bias that is not finite, U8 with scale != 1 or bias != 0, a data not aligned to its
 * element size (or records not aligned as above), a restart_stride < 1 with a restart, more than 2^31 - 1 blocks;
 * IGW_VOX_ERR_HIP if the launch failed.  Arguments are checked before anything is launched.
 */
int igw_vox_obs(const void* agent, const void* aux, int32_t n, const igw_vox_spec* spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif
