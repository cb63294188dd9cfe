/*
 * igw_recall.h -- C ABI of the recall query of the episode log (libigw_recall.so), version 1.
 *
 * A library of its own: it reads trajectory records (include/igw.h: igw_set_trajectory_log), starting grids, reset poses
 * and goal rows and writes only its outputs; libigw_hip.so and the other libraries, their sources and their build ids
 * stay what they were.  Every pointer but the spec is a device pointer (or device-mapped host memory), `stream` a
 * hipStream_t; calls are asynchronous on it, never allocate and never synchronise.
 */
#ifndef IGW_RECALL_H_ABI
#define IGW_RECALL_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_RECALL_VERSION 1
#define IGW_RECALL_ROW 1104            /* bytes of a grid row: 1089 cells + 15 pad bytes */
#define IGW_RECALL_CELLS 1089          /* 9 * 11 * 11; cell c = y * 121 + x * 11 + z */
#define IGW_RECALL_LEVELS 9
#define IGW_RECALL_RECORD 64           /* bytes of a trajectory record (IGW_TRAJ_BYTES) */
#define IGW_RECALL_MAX_PLANES 4
#define IGW_RECALL_MAX_STACK 8
#define IGW_RECALL_MAX_RADIUS 10
#define IGW_RECALL_SPEC_BYTES 64       /* sizeof(igw_recall_spec) */

enum igw_recall_status {
    IGW_RECALL_OK = 0,
    IGW_RECALL_ERR_INVALID = -1,       /* bad argument */
    IGW_RECALL_ERR_HIP = -3            /* a HIP call failed (no usable device included) */
};
enum { IGW_RECALL_GRID = 0, IGW_RECALL_GOAL = 1 };                    /* igw_recall_plane.source */
enum { IGW_RECALL_ONEHOT = 0, IGW_RECALL_OCC = 1 };                   /* igw_recall_plane.encoding (= IGW_VOX_*) */
enum { IGW_RECALL_WORLD = 0, IGW_RECALL_EGO = 1 };                    /* igw_recall_spec.frame (= IGW_VOX_*) */
enum { IGW_RECALL_U8 = 0, IGW_RECALL_F16 = 1, IGW_RECALL_BF16 = 2, IGW_RECALL_F32 = 3 };   /* dtype (= IGW_VOX_*) */

int igw_recall_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/recall.py: LIBRARY.source_hash) */
const char* igw_recall_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_recall_last_error(void);

/*
 * One grid of colour ids per entry: IGW_RECALL_GRID is the entry's own grid (below), IGW_RECALL_GOAL the sample's goal
 * row, the same for every entry of the sample.  The channels are include/igw_vox.h's:
 *   IGW_RECALL_ONEHOT  6 channels, channel k = [v == k + 1]; a value outside 1..6 sets none
 *   IGW_RECALL_OCC     1 channel, [v != 0]
 */
typedef struct igw_recall_plane {
    int32_t source;                 /* IGW_RECALL_GRID / IGW_RECALL_GOAL */
    int32_t encoding;               /* IGW_RECALL_ONEHOT / IGW_RECALL_OCC */
} igw_recall_plane;

/*
 * The layout of one observation, igw_vox_spec's fields that make sense for a logged entry: [K][C][9][S][S] elements of
 * `dtype` per sample.  C = the planes' channels in their order, then one agent channel if agent_plane; S = 11
 * (IGW_RECALL_WORLD) or 2 * radius + 1 (IGW_RECALL_EGO).  Agent channel, frames and element are include/igw_vox.h's:
 * with the entry's pose (x, y, z, yaw) in binary64 the head cell is (rint(x) + 5, rint(y) + 1, rint(z) + 5), rint =
 * round-half-even; the channel is 1 at the head cell and the cell below it where those lie inside the grid.  WORLD:
 * plane[y][x][z].  EGO: output [y][u][w] reads world cell (y, hx + a, hz + b), s = R - u cells ahead, t = w - R cells to
 * the right, (a, b) = s * f_q + t * r_q with the heading quadrant q = floor((yaw + 45.0) / 90.0) mod 4 (binary64) and
 * f_0..3 = (0,-1), (1,0), (0,1), (-1,0), r_0..3 = (1,0), (0,1), (-1,0), (0,-1); a world cell outside the grid reads 0 in
 * every channel.  Element: b in {0, 1}; U8 stores b (scale 1, bias 0 required); F32 (float)b * scale, then + bias, two
 * f32 operations that are never fused; F16 / BF16 that f32 value rounded to nearest-even.
 * The struct is host memory, read during the call; its values reach the kernel by value.
 */
typedef struct igw_recall_spec {
    igw_recall_plane planes[IGW_RECALL_MAX_PLANES];
    int32_t          num_planes;    /* 1..4 */
    int32_t          agent_plane;   /* 0 / 1 */
    int32_t          frame;         /* IGW_RECALL_WORLD / IGW_RECALL_EGO */
    int32_t          radius;        /* R, 1..10 (EGO only) */
    int32_t          dtype;         /* IGW_RECALL_U8 / F16 / BF16 / F32 */
    int32_t          stack;         /* K, 1..8 */
    float            scale, bias;
} igw_recall_spec;

/*
 * The voxel observations before and after one logged step, for B samples (episode[b], step[b]) of E logged episodes,
 * from the log's records alone.  No env state is read or written.
 *
 * Inputs.
 *   records     [n_records][64], 4-byte aligned: trajectory records (include/igw.h).  Read: the u16 `change` at byte 40
 *               (0xffff, or cell (bits 0-10) | colour (bits 11-13)), the f32 agentPos[5] at byte 0 (x, y, z, pitch, yaw),
 *               and the whole record of the sampled step for `record`.
 *   first       int64 [E]: index of the episode's first record; length int32 [E]: its steps, clamped to 0..L (L >= 1).
 *               Episodes may share records.
 *   start_grid  int8 [E][1104], 16-byte aligned: the grid the episode started from (a cell outside 0..6 reads as 0).
 *   init_pose   f64 [E][5]: x, y, z, yaw, pitch of the reset (the order of the task table; the record swaps the angles).
 *   episode     int32 [B], step int32 [B]: sample b is step t = step[b] of episode e = episode[b], 1 <= t <= length[e].
 *   goal        NULL, or int8 rows of goal_stride >= 1089 bytes at any alignment, n_goal_rows of them: targets in the
 *               user's frame (igw_relabel's `target` output, or task_target + task_start).  Sample b reads row
 *               goal_index[b] (int64 [B]), or row e when goal_index is NULL.  Required by an IGW_RECALL_GOAL plane.
 *
 * Entries (igw_render_episodes' definition).  Entry 0 of episode e is start_grid[e] at init_pose[e].  Entry s >= 1 is
 * start_grid[e] with the changes of records first[e] .. first[e] + s - 1 applied in order (a change to a cell >= 1089 is
 * ignored; the colour is the word's three bits, 0..7) at the f32 agentPos of record first[e] + s - 1, widened to f64.
 * The log keeps float32 poses while the live state is float64: near a half-integer coordinate the two round to
 * different head cells.  The query is defined on the log's values, not as "what igw_vox_obs wrote at the time".
 *
 * Outputs (NULL = not wanted; not all NULL), indexed with 64-bit offsets; obs / next_obs need only be aligned to their
 * element size, record and valid to nothing.
 *   obs      [B][K][C][9][S][S]: slot j holds entry max(0, t - K + j)        (what a stack of K showed before step t)
 *   next_obs [B][K][C][9][S][S]: slot j holds entry max(0, t - K + 1 + j)    (... and after it)
 *   record   uint8 [B][64]: a copy of record first[e] + t - 1
 *   valid    uint8 [B]: 1, or 0 for a padding sample
 * Padding.  A sample is padding when episode[b] is outside 0..E-1, step[b] outside 1..length[e] (clamped), first[e] < 0
 * or first[e] + length[e] > n_records, or, with a goal, its row index outside 0..n_goal_rows-1.  Every element of its obs
 * and next_obs is the value of bit 0 (0, or `bias` for the float types), its record is zeros, its valid 0.
 * Nothing outside the B samples' rows is written.  B == 0 is a no-op.
 *
 * Returns IGW_RECALL_OK; IGW_RECALL_ERR_INVALID for a NULL records / first / length / start_grid / init_pose / episode /
 * step / spec, every output NULL, B, E or n_records < 0, L < 1, num_planes outside 1..4, an unknown source, encoding,
 * frame or dtype, a radius outside 1..10 with EGO, a stack outside 1..8, a scale or bias that is not finite, U8 with
 * scale != 1 or bias != 0, a goal plane without goal, a goal with goal_stride < 1089 or n_goal_rows < 0, a start_grid not
 * 16-byte, first / init_pose / goal_index not 8-byte, records / length / episode / step not 4-byte aligned, obs or
 * next_obs not aligned to its element size (more than 2^31 - 1 blocks cannot be asked for: a block is a sample);
 * IGW_RECALL_ERR_HIP if the launch failed.  Arguments are checked before anything is launched.
 */
int igw_recall(const void* records, int64_t n_records, const int64_t* first, const int32_t* length,
               const int8_t* start_grid, const double* init_pose, int32_t E, int32_t L, const int32_t* episode,
               const int32_t* step, int32_t B, const int8_t* goal, int64_t goal_stride, int64_t n_goal_rows,
               const int64_t* goal_index, const igw_recall_spec* spec, void* obs, void* next_obs, uint8_t* record,
               uint8_t* valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif
