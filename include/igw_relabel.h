/*
 * igw_relabel.h -- C ABI of the relabel query of the episode log (libigw_relabel.so), version 1.
 *
 * A library of its own: it reads trajectory records (include/igw.h: igw_set_trajectory_log), starting grids and
 * candidate targets and writes only its outputs; libigw_hip.so, its sources and its build id stay what they were.
 * Every pointer is a device pointer (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on
 * it, never allocate and never synchronise.
 */
#ifndef IGW_RELABEL_H_ABI
#define IGW_RELABEL_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_RELABEL_VERSION 1
#define IGW_RELABEL_ROW 1104           /* bytes of a grid row: 1089 cells + 15 pad bytes */
#define IGW_RELABEL_CELLS 1089         /* 9 x 11 x 11 */
#define IGW_RELABEL_RECORD 64          /* bytes of a trajectory record (IGW_TRAJ_BYTES) */
#define IGW_RELABEL_MAX_G 256          /* goals per episode */

enum igw_relabel_status {
    IGW_RELABEL_OK = 0,
    IGW_RELABEL_ERR_INVALID = -1,      /* bad argument */
    IGW_RELABEL_ERR_HIP = -3           /* a HIP call failed (no usable device included) */
};

int igw_relabel_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/relabel.py: LIBRARY.source_hash) */
const char* igw_relabel_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_relabel_last_error(void);

/*
 * Hindsight relabelling: what the step (without SizeReward) would have returned on every step of E logged episodes had
 * the target of episode e been goal g (g < G), from the log's `change` words alone.  No env state is read or written.
 *
 * Inputs.
 *   records     [n_records][64]: trajectory records (include/igw.h); only the u16 `change` at byte 40 of a record is
 *               read: 0xffff, or cell (bits 0-10) | colour (bits 11-13).  4-byte aligned.
 *   first       int64 [E]: index of the episode's first record; length int32 [E]: its steps, clamped to 0..L.  An
 *               episode with first < 0 or first + length > n_records is out of the buffer: every one of its outputs is
 *               written as padding (zeros).  Episodes may share records.
 *   start_grid  int8 [E][1104], 16-byte aligned: the grid the episode started from (a cell outside 0..6 reads as 0, as
 *               in the task table).
 *   Exactly one of
 *   targets     int8 [E][G][1104], 16-byte aligned: USER targets (a cell outside 0..7 reads as 0); or
 *   at          int32 [E][G]: goal g is the episode's own grid at entry at[e][g], clamped to 0..length[e]; entry 0 is
 *               the starting grid, entry t the grid after step t.
 *
 * Semantics.  grid_t is the starting grid with the changes of records first .. first + t - 1 applied in order (a change
 * to a cell >= 1089 is ignored).  Pair (e, g) is scored as by a fresh synthetic Task(target - start), always invariant,
 * fed grid_t - start for t = 1 .. length (tasks/task.py:103-119, env.py:290-296): with size_t the non-zero cells of
 * grid_t - start, size_0 := 0 and the cached max_int_0 := 0,
 *   wrong = size_(t-1) - size_t                        (size_(-) of step 1 is 0: a starting grid counts for nothing)
 *   max_int_t = wrong != 0 ? maximal_intersection(grid_t - start) : max_int_(t-1)     (a cell recoloured in place
 *               leaves the cache stale, as the step's `dirty` bit does)
 *   right = max_int_t - max_int_(t-1)
 *   done = (max_int_t == target_size) | (t == max_steps)
 *   reward = (float)(right == 0 ? wrong * wrong_placement_scale : right * right_placement_scale)     (binary64)
 * Scoring goes on after a done step, as the reference does when stepped on.
 *
 * Outputs (NULL = not wanted; not all NULL), indexed with 64-bit offsets:
 *   reward float32 [E][G][L], done uint8 [E][G][L], progress int16 [E][G][L] (max_int_t): +0 from step length[e] on
 *   end    int32 [E][G]: t of the first done step, 0 without one
 *   ret    float32 [E][G]: ret = ret + g * reward_t; g = g * gamma in binary64 (g = 1 at t = 1), one rounding per
 *          operation, over t = 1 .. end, or 1 .. length when end == 0 (the recurrence of igw_peek.h)
 *   target_size int16 [E][G]: non-zero cells of target - start
 *   target int8 [E][G][1104], 16-byte aligned: the goal grid that was used (with `at`: the rebuilt grid), pad bytes 0
 *
 * E == 0 is a no-op.  Returns IGW_RELABEL_OK; IGW_RELABEL_ERR_INVALID for a NULL records / first / length / start_grid,
 * targets and at both NULL or both given, every output NULL, a misaligned pointer, E < 0, n_records < 0, G outside
 * 1..256, L < 1, E * G * L >= 2^40, max_steps outside 1..65534, a gamma that is not finite; IGW_RELABEL_ERR_HIP if
 * the launch failed.  Arguments are checked before anything is launched.
 */
int igw_relabel(const void* records, int64_t n_records, const int64_t* first, const int32_t* length,
                const int8_t* start_grid, const int8_t* targets, const int32_t* at, int32_t E, int32_t G, int32_t L,
                double right_placement_scale, double wrong_placement_scale, int32_t max_steps, double gamma,
                float* reward, uint8_t* done, int16_t* progress, int32_t* end, float* ret, int16_t* target_size,
                int8_t* target, void* stream);

#ifdef __cplusplus
}
#endif
#endif
