/*
 * igw_worth.h -- C ABI of the worth query of the step path (libigw_worth.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (grid, vote histogram, agent and episode records,
 * the task table) and writes only its outputs; libigw_hip.so, its sources and its build id stay what they were.
 * Every pointer is a device pointer (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on
 * it, never allocate and never synchronise.
 */
#ifndef IGW_WORTH_H_ABI
#define IGW_WORTH_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_WORTH_VERSION 1
#define IGW_WORTH_PLANES 7             /* plane 0: break the cell; planes 1..6: place colour 1..6 in it */
#define IGW_WORTH_ROW 1104             /* int16 words per env and plane: 1089 cells + 15 pad words (written as -1) */
#define IGW_WORTH_CELLS 1089           /* 9 x 11 x 11 */

enum igw_worth_status {
    IGW_WORTH_OK = 0,
    IGW_WORTH_ERR_INVALID = -1,        /* bad argument */
    IGW_WORTH_ERR_HIP = -3             /* a HIP call failed (no usable device included) */
};

int igw_worth_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/worth.py: LIBRARY.source_hash) */
const char* igw_worth_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_worth_last_error(void);

/*
 * What the step (without SizeReward) would pay for every single-cell edit of the LIVE state of env i (i < n).
 * S = grid - start is the env's synthetic grid, `cached` the episode record's max_int, M the maximum of the env's
 * histogram row (the live maximal intersection), target_size the episode record's.
 *
 * State (include/igw.h; all 16-byte aligned, none NULL): grid [n][1104], hist [n][512], aux [n] 16-byte records, agent
 * [n] 64-byte records; the task table task_target / task_start [T][1104], task_meta [T] 128-byte records, task_index
 * [T][9 * 160].  The histogram row is current whenever a query can run (include/igw_goal.h).
 *
 * Edits.  Plane 0, cell c: break the block in c; valid where grid[c] != 0.  Plane k = 1..6, cell c: place colour k in
 * c; valid where grid[c] == 0.  Nothing else gates validity: not the inventory, not adjacency, not the agent's overlap,
 * not reach (igw_aim and igw_action_mask say whether the agent can make the edit).  An edit takes the cell's synthetic
 * value from s0 to s1: a break from grid - start to -start, a place from -start to k - start.
 *   wrong = [s0 != 0] - [s1 != 0];
 *   m'    = wrong != 0 ? the maximum over the row with the cell's votes for s0 removed and those for s1 added : cached;
 *   right = m' - cached   (the CACHED value: a cache that lags the live maximum is reproduced, as by igw_goal's gain);
 *   ends  = (m' == target_size) | (step_no + 1 == max_steps).
 *
 * Outputs (NULL = not wanted; not both NULL):
 *   word int16 [n][7][1104], 16-byte aligned: per plane a row in the layout of `grid` (cell c = y * 121 + x * 11 + z):
 *       bits 0..11   right, 12-bit two's complement (|right| <= 1089)
 *       bits 12..13  wrong + 1
 *       bit  14      ends
 *       bit  15      0
 *     -1 for an invalid edit and in the 15 pad words of every row.
 *   best int32 [n][4], 16-byte aligned: (plane, cell, word, candidates): the candidate edit with the highest reward
 *     right != 0 ? right * right_scale : wrong * wrong_scale  (binary64, compared as binary64; ties go to the lowest
 *     plane, then to the lowest cell), its word, and the number of candidates; (-1, -1, -1, 0) without one.
 *     Candidates are the valid edits that pass two gates, neither of which changes `word`:
 *       allow   uint8 [n][2][1104], 16-byte aligned, or NULL: a break of cell c is a candidate where
 *               allow[i][0][c] != 0, a place into it where allow[i][1][c] != 0;
 *       stocked != 0: the place planes k whose inventory (agent record, inv[k - 1]) is <= 0 are left out.
 *
 * Nothing but rows [0, n) of the outputs is written.  n == 0 is a no-op.
 * Returns IGW_WORTH_OK; IGW_WORTH_ERR_INVALID for a NULL state pointer, word and best both NULL, a negative n, a
 * misaligned pointer, max_steps outside 1..65534; IGW_WORTH_ERR_HIP if the launch failed.  Arguments are checked
 * before anything is launched.
 */
int igw_worth(const int8_t* grid, const uint16_t* hist, const void* aux, const void* agent, const int8_t* task_target,
              const int8_t* task_start, const void* task_meta, const uint8_t* task_index, int32_t n, int32_t max_steps,
              const uint8_t* allow, int32_t stocked, double right_scale, double wrong_scale, int16_t* word,
              int32_t* best, void* stream);

#ifdef __cplusplus
}
#endif
#endif
