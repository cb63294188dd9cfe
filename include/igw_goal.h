/*
 * igw_goal.h -- C ABI of the goal query of the step path (libigw_goal.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (grid, vote histogram, agent and episode records,
 * the task table) and writes only its outputs; libigw_hip.so, its sources and its build id stay what they were.
 * Every pointer is a device pointer (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on
 * it, never allocate and never synchronise.
 */
#ifndef IGW_GOAL_H_ABI
#define IGW_GOAL_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_GOAL_VERSION 1
#define IGW_GOAL_ACTIONS 18            /* Discrete(18): the walking action space with discretize=True */

enum igw_goal_status {
    IGW_GOAL_OK = 0,
    IGW_GOAL_ERR_INVALID = -1,         /* bad argument */
    IGW_GOAL_ERR_HIP = -3              /* a HIP call failed (no usable device included) */
};

int igw_goal_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/goal.py: LIBRARY.source_hash) */
const char* igw_goal_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_goal_last_error(void);

/*
 * Where the reward wants the target, what is left of it, and what each action would earn, for the LIVE state of env i
 * (i < n).  S = grid - start is the env's synthetic grid, T_r rotation r of its synthetic target task_target[aux.task]
 * (rotation r sends target cell (x, z) to (x, z), (z, 10 - x), (10 - x, 10 - z), (10 - z, x)).
 *
 * State (include/igw.h; all 16-byte aligned, none NULL): grid [n][1104], hist [n][512], aux [n] 16-byte records, agent
 * [n] 64-byte records; the task table task_target / task_start [T][1104], task_meta [T] 128-byte records, task_index
 * [T][9 * 160].  The histogram row is the state the answers are read from: it is current whenever a query can run,
 * because every kernel that changes a cell of `grid` updates the row in the same launch and every reset zeroes it.
 *
 * Outputs (NULL = not wanted):
 *   align int8 [n][4], 4-byte aligned: (dx, dz, rot, 0) = Task.argmax_intersection(S): the first strict maximum in
 *     (rot, dx, dz) order -- the lowest bin of the row that holds its maximum -- or (0, 0, 0) where nothing matches.
 *   fit   int16 [n][4], 8-byte aligned: (max_int, target_size, size, cached_max_int): the row maximum; the target's
 *     blocks; nnz(S) (the episode record's prev_size, which every step keeps equal to it); the episode record's
 *     max_int, the value the next step's reward is counted from (it lags max_int after a change that left nnz(S) as
 *     it was, as the reference's cache does).
 *   want  int8 [n][1104], 16-byte aligned: the aligned target in the grid's frame and layout:
 *     want[y][x][z] = T_rot[y][x + dx][z + dz] where both indices are in 0..10, else 0.
 *   todo  int8 [n][1104], 16-byte aligned: want where want != S, else 0.  The 15 pad bytes of both rows are 0.
 *   gain  float32 [n][18], 4-byte aligned, and ends uint8 [n][18]: the reward and the done flag that the step
 *     (igw_step_walking without SizeReward) would return for each action.  They need
 *       mask uint8 [n][18] and look int16 [n][2] (2-byte aligned) as igw_action_mask (include/igw_query.h) wrote them
 *       for the same state, right_placement_scale, wrong_placement_scale, max_steps, select_and_place of the env.
 *     An action with mask 0, or one that never changes the grid (all but 6..11, 16, 17; the hotbar actions too when
 *     select_and_place == 0): gain = 0 * wrong_placement_scale, ends = (cached_max_int == target_size) |
 *     (step_no + 1 == max_steps).  Otherwise the action changes one cell -- look[1] with colour a - 5 (hotbar) or
 *     active_block (17), look[0] emptied (16) -- from synthetic value s0 to s1; wrong = [s0 != 0] - [s1 != 0]; if
 *     wrong != 0, m' = the row maximum with the cell's votes for s0 removed and those for s1 added, else m' =
 *     cached_max_int; right = m' - cached_max_int; gain = (float)(right != 0 ? right * right_placement_scale : wrong *
 *     wrong_placement_scale) in binary64; ends = (m' == target_size) | (step_no + 1 == max_steps).
 *     igw_action_mask names the place cell only where the ACTIVE colour can be placed.  Where a hotbar action's mask
 *     bit is set and look[1] is -1 (the active colour's inventory is empty, another colour's is not) the cell is
 *     unknown: gain is NaN and ends the unchanged-grid value.  A caller that wants those too passes the `look` of a
 *     second igw_action_mask launch over a copy of the agent records with a full inventory (gridworld_amd/goal.py
 *     does): the place cell does not depend on the inventory.
 * The query marches no ray.  With align and fit alone it reads 1 KB of histogram, the episode record and 16 bytes of
 * task metadata per env: no grid, target or start row.  want / todo add the target row, the grid row and -- where the
 * task has a starting grid -- the start row; they never read task_index.  gain / ends add the agent record, mask, look
 * and per acting action one level block of task_index and at most two bytes of grid / start.
 * Nothing but the outputs' rows [0, n) is written.  n == 0 is a no-op.
 * Returns IGW_GOAL_OK; IGW_GOAL_ERR_INVALID for a NULL state pointer, a negative n, a misaligned pointer, gain or
 * ends without mask and look, max_steps outside 1..65534; IGW_GOAL_ERR_HIP if the launch failed.  Arguments are
 * checked before anything is launched.
 */
int igw_goal(const int8_t* grid, const uint16_t* hist, const void* aux, const void* agent, const int8_t* task_target,
             const int8_t* task_start, const void* task_meta, const uint8_t* task_index, int32_t n,
             double right_placement_scale, double wrong_placement_scale, int32_t max_steps, int32_t select_and_place,
             const uint8_t* mask, const int16_t* look, int8_t* align, int16_t* fit, int8_t* want, int8_t* todo,
             float* gain, uint8_t* ends, void* stream);

#ifdef __cplusplus
}
#endif
#endif
