/*
 * igw_peek.h -- C ABI of the peek query of the step path (libigw_peek.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (grid, occupancy, vote histogram, agent and
 * episode records, the task table) and writes only its outputs; libigw_hip.so, its sources and its build id stay what
 * they were.  Every pointer is a device pointer (or device-mapped host memory), `stream` a hipStream_t; calls are
 * asynchronous on it, never allocate and never synchronise.
 */
#ifndef IGW_PEEK_H_ABI
#define IGW_PEEK_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_PEEK_VERSION 1
#define IGW_PEEK_ACTIONS 18            /* Discrete(18): the walking action space with discretize=True */
#define IGW_PEEK_MAX_H 32              /* steps per candidate */
#define IGW_PEEK_MAX_K 4096            /* candidates per env */
#define IGW_PEEK_POSE 5                /* agentPos: x, y, z, pitch, yaw */

enum igw_peek_status {
    IGW_PEEK_OK = 0,
    IGW_PEEK_ERR_INVALID = -1,         /* bad argument */
    IGW_PEEK_ERR_HIP = -3              /* a HIP call failed (no usable device included) */
};

int igw_peek_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/peek.py: LIBRARY.source_hash) */
const char* igw_peek_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_peek_last_error(void);

/*
 * What env i (i < n) would be paid, when its episode would end, what it would build and where it would stand if it
 * played each of K sequences of H walking actions from its LIVE state -- without touching that state.
 *
 * State (include/igw.h; all 16-byte aligned, none NULL): grid [n][1104], occ [n][48], hist [n][512], aux [n] 16-byte
 * records, agent [n] 64-byte records; the task table task_target / task_start [T][1104], task_meta [T] 128-byte
 * records, task_index [T][9 * 160].
 *
 * actions: int32, 4-byte aligned, not NULL: [K][H] when per_env == 0 (every env plays the same K sequences), else
 *   [n][K][H].  1 <= K <= 4096, 1 <= H <= 32.
 *
 * Candidate (i, k) starts from what env i's records hold: pose and vy, time_int_steps, the active block and the
 * inventory, step_no, prev_size, the CACHED max_int and target_size, on the env's grid and occupancy.  It plays its H
 * actions one after the other; each step is, bit for bit, what igw_step_walking (without SizeReward) would do and
 * return for that state and action: World.step's order, the 40-sample ray march, place and break with the inventory
 * refund, the sub-steps and time_int_steps, the yaw wrap, step_no + 1, Task.step_intersection -- the maximal
 * intersection is recounted only where wrong_placement != 0 and right_placement is counted from the cached value,
 * which therefore stays stale across the steps of a candidate exactly as it would across steps of the env --, done =
 * (max_int == target_size) | (step_no == max_steps), and the reward in binary64.  An action outside 0..17 is a no-op
 * (the step counts it in its statistics; nothing is counted here).  A candidate sees the blocks IT placed and broke:
 * it collides with them, stands on them, aims at them.  A candidate ends with the first step that returns done;
 * nothing after that step is simulated, a reset included.
 *
 * Outputs (NULL = not wanted; not all five):
 *   reward float32 [n][K][H], 4-byte aligned: the reward of step h cast to float32; +0.0f for every step after the
 *          candidate ended.
 *   ends   int16 [n][K], 2-byte aligned: h + 1 of the step that returned done, 0 if none of the H steps did.
 *   change int16 [n][K][H], 2-byte aligned: colour << 11 | cell for a step that changed a grid cell -- cell = 0..1088 in
 *          the numbering of `look` (igw_query.h) and of the grid rows, colour the block id now in it, 0 for a break --,
 *          -1 for a step that changed nothing and for the steps after the end.
 *   pose   float32 [n][K][5], 4-byte aligned: agentPos (x, y, z, pitch, yaw) as the observation of the last executed
 *          step shows it (the float32 casts of the binary64 pose).
 *   ret    float32 [n][K], 4-byte aligned: (float)R_H with R_0 = +0.0 and R_{h+1} = R_h + g_h * r_h over the executed
 *          steps in order, r_h the binary64 reward BEFORE its cast, g_0 = 1, g_{h+1} = g_h * gamma, every operation in
 *          binary64 with one rounding (no contraction).  gamma == 1.0: the plain return.
 *
 * right_placement_scale, wrong_placement_scale, max_steps (1..65534), select_and_place: the env's.  gamma: finite.
 *
 * Nothing but rows [0, n) of the outputs is written: no state buffer, no counter, no trajectory log.  n == 0 is a
 * no-op.  Returns IGW_PEEK_OK; IGW_PEEK_ERR_INVALID for a NULL state pointer or actions, a misaligned pointer, n < 0, K,
 * H or max_steps out of range, a gamma that is not finite, or all five outputs NULL; IGW_PEEK_ERR_HIP if the launch
 * failed.  Arguments are checked before anything is launched.
 */
int igw_peek(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux, const void* agent,
             const int8_t* task_target, const int8_t* task_start, const void* task_meta, const uint8_t* task_index,
             int32_t n, int32_t K, int32_t H, const int32_t* actions, int32_t per_env, double right_placement_scale,
             double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma, float* reward,
             int16_t* ends, int16_t* change, float* pose, float* ret, void* stream);

#ifdef __cplusplus
}
#endif
#endif
