/*
 * igw_peek_dict.h -- C ABI of the peek query for the flying and the walking Dict action spaces (libigw_peek_dict.so),
 * version 1.
 *
 * A library of its own beside libigw_peek.so (include/igw_peek.h, the Discrete(18) space): it reads the state buffers
 * of include/igw.h (grid, occupancy, vote histogram, agent and episode records, the task table) and writes only its
 * outputs; libigw_hip.so and libigw_peek.so, their sources and their build ids stay what they were.  Every pointer is a
 * device pointer (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on it, never allocate
 * and never synchronise.
 *
 * Two entry points, one per action space, so that every action argument keeps the type and the layout its step entry
 * gives it (igw_step_flying, igw_step_walking_dict); the state, the scalars, the outputs, the limits and the status
 * codes are igw_peek's (IGW_PEEK_OK, IGW_PEEK_ERR_INVALID, IGW_PEEK_ERR_HIP of include/igw_peek.h).
 */
#ifndef IGW_PEEK_DICT_H_ABI
#define IGW_PEEK_DICT_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_PEEK_DICT_VERSION 1
#define IGW_PEEK_DICT_MAX_H 32         /* steps per candidate (IGW_PEEK_MAX_H) */
#define IGW_PEEK_DICT_MAX_K 4096       /* candidates per env (IGW_PEEK_MAX_K) */
#define IGW_PEEK_DICT_POSE 5           /* agentPos: x, y, z, pitch, yaw */
#define IGW_PEEK_DICT_BUTTONS 8        /* forward, back, left, right, jump, attack, use, hotbar */

int igw_peek_dict_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/peek_dict.py: LIBRARY.source_hash) */
const char* igw_peek_dict_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_peek_dict_last_error(void);

/*
 * What env i (i < n) would be paid, when its episode would end, what it would build and where it would stand if it
 * played each of K sequences of H actions of its space from its LIVE state -- without touching that state.
 *
 * State (include/igw.h; all 16-byte aligned, none NULL): grid [n][1104], occ [n][48], hist [n][512], aux [n] 16-byte
 * records, agent [n] 64-byte records; the task table task_target / task_start [T][1104], task_meta [T] 128-byte
 * records, task_index [T][9 * 160].
 *
 * Actions, none NULL, in the step's own layouts behind a leading [K][H] when per_env == 0 (every env plays the same K
 * sequences), else [n][K][H]; 1 <= K <= 4096, 1 <= H <= 32:
 *   igw_peek_flying        movement float32 [..][3] (strafe forward / back, strafe left / right, up / down), camera
 *                          float32 [..][2] (yaw, pitch deltas in degrees), inventory int32 [..] (0: no hotbar change,
 *                          1..6: that block), placement int32 [..] (0: nothing, 1: place, 2: break); all 4-byte aligned.
 *   igw_peek_walking_dict  buttons uint8 [..][8] (forward, back, left, right, jump, attack, use: pressed when not 0;
 *                          hotbar 0..6), 8-byte aligned as for igw_step_walking_dict; camera float32 [..][2], 4-byte
 *                          aligned.
 *
 * Candidate (i, k) starts from what env i's records hold: pose and vy, time_int_steps, the active block and the
 * inventory, step_no, prev_size, the CACHED max_int and target_size, on the env's grid and occupancy.  It plays its H
 * actions one after the other; each step is, bit for bit, what igw_step_flying / igw_step_walking_dict (without
 * SizeReward) would do and return for that state and action: the action parsing (inventory == 0 or hotbar == 0: the
 * active block stays; with select_and_place a hotbar change places and cancels a break), World.step's order, the pitch
 * clamp, the general double-double sin / cos / atan2 of the sight vector and of the motion vector (the walking Dict
 * space takes the table on the 5-degree lattice, as its step does), the 40-sample ray march, place and break with the
 * inventory refund, flying's vy rules and its padded-zone gate (a sub-step whose candidate position lies outside the
 * padded zone does not move a flying agent), the sub-steps and time_int_steps, the strict yaw wrap at the END of the
 * step on any float yaw, step_no + 1, Task.step_intersection -- the maximal intersection is recounted only where
 * wrong_placement != 0 and right_placement is counted from the cached value, which therefore stays stale across the
 * steps of a candidate exactly as it would across steps of the env --, done = (max_int == target_size) | (step_no ==
 * max_steps), and the reward in binary64.  A candidate sees the blocks IT placed and broke: it collides with them,
 * stands on them, aims at them.  A candidate ends with the first step that returns done; nothing after that step is
 * simulated, a reset included.
 *
 * Invalid actions.  The step runs the offending COMPONENT of an action as a no-op, runs the others as they are, and
 * counts the env-step (IGW_STAT_BAD_ACTION) for every kind below but the last, which it runs as 0 without counting; a
 * candidate step does exactly the same and counts nothing:
 *   a movement component that is not finite                          that component = 0.0
 *   a camera component that is not finite or beyond +-IGW_CAMERA_MAX that component = 0.0
 *   inventory outside 0..6, a hotbar byte above 6                    0: the active block stays, and with
 *                                                                    select_and_place nothing is placed for it
 *   placement outside 0..2                                           neither place nor break (as 0)
 *
 * Outputs (NULL = not wanted; not all five), exactly igw_peek's:
 *   reward float32 [n][K][H], 4-byte aligned: the reward of step h cast to float32; +0.0f for every step after the
 *          candidate ended.
 *   ends   int16 [n][K], 2-byte aligned: h + 1 of the step that returned done, 0 if none of the H steps did.
 *   change int16 [n][K][H], 2-byte aligned: colour << 11 | cell for a step that changed a grid cell -- cell = 0..1088 in
 *          the numbering of the grid rows, colour the block id now in it, 0 for a break --, -1 for a step that changed
 *          nothing and for the steps after the end.
 *   pose   float32 [n][K][5], 4-byte aligned: agentPos (x, y, z, pitch, yaw) as the observation of the last executed
 *          step shows it (the float32 casts of the binary64 pose).
 *   ret    float32 [n][K], 4-byte aligned: (float)R_H with R_0 = +0.0 and R_{h+1} = R_h + g_h * r_h over the executed
 *          steps in order, r_h the binary64 reward BEFORE its cast, g_0 = 1, g_{h+1} = g_h * gamma, every operation in
 *          binary64 with one rounding (no contraction).  gamma == 1.0: the plain return.
 *
 * right_placement_scale, wrong_placement_scale, max_steps (1..65534), select_and_place: the env's.  gamma: finite.
 *
 * Nothing but rows [0, n) of the outputs is written: no state buffer, no counter, no trajectory log.  n == 0 is a
 * no-op.  Returns IGW_PEEK_OK (0); IGW_PEEK_ERR_INVALID (-1) for a NULL state pointer or action pointer, a misaligned
 * pointer, n < 0, K, H or max_steps out of range, a gamma that is not finite, or all five outputs NULL;
 * IGW_PEEK_ERR_HIP (-3) if the launch failed.  Arguments are checked before anything is launched.
 */
int igw_peek_flying(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux, const void* agent,
                    const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                    const uint8_t* task_index, int32_t n, int32_t K, int32_t H, const float* movement,
                    const float* camera, const int32_t* inventory, const int32_t* placement, int32_t per_env,
                    double right_placement_scale, double wrong_placement_scale, int32_t max_steps,
                    int32_t select_and_place, double gamma, float* reward, int16_t* ends, int16_t* change, float* pose,
                    float* ret, void* stream);

int igw_peek_walking_dict(const int8_t* grid, const uint32_t* occ, const uint16_t* hist, const void* aux,
                          const void* agent, const int8_t* task_target, const int8_t* task_start, const void* task_meta,
                          const uint8_t* task_index, int32_t n, int32_t K, int32_t H, const uint8_t* buttons,
                          const float* camera, int32_t per_env, double right_placement_scale,
                          double wrong_placement_scale, int32_t max_steps, int32_t select_and_place, double gamma,
                          float* reward, int16_t* ends, int16_t* change, float* pose, float* ret, void* stream);

#ifdef __cplusplus
}
#endif
#endif
