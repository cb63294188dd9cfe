/*
 * igw_query.h -- C ABI of the state queries of the step path (libigw_query.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (agent records, occupancy rows) and writes only
 * its outputs; libigw_hip.so, its sources and its build id stay what they were.  Every pointer is a device pointer
 * (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on it, never allocate and never
 * synchronise.
 */
#ifndef IGW_QUERY_H_ABI
#define IGW_QUERY_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_QUERY_VERSION 1
#define IGW_QUERY_ACTIONS 18           /* Discrete(18): the walking action space with discretize=True */

enum igw_query_status {
    IGW_QUERY_OK = 0,
    IGW_QUERY_ERR_INVALID = -1,        /* bad argument */
    IGW_QUERY_ERR_HIP = -3             /* a HIP call failed (no usable device included) */
};

int igw_query_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/query.py: LIBRARY.source_hash) */
const char* igw_query_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_query_last_error(void);

/*
 * Which of the 18 walking actions would act on the LIVE state of env i (i < n): mask[i][a] = 1 or 0.
 *   a = 0 (no-op), 1..4 (moves), 12, 13 (yaw)    1 (collisions are not evaluated)
 *   a = 5 (jump)                                 agent.dy == 0.0
 *   a = 6..11 (hotbar k = a - 5)                 select_and_place != 0: can_place(k); else active_block != k
 *   a = 14 / 15 (pitch down / up by 5)           pitch > -90 / pitch < 90
 *   a = 16 (break)                               the sight ray hits a block that is not the ground
 *   a = 17 (place)                               can_place(active_block)
 * can_place(c): the sight ray (40 samples, 8 units, from the current position along the current rotation -- the ray
 * the next step marches, because no Discrete(18) action turns the camera and places) hits and has a `previous`
 * cell, inventory[c - 1] > 0, `previous` is inside the build zone and the agent does not stand in it: the predicate
 * of the step's place_or_remove_block, evaluated with the step's own arithmetic.
 *
 * agent: [n] 64-byte agent records, 16-byte aligned; occ: [n][48] occupancy words, 16-byte aligned (include/igw.h).
 * mask:  uint8 [n][18].
 * look (NULL = not wanted): int16 [n][2], 2-byte aligned: {break_cell, place_cell}, the grid cell
 *   (y + 1) * 121 + (x + 5) * 11 + (z + 5) action 16 would clear / action 17 would fill, -1 if it would do nothing.
 * actions (NULL = not wanted): int32 [n], 4-byte aligned: one action drawn uniformly from the set bits of mask[i]
 *   (bit 0 is always set): with e = env_offset + i, h = splitmix64(seed ^ splitmix64(e * 0x9E3779B1 + t *
 *   0x100000001B3 + 0x6d61736b)) in 64-bit wrapping arithmetic (splitmix64: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 *   0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), r = h >> 32, k = (r * popcount(mask[i]))
 *   >> 32, and the action is the k-th set bit of mask[i], counted from action 0.
 * Nothing but mask[0 .. n), look[0 .. n) and actions[0 .. n) is written.  n == 0 is a no-op.
 * Returns IGW_QUERY_OK; IGW_QUERY_ERR_INVALID for a NULL agent, occ or mask, a negative n or a misaligned pointer;
 * IGW_QUERY_ERR_HIP if the launch failed.
 */
int igw_action_mask(const void* agent, const uint32_t* occ, int32_t n, int32_t select_and_place, uint8_t* mask,
                    int16_t* look, int32_t* actions, uint64_t seed, uint64_t t, int64_t env_offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif
