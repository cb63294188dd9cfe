/*
 * igw_aim.h -- C ABI of the aim query of the step path (libigw_aim.so), version 1.
 *
 * A library of its own: it reads the state buffers of include/igw.h (agent records, occupancy rows) and writes only
 * its outputs; libigw_hip.so, its sources and its build id stay what they were.  Every pointer is a device pointer
 * (or device-mapped host memory), `stream` a hipStream_t; calls are asynchronous on it, never allocate and never
 * synchronise.
 */
#ifndef IGW_AIM_H_ABI
#define IGW_AIM_H_ABI

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGW_AIM_VERSION 1
#define IGW_AIM_ROW 1104               /* int32 words per env and plane: 1089 cells + 15 pad words (written as -1) */
#define IGW_AIM_CELLS 1089             /* 9 x 11 x 11 */
#define IGW_AIM_MAX_TURNS 72           /* 36 yaw steps + 36 pitch steps */

enum igw_aim_status {
    IGW_AIM_OK = 0,
    IGW_AIM_ERR_INVALID = -1,          /* bad argument */
    IGW_AIM_ERR_HIP = -3               /* a HIP call failed (no usable device included) */
};

int igw_aim_version(void);
/* sha256 prefix of this library's sources and flags (gridworld_amd/aim.py: LIBRARY.source_hash) */
const char* igw_aim_build_id(void);
/* the message of the calling thread's last failed call */
const char* igw_aim_last_error(void);

/*
 * Which grid cells a place or a break can reach from the LIVE state of env i (i < n) by turning the camera alone, and
 * the cheapest turn that gets there.
 *
 * Directions.  (di, dj), di = -36..35, dj = -36..36, names the rotation yaw_d = yaw + 5.0 * di, pitch_d = pitch +
 * 5.0 * dj (binary64, one exact product and one add, no contraction).  A direction whose pitch_d lies outside
 * [-90, 90] does not exist: move_camera clamps the pitch, so no action sequence reaches it.  Its cost is turns =
 * |di| + |dj|; only directions with turns <= max_turns (0..72) are evaluated.
 *
 * What a direction is asked: what the step's place_or_remove_block would do from the agent's current position with
 * that rotation, in the step's own arithmetic -- the sight vector of get_sight_vector (the step's sincos over the same
 * table), the 40-sample hit_test recurrence, normalize:
 *   break cell   the block hit, if it is not the ground (y != -2);
 *   place cell   `previous`, if there is one, it lies in the build zone and the agent does not overlap it (the
 *                predicate of igw_action_mask's can_place without the inventory).
 * Inventory and the active block are NOT looked at: igw_action_mask and the inventory observation say that.
 *
 * agent: [n] 64-byte agent records, 16-byte aligned; occ: [n][48] occupancy words, 16-byte aligned (include/igw.h).
 * place, brk: int32 [n][1104], 16-byte aligned; either may be NULL (not wanted), not both.  Word c < 1089 of a row
 *   belongs to grid cell c = (y + 1) * 121 + (x + 5) * 11 + (z + 5) (the numbering of `look` in igw_query.h and of
 *   the grid rows); words 1089..1103 are written as -1.
 *   place[i][c] = the smallest code, compared as an unsigned integer, of a direction whose place cell is c, or -1 if
 *   there is none; brk[i][c] the same for break cells.
 *     code = turns << 16 | (dj + 36) << 8 | (di + 36)
 *   so among directions of equal cost the lowest dj wins, then the lowest di.
 *
 * What the answer means.  Where yaw and pitch are integer multiples of 5, every yaw_d and pitch_d equals what |di| and
 * |dj| successive camera actions produce: everything Discrete(18) reaches from a pose on that lattice.  For an agent
 * whose position does not change over those steps, playing the turns (action 12 while di < 0, 13 while di > 0, 14
 * while dj < 0, 15 while dj > 0) and then action 16 or 17 touches exactly the cell named, inventory permitting.  For an
 * agent in motion (falling, or pushed out of a block) the answer is for the position it has now.
 *
 * Nothing but place[0 .. n) and brk[0 .. n) is written.  n == 0 is a no-op.
 * Returns IGW_AIM_OK; IGW_AIM_ERR_INVALID for a NULL agent or occ, place and brk both NULL, a negative n, a
 * max_turns outside 0..72 or a misaligned pointer; IGW_AIM_ERR_HIP if the launch failed.
 */
int igw_aim(const void* agent, const uint32_t* occ, int32_t n, int32_t max_turns, int32_t* place, int32_t* brk,
            void* stream);

#ifdef __cplusplus
}
#endif
#endif
