// igw_vote.h -- the histogram vote of the query libraries (goal, peek, peek_dict, worth, relabel), one copy: the layout of
// a level block of a task's colour index (include/igw.h) and the arithmetic of the step's histogram update
// (resolve_changes of igw_kernels.hip) on a row in LDS.  The step library keeps its own: nothing moves out of
// igw_kernels.hip or igw_device.h, whose build id is stamped on every profile.  Same operations, same order.
#pragma once

#include "igw_device.h"

namespace igw {

constexpr int kLvlBytes = IGW_LEVEL_INDEX_BYTES;   // one level block of a task's colour index (include/igw.h)
constexpr int kLvlOffs = 16;                       // offs[15] behind the four rotation bounding boxes
constexpr int kLvlCells = 32;                      // cells[<= 121]: (x + 5) << 4 | (z + 5), sorted by colour class
static_assert(kLvlCells + LEVEL <= kLvlBytes && kLvlBytes % 16 == 0, "level index block layout");
static_assert(IGW_TASK_INDEX_BYTES == IGW_GRID_Y * kLvlBytes && IGW_TASK_INDEX_BYTES % 16 == 0, "task colour index layout");
static_assert(HIST_ROW * 2 == WAVE * 16, "a wavefront holds a histogram row as one dwordx4 per lane");

// class + 1 of a synthetic colour in the colour index (0: nothing in a target can match it); a colour outside -7..7
// clamps to the empty slice behind the last class (include/igw.h)
__device__ inline int class1(int c) {
    const int k = min(max(c + 7 + (int)((uint32_t)c >> 31), 0), 15);
    return c == 0 ? 0 : k;
}

// the maximum of the eight 16-bit bins a lane holds of a histogram row
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ inline int row_piece_max(const uint4& v) {
    const us2 m = __builtin_elementwise_max(
        __builtin_elementwise_max(__builtin_bit_cast(us2, v.x), __builtin_bit_cast(us2, v.y)),
        __builtin_elementwise_max(__builtin_bit_cast(us2, v.z), __builtin_bit_cast(us2, v.w)));
    return (int)max((uint32_t)m.x, (uint32_t)m.y);
}

__device__ inline int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One change's votes on a histogram row in LDS, by the whole wavefront: the target cells of the changed cell's level
// whose colour is the cell's old synthetic colour lose a vote, those of its new one gain one, per rotation and
// admissible translation.  Uniform arguments.
__device__ inline void vote_change(uint32_t* hrow, const uint8_t* index, int cell, int s0, int s1) {
    const int lane = __lane_id();
    const int q = lane & 3, mi = lane >> 2;
    const int lvl = cell / LEVEL, rem = cell - lvl * LEVEL, gx = rem / 11, gz = rem - gx * 11;
    const uint8_t* blk = index + lvl * kLvlBytes;
    const int ka = class1(s0), kb = class1(s1);
    const int oa0 = blk[kLvlOffs - 1 + ka], oa1 = blk[kLvlOffs + ka], ob0 = blk[kLvlOffs - 1 + kb], ob1 = blk[kLvlOffs + kb];
    const int na = ka != 0 ? oa1 - oa0 : 0, nv = na + (kb != 0 ? ob1 - ob0 : 0);
    const int bb = (int)reinterpret_cast<const uint32_t*>(blk)[q];
    const int xmin = (int)(int8_t)(bb & 0xff), dxlo = (int)(int8_t)((bb >> 8) & 0xff) - 10;
    const int zmin = (int)(int8_t)((bb >> 16) & 0xff), dzlo = (int)(int8_t)((bb >> 24) & 0xff) - 10;
    for (int i0 = 0; i0 < nv; i0 += WAVE / 4) {   // nv <= 2 * 121
        const int idx = i0 + mi;
        if (idx < nv) {
            const bool dec = idx < na;
            const int tc = blk[kLvlCells + (dec ? oa0 + idx : ob0 + (idx - na))];
            const int tx = tc >> 4, tz = tc & 15;
            const int bx = (q & 1) ? tz : tx, bz = (q & 1) ? tx : tz;
            const int rx = q >= 2 ? 10 - bx : bx, rz = (q == 1 || q == 2) ? 10 - bz : bz;
            const int u = rx - gx - dxlo, v = rz - gz - dzlo;
            if ((unsigned)u <= (unsigned)(xmin - dxlo) && (unsigned)v <= (unsigned)(zmin - dzlo)) {   // (extents <= 10: bins < 484)
                const int bin = q * LEVEL + u * 11 + v;
                atomicAdd(&hrow[bin >> 1], (dec ? 0xffffffffu : 1u) << (16 * (bin & 1)));
            }
        }
    }
}

}  // namespace igw
