// igw_voxel.h -- what the two voxel writers share (vox/igw_vox.hip: the live state; recall/igw_recall.hip: logged
// transitions), one copy: the element of the channel-first one-hot / occupancy planes in u8 / f16 / bf16 / f32, the frame
// a pose gives the window, and the writer of a slot.  One workgroup of 256 lanes per env or sample.
//   stage   Head cell and heading quadrant (Frame) are computed by every lane from the same pose: no exchange.  Each
//           lane walks output cells o = (y, u, w) of the S x S window, maps them to the world cell they show and leaves
//           one byte per plane in LDS, ALREADY in the output frame: for a one-hot plane 0 (empty, or outside the grid),
//           1..6 (the colour), 7 (any other non-zero value), for an occupancy plane [v != 0]; the agent's body is a
//           plane of the second kind.  A small table says which plane a channel reads and which code it compares
//           with, so every element is one byte load and one compare.  Table and loop are statements the kernels
//           include in their bodies, igw_voxel_table.h and igw_voxel_stage.h, over macros that say where a plane's
//           value is read.
//   write   A slot of C * 9 * S * S elements starts wherever the ones before it end, so it is not 16-byte aligned in
//           general.  It is cut at the ABSOLUTE 16-byte boundaries: a lane assembles a whole 16-byte piece (16 u8, 8 half,
//           4 f32 elements) from the LDS planes and stores it with one 16-byte store, so a wave instruction writes 1 KiB
//           of contiguous lines; the up to 15 bytes in front of the first boundary and behind the last go element by
//           element.
// Vector stores in plain C++ only.  Loop bounds depend on the spec only.  The constants are this file's own; each library
// asserts that its ABI's equal them.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {
namespace voxel {

constexpr int kThreads = 256;
constexpr int kLevels = 9;
constexpr int kMaxSources = 4;                                 // planes besides the agent's
constexpr int kMaxRadius = 10;
constexpr int kMaxSide = 2 * kMaxRadius + 1;
constexpr int kMaxPlane = kLevels * kMaxSide * kMaxSide;       // cells of the largest window: 3,969
constexpr int kTable = 32;                                     // >= 4 * 6 + 1 channels, and one behind the last
constexpr int kOther = 7;                                      // a non-zero value outside 1..6
constexpr int kOneHot = 0, kOcc = 1;                           // a plane's encoding
constexpr int kU8 = 0, kF16 = 1, kBF16 = 2, kF32 = 3;          // the element types

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int kDtype> struct Elem { using E = uint16_t; };
template <> struct Elem<kU8> { using E = uint8_t; };
template <> struct Elem<kF32> { using E = uint32_t; };

// b = 0 / 1 as the bits of an element: u8 as it is; the float types from (float)b * scale, then + bias (two roundings:
// the library is built with -ffp-contract=off), f16 / bf16 rounded to nearest-even from that f32.
template <int kDtype>
__device__ __forceinline__ typename Elem<kDtype>::E elem_value(uint32_t b, float scale, float bias) {
    if constexpr (kDtype == kU8) {
        return (uint8_t)b;
    } else {
        float f = (float)b * scale;
        f = f + bias;
        const uint32_t u = __float_as_uint(f);
        if constexpr (kDtype == kF32) {
            return u;
        } else if constexpr (kDtype == kF16) {
            const _Float16 h = (_Float16)f;
            return __builtin_bit_cast(uint16_t, h);
        } else {   // (scale and bias are finite, so f is no NaN unless inf - inf: kept a quiet NaN)
            if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
            return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    }
}

template <bool kNonTemporal>
__device__ __forceinline__ void store16(void* p, u32x4 v) {
    if constexpr (kNonTemporal) {
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
    } else {
        *reinterpret_cast<u32x4*>(p) = v;
    }
}

// rint(v) as an int, clamped to +-64: a centre that far out sees only cells outside the grid, as any farther one does
__device__ __forceinline__ int pose_cell(double v) {
    const double r = __builtin_rint(v);
    return (int)__builtin_fmin(__builtin_fmax(r, -64.0), 64.0);
}

// How a run of L elements at `base` is cut at the absolute 16-byte boundaries: `head` elements in front of the first,
// `pieces` whole 16-byte pieces, and the rest from `tail` on.
template <typename E> struct Cut {
    int head, pieces, tail;
    __device__ __forceinline__ Cut(const E* base, int L) {
        constexpr int P = 16 / (int)sizeof(E);
        const unsigned lead = (16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u;
        head = min(L, (int)(lead / sizeof(E)));
        pieces = (L - head) / P;
        tail = head + pieces * P;
    }
};

struct Planes {
    const uint8_t* cells;      // [kMaxSources + 1][kMaxPlane] bytes in LDS
    const uint8_t* ch_plane;   // [kTable]
    const uint8_t* ch_match;   // [kTable]: the channel is [code == it]
    int P9;                    // cells of one channel: 9 * S * S
};

// The staged planes into one slot of L elements.
template <int kDtype, bool kNonTemporal>
__device__ __forceinline__ void write_slot(typename Elem<kDtype>::E* base, int L, const Planes& pl,
                                           typename Elem<kDtype>::E v0, typename Elem<kDtype>::E v1) {
    using E = typename Elem<kDtype>::E;
    constexpr int P = 16 / (int)sizeof(E);
    const int tid = threadIdx.x;
    const Cut<E> cut(base, L);
    const int rounds = (L / P + kThreads) / kThreads;   // >= pieces / kThreads, from the spec alone
#pragma unroll 1
    for (int it = 0; it < rounds; it++) {
        const int p = tid + it * kThreads;
        if (p >= cut.pieces) continue;
        const int e0 = cut.head + p * P;
        const int ch = e0 / pl.P9, o = e0 - ch * pl.P9;
        // A piece lies in one channel or straddles two (a channel has an odd number of cells): its first `own`
        // elements are channel ch's from cell o on, the others channel ch + 1's from cell 0 on (behind the last
        // channel the table still answers, and no piece reaches there).  No branch, no carried cell counter.
        const int own = pl.P9 - o;
        const int at1 = (int)pl.ch_plane[ch] * kMaxPlane + o, at2 = (int)pl.ch_plane[ch + 1] * kMaxPlane - own;
        const uint32_t m1 = pl.ch_match[ch], m2 = pl.ch_match[ch + 1];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < P; j++) {
            const bool next = j >= own;
            const uint32_t code = pl.cells[(next ? at2 : at1) + j];
            const uint32_t e = code == (next ? m2 : m1) ? v1 : v0;
            w[j * (int)sizeof(E) / 4] |= e << (8 * ((j * (int)sizeof(E)) & 3));
        }
        store16<kNonTemporal>(base + e0, u32x4{w[0], w[1], w[2], w[3]});
    }
    const int edge = cut.head + (L - cut.tail);   // < 2 * P
    if (tid < edge) {
        const int e = tid < cut.head ? tid : cut.tail + (tid - cut.head);
        const int ch = e / pl.P9, o = e - ch * pl.P9;
        base[e] = pl.cells[(int)pl.ch_plane[ch] * kMaxPlane + o] == pl.ch_match[ch] ? v1 : v0;
    }
}

// What a pose (x, y, z, yaw) makes of the window: the head's cell and the heading quadrant's ahead and right vectors.
struct Frame {
    int hx, hy, hz, fx, fz, rx, rz;
    __device__ __forceinline__ Frame(double x, double y, double z, double yaw) {
        hx = pose_cell(x) + 5, hy = pose_cell(y) + 1, hz = pose_cell(z) + 5;
        const double f = __builtin_floor((yaw + 45.0) / 90.0);
        const int q = (int)(f - 4.0 * __builtin_floor(f / 4.0)) & 3;
        fx = (q == 1) - (q == 3), fz = (q == 2) - (q == 0), rx = (q == 0) - (q == 2), rz = (q == 1) - (q == 3);
    }
};

}  // namespace voxel
}  // namespace
