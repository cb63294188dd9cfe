// igw_render_obs_stage.h -- the observation stage of igw_render_pov_obs (include/igw_render_obs.h: igw_render_obs): the chunk's
// colours, staged in LDS by render_frame() (igw_render_frame.h), leave as the channel-first, optionally grey, scaled
// and stacked observation a policy network reads.  The contract is DESIGN.md section 8, "Training-layout observations".
//
// Every thread owns pixels of the chunk and walks their (slot, plane) positions itself: the in-place shift of the
// stack reads slot k + 1 and writes slot k of the same pixels from the same thread, so the stage needs no barrier of
// its own.  Consecutive lanes hold consecutive pixels (groups of four where every row of the stack is aligned for
// it), so each plane row leaves as one coalesced run of 4-byte (u8), 8-byte (f16 / bf16) or 16-byte (f32) stores.
#ifndef IGW_RENDER_OBS_STAGE_H
#define IGW_RENDER_OBS_STAGE_H

#include "igw_render_frame.h"
#include "../../../include/igw_render_obs.h"

namespace {

constexpr int kMaxStack = IGW_RENDER_MAX_STACK;

// `N` consecutive elements of type E as the one value a lane loads and stores (native vectors: they stay in registers).
typedef uint32_t obs_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t obs_u32x4 __attribute__((ext_vector_type(4)));
template <typename E, int N> struct ObsLane { using V = E; static __device__ __forceinline__ V make(const E* e) { return e[0]; } };
template <> struct ObsLane<uint8_t, 4> {
    using V = uint32_t;
    static __device__ __forceinline__ V make(const uint8_t* e) {
        return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    }
};
template <> struct ObsLane<uint16_t, 4> {
    using V = obs_u32x2;
    static __device__ __forceinline__ V make(const uint16_t* e) {
        return V{(uint32_t)e[0] | (uint32_t)e[1] << 16, (uint32_t)e[2] | (uint32_t)e[3] << 16};
    }
};
template <> struct ObsLane<uint32_t, 4> {
    using V = obs_u32x4;
    static __device__ __forceinline__ V make(const uint32_t* e) { return V{e[0], e[1], e[2], e[3]}; }
};

// The element of each dtype as its bits, and the value v = 0..255 in it: u8 as it is; the float types from
// (float)v * scale, then + bias (two roundings: the library is built with -ffp-contract=off), f16 / bf16 rounded to
// nearest-even from that f32.
template <int kDtype> struct ObsElem { using E = uint16_t; };
template <> struct ObsElem<IGW_OBS_U8> { using E = uint8_t; };
template <> struct ObsElem<IGW_OBS_F32> { using E = uint32_t; };

template <int kDtype>
__device__ __forceinline__ typename ObsElem<kDtype>::E obs_value(uint32_t v, float scale, float bias) {
    if constexpr (kDtype == IGW_OBS_U8) {
        return (uint8_t)v;
    } else {
        float f = (float)v * scale;
        f = f + bias;
        const uint32_t b = __float_as_uint(f);
        if constexpr (kDtype == IGW_OBS_F32) {
            return b;
        } else if constexpr (kDtype == IGW_OBS_F16) {
            const _Float16 h = (_Float16)f;
            return __builtin_bit_cast(uint16_t, h);
        } else {
            if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
            return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
        }
    }
}

// What the kernel receives of an igw_render_obs, by value.
struct ObsOut {
    void* data;
    const uint8_t* restart;
    int64_t restart_stride;
    float scale, bias;
    int dtype, gray, stack, fill;

    // kN = 4 or 1 consecutive pixels from q of the chunk: their planes into every slot (`all`) or shifted into the
    // stack; p is slot 0, plane 0 of pixel q.
    template <int kDtype, int kN>
    __device__ __forceinline__ void lane(const uint8_t* stage, typename ObsElem<kDtype>::E* p, int q, bool all,
                                         int64_t plane, int64_t slot) const {
        using E = typename ObsElem<kDtype>::E;
        using V = typename ObsLane<E, kN>::V;
        uint32_t rgb[kN];   // R | G << 8 | B << 16 of each pixel, from the 3-byte staging
        bool packed = false;
        if constexpr (kN == 4) {
            if ((q & 3) == 0) {   // 12 staged bytes at a 4-byte boundary: three LDS words
                const uint32_t* s = reinterpret_cast<const uint32_t*>(stage + 3 * q);
                const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
                rgb[0] = w0 & 0xffffffu;
                rgb[1] = (w0 >> 24) | (w1 & 0xffffu) << 8;
                rgb[2] = (w1 >> 16) | (w2 & 0xffu) << 16;
                rgb[3] = w2 >> 8;
                packed = true;
            }
        }
        if (!packed) {
#pragma unroll
            for (int j = 0; j < kN; j++) {
                const uint8_t* s = stage + 3 * (q + j);
                rgb[j] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
            }
        }
        const int planes = gray ? 1 : 3, K = stack;
#pragma unroll 1
        for (int c = 0; c < planes; c++) {
            E e[kN];
#pragma unroll
            for (int j = 0; j < kN; j++) {
                const uint32_t r = rgb[j] & 255u, g = (rgb[j] >> 8) & 255u, b = rgb[j] >> 16;
                const uint32_t v = gray ? (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16 : (rgb[j] >> (8 * c)) & 255u;
                e[j] = obs_value<kDtype>(v, scale, bias);
            }
            const V nv = ObsLane<E, kN>::make(e);
            E* pc = p + c * plane;
            if (all) {
                for (int k = 0; k < K; k++, pc += slot) *reinterpret_cast<V*>(pc) = nv;
            } else {
                // every load of the shift is issued before its first store (named values, not an array: each stays
                // a register of its own)
                V o1 = nv, o2 = nv, o3 = nv, o4 = nv, o5 = nv, o6 = nv, o7 = nv;
                const E* src = pc;
#define IGW_OBS_LOAD(k) if (k < K) o##k = *reinterpret_cast<const V*>(src += slot);
                IGW_OBS_LOAD(1) IGW_OBS_LOAD(2) IGW_OBS_LOAD(3) IGW_OBS_LOAD(4) IGW_OBS_LOAD(5) IGW_OBS_LOAD(6)
                IGW_OBS_LOAD(7)
#undef IGW_OBS_LOAD
#define IGW_OBS_STORE(k) if (k < K) { *reinterpret_cast<V*>(pc) = o##k; pc += slot; }
                IGW_OBS_STORE(1) IGW_OBS_STORE(2) IGW_OBS_STORE(3) IGW_OBS_STORE(4) IGW_OBS_STORE(5) IGW_OBS_STORE(6)
                IGW_OBS_STORE(7)
#undef IGW_OBS_STORE
                *reinterpret_cast<V*>(pc) = nv;
            }
        }
    }

    template <int kDtype>
    __device__ __forceinline__ void store_as(const uint8_t* stage, int64_t frame, int wh, int c0, int len) const {
        using E = typename ObsElem<kDtype>::E;
        const int tid = threadIdx.x;
        const bool all = fill != 0 || (restart != nullptr && restart[frame * restart_stride] != 0);
        const int64_t plane = wh, slot = (int64_t)(gray ? 1 : 3) * wh;
        E* base = static_cast<E*>(data) + frame * stack * slot + c0;   // slot 0, plane 0, pixel c0 of this env
        // Rows of the stack start wh elements apart: with wh a multiple of 4 they are all aligned alike, and a lane
        // takes 4 pixels from the first aligned one on (c0 is a multiple of 4).  Otherwise every pixel goes alone.
        const int lead = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(base) / sizeof(E))) & 3u);
        const int head = (wh & 3) ? len : min(len, lead);
        const int groups = (len - head) >> 2;
        const int tail = head + 4 * groups;
#pragma unroll 1
        for (int g = tid; g < groups; g += kThreads) {
            const int q = head + 4 * g;
            lane<kDtype, 4>(stage, base + q, q, all, plane, slot);
        }
#pragma unroll 1
        for (int s = tid; s < head + (len - tail); s += kThreads) {
            const int q = s < head ? s : tail + (s - head);
            lane<kDtype, 1>(stage, base + q, q, all, plane, slot);
        }
    }

    // Called by every thread of the block once the chunk's colours (3 bytes per pixel) are staged and published.
    __device__ __forceinline__ void store(const uint8_t* stage, int64_t frame, int wh, int c0, int len) const {
        switch (dtype) {   // block-uniform
            case IGW_OBS_U8: store_as<IGW_OBS_U8>(stage, frame, wh, c0, len); break;
            case IGW_OBS_F16: store_as<IGW_OBS_F16>(stage, frame, wh, c0, len); break;
            case IGW_OBS_BF16: store_as<IGW_OBS_BF16>(stage, frame, wh, c0, len); break;
            default: store_as<IGW_OBS_F32>(stage, frame, wh, c0, len); break;
        }
    }
};

}  // namespace

#endif
