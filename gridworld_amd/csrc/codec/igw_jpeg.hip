// igw_jpeg.hip -- baseline JPEG of rendered frames on gfx950 (include/igw_codec.h).
//
// The stream and its integer arithmetic are specified in DESIGN.md, section 9 ("JPEG frames and MJPEG video");
// tests/jpeg_model.py is an independent numpy model of that section that the GPU tests compare against byte for byte.
//
// Layout: one workgroup of 256 threads per frame.  The frame is taken in chunks of 64 MCUs in scan order (4:4:4: an
// MCU is one 8 x 8 block of each of Y, Cb, Cr, so a chunk is up to 192 blocks; a 64 x 64 frame is exactly one chunk).
// Per chunk: pixels -> level-shifted YCbCr in LDS (int16), the row and the column pass of the DCT per thread on LDS,
// quantisation in the column pass; then one thread per block walks its 64 coefficients twice: once for the block's bit
// count (a workgroup prefix sum turns the counts into bit offsets), once to OR its codes into an LDS bit window with
// LDS atomics.  The window holds 4 KiB of the scan; a chunk that needs more takes several rounds, every thread resuming
// where the window ended.  Complete bytes of the window are byte-stuffed into a staging area (a second prefix sum, over
// bytes + FF bytes) and leave as consecutive stores.  The DC predictors, the bit position and the output position
// carry from chunk to chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/igw_codec.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunkMcus = 64;
constexpr int kChunkBlocks = 3 * kChunkMcus;
constexpr int kWinWords = 1024;              // the bit window: 4 KiB of the scan ...
constexpr int kWinBits = 32 * kWinWords;
constexpr int kWinBytes = 4 * kWinWords;
constexpr int kSlackWords = 2;               // ... plus what the last code of a round may reach past it (< 26 + 31 bits)
constexpr int kHeader = IGW_JPEG_HEADER_BYTES;
constexpr int kBlockBytes = 420;             // igw_jpeg_bound: 2 * ceil((22 + 63 * 26) / 8) rounded up

// ---- Annex K --------------------------------------------------------------------------------------------------------
struct Tables {
    uint8_t quant[2][64];    // K.1, K.2 in natural order
    uint8_t zigzag[64];      // zigzag position -> natural index
    uint32_t dc[2][12];      // symbol -> length << 16 | code (luma, chroma)
    uint32_t ac[2][256];
    uint8_t header[kHeader]; // SOI .. SOS with the tables' contents and the frame's size left 0
};

constexpr uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// where the header's variable bytes are: the two DQT tables' 64 entries, and SOF0's height and width
constexpr int kDqt0 = 25, kDqt1 = 94, kSofSize = 163;

constexpr Tables make_tables() {
    Tables t{};
    for (int k = 0; k < 64; k++) {
        t.quant[0][k] = kLumaQ[k];
        t.quant[1][k] = kChromaQ[k];
        t.zigzag[k] = kZigzag[k];
    }
    // the canonical code assignment of Annex C
    for (int tab = 0; tab < 2; tab++) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < kDcBits[tab][len - 1]; i++) t.dc[tab][k++] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < kAcBits[tab][len - 1]; i++) t.ac[tab][kAcVals[tab][k++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
    int n = 0;
    uint8_t* h = t.header;
    const uint8_t soi_app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t b : soi_app0) h[n++] = b;
    for (int tab = 0; tab < 2; tab++) {
        const uint8_t dqt[5] = {0xff, 0xdb, 0, 67, (uint8_t)tab};
        for (uint8_t b : dqt) h[n++] = b;
        n += 64;
    }
    const uint8_t sof[19] = {0xff, 0xc0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (uint8_t b : sof) h[n++] = b;
    for (int tab = 0; tab < 2; tab++) {
        const uint8_t dht_dc[5] = {0xff, 0xc4, 0, 19 + 12, (uint8_t)tab};
        for (uint8_t b : dht_dc) h[n++] = b;
        for (int i = 0; i < 16; i++) h[n++] = kDcBits[tab][i];
        for (int i = 0; i < 12; i++) h[n++] = (uint8_t)i;
        const uint8_t dht_ac[5] = {0xff, 0xc4, 0, 19 + 162, (uint8_t)(0x10 | tab)};
        for (uint8_t b : dht_ac) h[n++] = b;
        for (int i = 0; i < 16; i++) h[n++] = kAcBits[tab][i];
        for (int i = 0; i < 162; i++) h[n++] = kAcVals[tab][i];
    }
    const uint8_t sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (uint8_t b : sos) h[n++] = b;
    return t;
}

__constant__ const Tables kT = make_tables();

// ---- the workgroup's LDS ----------------------------------------------------------------------------------------------
__shared__ __attribute__((aligned(16))) int16_t s_coef[kChunkBlocks * 64];   // samples, then quantised coefficients
__shared__ uint32_t s_win[kWinWords + kSlackWords];                          // the bit window, big-endian words
__shared__ uint8_t s_stage[2 * kWinBytes];                                   // stuffed bytes on their way out
__shared__ uint32_t s_huff[24 + 512];                                        // dc[2][12], ac[2][256]
__shared__ uint32_t s_rcp[128];                                              // 2^20 / q + 1 of the scaled tables
__shared__ uint16_t s_q[128];                                                // the scaled tables, natural order
__shared__ uint8_t s_zz[64];
__shared__ int s_pred[3];                                                    // DC predictors carried between chunks
__shared__ int s_wave[kThreads / 64];

// Exclusive prefix sum of `v` over the workgroup's threads; `total` is the sum.  Two barriers.
__device__ __forceinline__ int block_scan(int v, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the wavefront's inclusive scan on DPP: shifts by 1, 2, 4, 8 inside every row of 16 lanes (a lane without a
    // source adds 0), then lane 15 of a row into the next row (rows 1, 3) and lane 31 into rows 2 and 3
    int inc = v;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, false);
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, false);
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, false);
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, false);
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xa, 0xf, false);
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xc, 0xf, false);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; i++) {
        const int x = s_wave[i];
        if (i < w) base += x;
        total += x;
    }
    __syncthreads();
    return base + inc - v;
}

// One pass of the DCT: o[u] = (sum_x C[u][x] s[x] + round) >> shift.  C[u][7 - x] =
// (-1)^u C[u][x], so the sums are taken over the four sums / differences of mirrored inputs: integer arithmetic, the
// same value as the plain sum.
__device__ __forceinline__ void dct8(const int (&s)[8], int (&o)[8], int round, int shift) {
    const int a0 = s[0] + s[7], a1 = s[1] + s[6], a2 = s[2] + s[5], a3 = s[3] + s[4];
    const int b0 = s[0] - s[7], b1 = s[1] - s[6], b2 = s[2] - s[5], b3 = s[3] - s[4];
    o[0] = (2896 * (a0 + a1 + a2 + a3) + round) >> shift;
    o[4] = (2896 * (a0 - a1 - a2 + a3) + round) >> shift;
    o[2] = (3784 * (a0 - a3) + 1567 * (a1 - a2) + round) >> shift;
    o[6] = (1567 * (a0 - a3) - 3784 * (a1 - a2) + round) >> shift;
    o[1] = (4017 * b0 + 3406 * b1 + 2276 * b2 + 799 * b3 + round) >> shift;
    o[3] = (3406 * b0 - 799 * b1 - 4017 * b2 - 2276 * b3 + round) >> shift;
    o[5] = (2276 * b0 - 4017 * b1 + 799 * b2 + 3406 * b3 + round) >> shift;
    o[7] = (799 * b0 - 2276 * b1 + 3406 * b2 - 4017 * b3 + round) >> shift;
}

// ORs the n-bit code (n <= 26) into the window at bit `rel` of it (MSB first).
__device__ __forceinline__ void put(uint32_t code, int n, int rel) {
    const uint64_t t = (uint64_t)code << (64 - n - (rel & 31));
    const uint32_t hi = (uint32_t)(t >> 32), lo = (uint32_t)t;
    atomicOr(&s_win[rel >> 5], hi);
    if (lo) atomicOr(&s_win[(rel >> 5) + 1], lo);
}

// category and extra bits of a non-zero value (F.1.2.1); a zero gives category 0
__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }
__device__ __forceinline__ uint32_t extra_bits(int v, int cat) { return (uint32_t)(v >= 0 ? v : v + (1 << cat) - 1); }

// Byte-stuffs the window's bytes [from, upto) and stores them at o[pos ..] (only below `stride`); returns how many
// bytes that is.  Every thread looks at 16 bytes of the window.  Three barriers; the window is not read after the
// first.
__device__ __forceinline__ int flush(int from, int upto, uint8_t* __restrict__ o, int64_t pos, int64_t stride) {
    const int tid = threadIdx.x;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = s_win[4 * tid + i];
    // bit j of `ff`: byte j of the 16 is FF; bit j of `take`: it lies in [from, upto)
    uint32_t ff = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) ff |= ((((w[j >> 2] >> (24 - 8 * (j & 3))) & 255u) + 1u) >> 8) << j;
    const int lo = min(max(from - 16 * tid, 0), 16), hi = min(max(upto - 16 * tid, 0), 16);
    const uint32_t take = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    int total;
    int off = block_scan(__popc(take) + __popc(take & ff), total);
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if ((take >> j) & 1u) {
            s_stage[off++] = (uint8_t)(w[j >> 2] >> (24 - 8 * (j & 3)));
            if ((ff >> j) & 1u) s_stage[off++] = 0;
        }
    }
    __syncthreads();
    for (int j = tid; j < total; j += kThreads)
        if (pos + j < stride) o[pos + j] = s_stage[j];
    return total;
}

__global__ __launch_bounds__(kThreads) void igw_jpeg_encode_kernel(const uint8_t* __restrict__ frames, int W, int H,
                                                               int C, int quality, uint8_t* __restrict__ out,
                                                               int64_t stride, int32_t* __restrict__ sizes) {
    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.x;
    const uint8_t* __restrict__ src = frames + frame * ((int64_t)H * W * C);
    uint8_t* __restrict__ o = out + frame * stride;

    // ---- tables to LDS: the scaled quantisation tables with their reciprocals, the Huffman codes, the window ----
    if (tid < 128) {
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        int q = ((int)kT.quant[tid >> 6][tid & 63] * scale + 50) / 100;
        q = min(max(q, 1), 255);
        s_q[tid] = (uint16_t)q;
        s_rcp[tid] = (1u << 20) / (uint32_t)q + 1u;   // (n * rcp) >> 20 == n / q for every n < 1400 and q <= 255
    } else if (tid < 192) {
        s_zz[tid - 128] = kT.zigzag[tid - 128];
    } else if (tid < 195) {
        s_pred[tid - 192] = 0;
    }
    for (int i = tid; i < 24 + 512; i += kThreads)
        s_huff[i] = i < 24 ? kT.dc[i / 12][i % 12] : kT.ac[(i - 24) >> 8][(i - 24) & 255];
    for (int i = tid; i < kWinWords + kSlackWords; i += kThreads) s_win[i] = 0;
    __syncthreads();

    // ---- the header ----
    for (int i = tid; i < kHeader; i += kThreads) {
        uint32_t b = kT.header[i];
        if (i >= kDqt0 && i < kDqt0 + 64) b = s_q[s_zz[i - kDqt0]];
        else if (i >= kDqt1 && i < kDqt1 + 64) b = s_q[64 + s_zz[i - kDqt1]];
        else if (i == kSofSize) b = (uint32_t)H >> 8;
        else if (i == kSofSize + 1) b = (uint32_t)H & 255u;
        else if (i == kSofSize + 2) b = (uint32_t)W >> 8;
        else if (i == kSofSize + 3) b = (uint32_t)W & 255u;
        if (i < stride) o[i] = (uint8_t)b;
    }

    const int mcus_x = (W + 7) >> 3, n_mcu = mcus_x * ((H + 7) >> 3);
    // what carries from chunk to chunk, the same in every thread: the absolute bit position of the scan's end so far,
    // the bit position of the window's first bit (a multiple of 32), the window's bytes already flushed, and the next
    // output byte
    int scan_bits = 0, win_base = 0, flushed = 0;
    int64_t pos = kHeader;

    for (int mcu0 = 0; mcu0 < n_mcu; mcu0 += kChunkMcus) {
        const int n_blk = 3 * min(kChunkMcus, n_mcu - mcu0);

        // ---- pixels -> level-shifted Y, Cb, Cr: thread (m, c) takes column c of MCUs m and m + 32, 8 rows each ----
        {
            const int c = tid & 7;
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int m = (tid >> 3) + 32 * half;
                if (3 * m >= n_blk) continue;
                const int g = mcu0 + m, gy = g / mcus_x, gx = g - gy * mcus_x;
                const int x = min(8 * gx + c, W - 1);
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const int y = min(8 * gy + r, H - 1);
                    const uint8_t* p = src + ((int64_t)y * W + x) * C;
                    const int R = p[0], G = p[1], B = p[2];
                    const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
                    const int Cb = min((-11058 * R - 21710 * G + 32768 * B + 32768 + (128 << 16)) >> 16, 255);
                    const int Cr = min((32768 * R - 27439 * G - 5329 * B + 32768 + (128 << 16)) >> 16, 255);
                    int16_t* d = s_coef + m * 192 + r * 8 + c;
                    d[0] = (int16_t)(Y - 128);
                    d[64] = (int16_t)(Cb - 128);
                    d[128] = (int16_t)(Cr - 128);
                }
            }
        }
        __syncthreads();

        // ---- DCT rows: task = (block, row), 8 consecutive int16 in place ----
        for (int task = tid; task < 8 * n_blk; task += kThreads) {
            uint4* row = reinterpret_cast<uint4*>(s_coef + 8 * task);
            const uint4 v = *row;
            const uint32_t in[4] = {v.x, v.y, v.z, v.w};
            int s[8], t[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                s[2 * i] = (int16_t)(in[i] & 0xffffu);
                s[2 * i + 1] = (int16_t)(in[i] >> 16);
            }
            dct8(s, t, 1 << 10, 11);
            uint4 r;
            r.x = ((uint32_t)t[0] & 0xffffu) | ((uint32_t)t[1] << 16);
            r.y = ((uint32_t)t[2] & 0xffffu) | ((uint32_t)t[3] << 16);
            r.z = ((uint32_t)t[4] & 0xffffu) | ((uint32_t)t[5] << 16);
            r.w = ((uint32_t)t[6] & 0xffffu) | ((uint32_t)t[7] << 16);
            *row = r;
        }
        __syncthreads();

        // ---- DCT columns and quantisation: task = (block, column u) ----
        for (int task = tid; task < 8 * n_blk; task += kThreads) {
            const int blk = task >> 3, u = task & 7;
            const int tab = (blk % 3) ? 64 : 0;
            int16_t* col = s_coef + 64 * blk + u;
            int s[8], f[8];
#pragma unroll
            for (int y = 0; y < 8; y++) s[y] = col[8 * y];
            dct8(s, f, 1 << 14, 15);
#pragma unroll
            for (int v = 0; v < 8; v++) {
                const int k = tab + 8 * v + u;
                const uint32_t a = (uint32_t)(f[v] < 0 ? -f[v] : f[v]) + (s_q[k] >> 1);
                const int qv = (int)((a * s_rcp[k]) >> 20);
                col[8 * v] = (int16_t)(f[v] < 0 ? -qv : qv);
            }
        }
        __syncthreads();

        // ---- bits of every block (thread = block), then their offsets ----
        const int16_t* blk = s_coef + 64 * tid;
        const int comp = tid % 3;
        const uint32_t* dc_tab = s_huff + (comp ? 12 : 0);
        const uint32_t* ac_tab = s_huff + 24 + (comp ? 256 : 0);
        int n_bits = 0, last = 0, dc_diff = 0;
        if (tid < n_blk) {
            dc_diff = blk[0] - (tid >= 3 ? blk[-192] : s_pred[comp]);
            const int cat = category(dc_diff);
            n_bits = (int)(dc_tab[cat] >> 16) + cat;
            int run = 0;
            for (int k = 1; k < 64; k++) {
                const int v = blk[s_zz[k]];
                if (v == 0) {
                    run++;
                    continue;
                }
                const int vc = category(v);
                n_bits += (run >> 4) * (int)(ac_tab[0xf0] >> 16) + (int)(ac_tab[((run & 15) << 4) | vc] >> 16) + vc;
                run = 0;
                last = k;
            }
            if (last < 63) n_bits += (int)(ac_tab[0] >> 16);
        }
        int chunk_bits;
        int p = scan_bits + block_scan(n_bits, chunk_bits);      // absolute bit position of this block's next code
        scan_bits += chunk_bits;
        // the frame's last chunk pads the scan to a whole byte with 1s: the code of the thread behind the last block,
        // whose position is the end of the chunk's bits
        const int pad = mcu0 + kChunkMcus >= n_mcu ? -scan_bits & 7 : 0;
        scan_bits += pad;

        // ---- codes into the window, a window at a time; step k of a block: 0 the DC code, 1..last the coefficients
        //      (a ZRL as soon as 16 zeros have passed: a non-zero follows), last + 1 the EOB ----
        const int k_end = tid < n_blk ? (last < 63 ? last + 2 : 64) : (tid == n_blk && pad ? 1 : 0);
        int k = 0, run = 0;
        for (;;) {
            const int win_end = win_base + kWinBits;
            while (k < k_end && p < win_end) {
                uint32_t code;
                int n;
                if (tid == n_blk) {
                    n = pad;
                    code = (1u << pad) - 1u;
                } else if (k == 0) {
                    const int cat = category(dc_diff);
                    const uint32_t e = dc_tab[cat];
                    n = (int)(e >> 16) + cat;
                    code = ((e & 0xffffu) << cat) | extra_bits(dc_diff, cat);
                } else if (k > last) {
                    const uint32_t e = ac_tab[0];
                    n = (int)(e >> 16);
                    code = e & 0xffffu;
                } else {
                    const int v = blk[s_zz[k]];
                    if (v == 0) {
                        k++;
                        if (++run < 16) continue;
                        run = 0;
                        const uint32_t e = ac_tab[0xf0];
                        n = (int)(e >> 16);
                        code = e & 0xffffu;
                        put(code, n, p - win_base);
                        p += n;
                        continue;
                    }
                    const int cat = category(v);
                    const uint32_t e = ac_tab[(run << 4) | cat];
                    n = (int)(e >> 16) + cat;
                    code = ((e & 0xffffu) << cat) | extra_bits(v, cat);
                    run = 0;
                }
                put(code, n, p - win_base);
                p += n;
                k++;
            }
            __syncthreads();
            const bool full = scan_bits >= win_end;            // the chunk goes on past this window
            const int upto = full ? kWinBytes : (scan_bits - win_base) >> 3;
            const uint32_t slack = tid < kSlackWords ? s_win[kWinWords + tid] : 0u;
            pos += flush(flushed, upto, o, pos, stride);
            if (!full) {
                flushed = upto;
                break;
            }
            // the next window: what reached past this one moves to the front, the rest is cleared
            for (int i = tid; i < kWinWords + kSlackWords; i += kThreads) s_win[i] = i < kSlackWords ? slack : 0u;
            win_base = win_end;
            flushed = 0;
            __syncthreads();
        }
        // the predictors of the next chunk (every read of the old ones is behind the barriers above)
        if (tid < n_blk && tid >= n_blk - 3) s_pred[comp] = blk[0];
        __syncthreads();
    }

    // ---- EOI and the size (the last chunk padded the scan to a whole byte and flushed all of it) ----
    if (tid == 0) {
        if (pos < stride) o[pos] = 0xff;
        if (pos + 1 < stride) o[pos + 1] = 0xd9;
        const int64_t total = pos + 2;
        sizes[frame] = (int32_t)(total <= stride ? total : -total);
    }
}

thread_local char g_err[512] = "";

int fail(int code, const char* entry, const char* what, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), "%s: %s%s", entry, what, detail);
    return code;
}

bool have_device() {
    static int seen = 0;   // once a device was seen it stays (the count is not re-queried per call)
    if (!seen) {
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1) return false;
        seen = 1;
    }
    return true;
}

}  // namespace

#ifndef IGW_CODEC_BUILD_ID
#define IGW_CODEC_BUILD_ID "igw-codec-build-id:unstamped"
#endif

extern "C" {

int igw_codec_version(void) { return IGW_CODEC_VERSION; }
// (the string carries a marker so that codec.py can read the id of a library file without loading it)
const char* igw_codec_build_id(void) { return &IGW_CODEC_BUILD_ID[sizeof("igw-codec-build-id:") - 1]; }
const char* igw_codec_last_error(void) { return g_err; }

int64_t igw_jpeg_bound(int32_t width, int32_t height) {
    if (width < 1 || width > IGW_CODEC_MAX_SIDE || height < 1 || height > IGW_CODEC_MAX_SIDE) return 0;
    const int64_t blocks = 3 * (int64_t)((width + 7) / 8) * ((height + 7) / 8);
    return (kHeader + kBlockBytes * blocks + 2 + 15) / 16 * 16;
}

int igw_jpeg_encode(const uint8_t* frames, int64_t n, int32_t width, int32_t height, int32_t channels, int32_t quality,
                    uint8_t* out, int64_t stride, int32_t* sizes, void* stream) {
    const char* entry = __func__;
    if (n < 0 || n > INT32_MAX) return fail(IGW_CODEC_ERR_INVALID, entry, "n must be in 0..2^31-1");
    if (channels != 3 && channels != 4) return fail(IGW_CODEC_ERR_INVALID, entry, "channels must be 3 or 4");
    if (width < 1 || width > IGW_CODEC_MAX_SIDE || height < 1 || height > IGW_CODEC_MAX_SIDE)
        return fail(IGW_CODEC_ERR_INVALID, entry, "width and height must be in 1..1024");
    if (quality < 1 || quality > 100) return fail(IGW_CODEC_ERR_INVALID, entry, "quality must be in 1..100");
    if (stride < kHeader + 2) return fail(IGW_CODEC_ERR_INVALID, entry, "stride must be >= 625 (the header and EOI)");
    if (n > 0 && (!frames || !out || !sizes)) return fail(IGW_CODEC_ERR_INVALID, entry, "null buffer");
    if (reinterpret_cast<uintptr_t>(sizes) & 3) return fail(IGW_CODEC_ERR_INVALID, entry, "sizes must be 4-byte aligned");
    if (!have_device())
        return fail(IGW_CODEC_ERR_NO_DEVICE, entry, "no HIP device available (the codec has no CPU fallback)");
    if (n == 0) return IGW_CODEC_OK;
    hipLaunchKernelGGL(igw_jpeg_encode_kernel, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, frames,
                       (int)width, (int)height, (int)channels, (int)quality, out, stride, sizes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IGW_CODEC_ERR_HIP, entry, "launch failed: ", hipGetErrorString(e));
    return IGW_CODEC_OK;
}

}  // extern "C"
