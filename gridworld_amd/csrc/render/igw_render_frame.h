// igw_render_frame.h -- what every kernel of libigw_render.so (igw_render.hip) shares: the block's LDS, the build of
// the occupancy bitmap from a grid, and the per-block body of the first-person ray caster (the camera basis of one
// pose, and the pixels of one chunk of one frame from a grid and occupancy bitmap already in LDS).  There is one ray
// caster; the kernels differ only in where the pose, the grid and the bitmap come from.  The contract is DESIGN.md, section "First-person frames".
#ifndef IGW_RENDER_FRAME_H
#define IGW_RENDER_FRAME_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/igw_render.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;           // pixels per block: one block per frame at 64 x 64
constexpr int kGridStride = 1104;      // include/igw.h: IGW_GRID_STRIDE
constexpr int kCells = 1089;           // include/igw.h: IGW_CELLS
constexpr int kOccWords = 48;          // include/igw.h: IGW_OCC_WORDS
constexpr float kNear = 0.1f, kFar = 30.f;   // gluPerspective(90, W/H, 0.1, 30), gridworld/render.py:104

// the six faces of a cube, by the side the ray enters through (gridworld/utils.py:26-43 names)
enum Face { kTop, kBottom, kLeft, kRight, kFront, kBack };

__device__ __forceinline__ bool occupied(const uint32_t* occ, int cy, int cx, int cz) {
    // include/igw.h: bit (y+1)*169 + (x+6)*13 + (z+6) for world (x, y, z) = grid[y+1][x+5][z+5]
    const int bit = cy * 169 + (cx + 1) * 13 + (cz + 1);
    return (occ[bit >> 5] >> (bit & 31)) & 1u;
}

__device__ __forceinline__ int texel_index(float u, int n) {   // GL_NEAREST texel of coordinate u in [0, 1] on n texels
    int k = (int)floorf(u * (float)n);
    return k < 0 ? 0 : k >= n ? n - 1 : k;
}

// The LDS of one block, declared once for every kernel: the env's grid, its occupancy bitmap, and the staging area
// of the chunk's colours (free until the pixels are shaded: the episodes kernel keeps its replay table there).
// 17,680 bytes.
__shared__ uint4 s_grid4[kGridStride / 16];
__shared__ uint4 s_occ4[kOccWords / 4];
__shared__ uint4 s_stage4[kChunk * 4 / 16];

__device__ __forceinline__ int8_t* lds_grid() { return reinterpret_cast<int8_t*>(s_grid4); }
__device__ __forceinline__ uint32_t* lds_occ() { return reinterpret_cast<uint32_t*>(s_occ4); }

// The occupancy bitmap of the grid in LDS (include/igw.h: bit (y+1)*169 + (x+6)*13 + (z+6) of grid[y+1][x+5][z+5]; a
// cell is occupied iff it is not 0).  Every thread of the block calls it; its barrier publishes the caller's stores to
// s_grid.  One thread per (y, x) row of 11 cells gathers the row's 11 bits and ORs them into the one or two words they
// fall in.  The words are complete after the next barrier (the first one of render_frame()).
__device__ __forceinline__ void build_occ(const int8_t* s_grid, uint32_t* s_occ) {
    const int tid = threadIdx.x;
    if (tid < kOccWords) s_occ[tid] = 0u;
    __syncthreads();
    if (tid < 99) {
        const int yv = tid / 11, xv = tid - yv * 11;
        const int8_t* cells = s_grid + tid * 11;
        uint32_t bits = 0;
        for (int z = 0; z < 11; z++) bits |= (uint32_t)(cells[z] != 0) << z;
        const int bit = yv * 169 + (xv + 1) * 13 + 1, sh = bit & 31;
        if (bits) {
            atomicOr(&s_occ[bit >> 5], bits << sh);
            if (sh > 21 && (bits >> (32 - sh))) atomicOr(&s_occ[(bit >> 5) + 1], bits >> (32 - sh));
        }
    }
}

// The optional per-pixel planes of the _aux entries (include/igw_render.h: igw_render_aux), handed to the kernels by
// value: depth f32 (the ray parameter t of the visible surface, +inf for sky), label u8 (0 sky, 1..6 the block's
// colour, 7 WHITE / 8 GREY ground), surface i16 (-1 sky, face * 1089 + cell, 6 * 1089 + ground quad).  NULL = not wanted.
struct Planes {
    float* depth;
    uint8_t* label;
    int16_t* surface;
};
constexpr int kGroundSpan = 37;        // ground quads per side, centres -18 .. 18
constexpr int kLabelWhite = 7;         // label of the WHITE ground; GREY is the next one

// One chunk of one frame: pixels [c0, c0 + kChunk) of frame `frame` of `out` ([*][H][W][C], c0 = blockIdx.y *
// kChunk), seen from `pose` (x, y, z, yaw, pitch in degrees: the order of an agent record, include/igw.h) in the grid
// and occupancy bitmap that the block is writing to LDS.  Every thread of the block calls it; its first barrier
// publishes s_grid / s_occ, so the caller's LDS stores may still be in flight.  The colours are staged in s_stage4
// (kChunk * 4 bytes) and leave as 16-byte stores where the alignment allows.
// kAux = true also writes the planes of `pl` that are not NULL, from the same registers the colour is shaded from:
// consecutive threads hold consecutive pixels, so each plane leaves as coalesced 4-, 2- and 1-byte stores.  `out`
// may then be NULL (no texel fetch, no staging, no colour stores).  kAux = false compiles all of it away (`pl` is
// never read and `out` is taken as given).
template <bool kAux>
__device__ __forceinline__ void render_frame(const double* pose, const uint32_t* s_occ, const int8_t* s_grid,
                                             uint4* s_stage4, const uint32_t* atlas, int side, uint8_t* out,
                                             int64_t frame, int W, int H, int C, Planes pl = Planes{}) {
    const int tid = threadIdx.x;
    const bool shade = !kAux || out != nullptr;
    // camera (gridworld/render.py:94-111): forward = get_sight_vector, right, up; f64 like the pose
    const double ex = pose[0], ey = pose[1], ez = pose[2];
    double sy, cy, sp, cp;
    sincos(pose[3] * (M_PI / 180.0), &sy, &cy);
    sincos(pose[4] * (M_PI / 180.0), &sp, &cp);
    const float fx = (float)(sy * cp), fy = (float)sp, fz = (float)(-cy * cp);
    const float rx = (float)cy, rz = (float)sy;
    const float ux = (float)(-sy * sp), uy = (float)cp, uz = (float)(cy * sp);
    // a pose that is not finite or far outside the world sees nothing but sky (the scene spans |x|, |z| <= 18.5)
    const bool visible = fabs(ex) < 1e4 && fabs(ey) < 1e4 && fabs(ez) < 1e4 && isfinite(fx + fy + fz + ux + uy + uz);
    // integer origin next to the eye: eye in [0, 1)^3, cell / quad boundaries exact
    const double oxd = visible ? floor(ex) : 0., oyd = visible ? floor(ey) : 0., ozd = visible ? floor(ez) : 0.;
    const int ox = (int)oxd, oy = (int)oyd, oz = (int)ozd;
    const float px0 = visible ? (float)(ex - oxd) : 0.f, py0 = visible ? (float)(ey - oyd) : 0.f,
                pz0 = visible ? (float)(ez - ozd) : 0.f;
    const float lox = -5.5f - (float)ox, loy = -1.5f - (float)oy, loz = -5.5f - (float)oz;   // build-zone box
    const float ground = -1.5f - (float)oy;
    __syncthreads();
    uint8_t* stage = reinterpret_cast<uint8_t*>(s_stage4);

    const int wh = W * H;
    const int c0 = blockIdx.y * kChunk;
    const int len = min(kChunk, wh - c0);
    const int sub = side >> 3;                // texels of a half tile (tex_coord(..., split=True))
    const float inv_h = 1.f / (float)H;
    for (int q = tid; q < len; q += kThreads) {
        const int pix = c0 + q;
        const int i = pix / W, j = pix - (pix / W) * W;
        uint32_t rgba = IGW_RENDER_CLEAR_RGBA;
        float depth = INFINITY;            // the planes' sky (kAux only)
        int label = 0, surface = -1;
        if (visible) {
            // d = f + ((2j+1)/W - 1)(W/H) r + (1 - (2i+1)/H) u: t along d is the eye-space depth
            const float a = (float)(2 * j + 1 - W) * inv_h, b = (float)(H - 2 * i - 1) * inv_h;
            const float dx = fx + a * rx + b * ux, dy = fy + b * uy, dz = fz + a * rz + b * uz;
            const float ix = 1.f / dx, iy = 1.f / dy, iz = 1.f / dz;
            // clip to the box [lo, lo + n]
            float t0 = 0.f, t1 = kFar;
            int axis = -1;
            bool miss = false;
#define IGW_SLAB(P, D, I, LO, N, K)                                                       \
            if (D != 0.f) {                                                               \
                float ta = (LO - P) * I, tb = (LO + N - P) * I;                           \
                if (ta > tb) { float s = ta; ta = tb; tb = s; }                           \
                if (ta > t0) { t0 = ta; axis = K; }                                       \
                t1 = fminf(t1, tb);                                                       \
            } else if (P < LO || P > LO + N) miss = true;
            IGW_SLAB(px0, dx, ix, lox, 11.f, 0)
            IGW_SLAB(py0, dy, iy, loy, 9.f, 1)
            IGW_SLAB(pz0, dz, iz, loz, 11.f, 2)
#undef IGW_SLAB
            int face = -1, hx = 0, hy = 0, hz = 0;
            float th = 0.f;
            if (!miss && t0 <= t1) {
                int cx = min(max((int)floorf(px0 + t0 * dx - lox), 0), 10);
                int cyy = min(max((int)floorf(py0 + t0 * dy - loy), 0), 8);
                int cz = min(max((int)floorf(pz0 + t0 * dz - loz), 0), 10);
                if (axis == 0) cx = dx > 0.f ? 0 : 10;
                if (axis == 1) cyy = dy > 0.f ? 0 : 8;
                if (axis == 2) cz = dz > 0.f ? 0 : 10;
                const int face_x = dx > 0.f ? kLeft : kRight, face_y = dy > 0.f ? kBottom : kTop,
                          face_z = dz > 0.f ? kBack : kFront;
                if (axis >= 0 && t0 >= kNear && occupied(s_occ, cyy, cx, cz)) {
                    face = axis == 0 ? face_x : axis == 1 ? face_y : face_z;
                    th = t0;
                }
                const int sx = dx > 0.f ? 1 : -1, syy = dy > 0.f ? 1 : -1, sz = dz > 0.f ? 1 : -1;
                // the next boundary crossed on each axis, recomputed from the cell (no accumulated error)
                float nx = dx != 0.f ? (lox + (float)(cx + (dx > 0.f)) - px0) * ix : INFINITY;
                float ny = dy != 0.f ? (loy + (float)(cyy + (dy > 0.f)) - py0) * iy : INFINITY;
                float nz = dz != 0.f ? (loz + (float)(cz + (dz > 0.f)) - pz0) * iz : INFINITY;
                // at most 10 + 8 + 10 crossings inside the box
                for (int it = 0; face < 0 && it < 30; ++it) {
                    float t;
                    int f;
                    if (nx <= ny && nx <= nz) {
                        t = nx; cx += sx; f = face_x;
                        if (cx < 0 || cx > 10) break;
                        nx = (lox + (float)(cx + (dx > 0.f)) - px0) * ix;
                    } else if (ny <= nz) {
                        t = ny; cyy += syy; f = face_y;
                        if (cyy < 0 || cyy > 8) break;
                        ny = (loy + (float)(cyy + (dy > 0.f)) - py0) * iy;
                    } else {
                        t = nz; cz += sz; f = face_z;
                        if (cz < 0 || cz > 10) break;
                        nz = (loz + (float)(cz + (dz > 0.f)) - pz0) * iz;
                    }
                    if (t > kFar) break;
                    if (t >= kNear && occupied(s_occ, cyy, cx, cz)) { face = f; th = t; }
                }
                hx = cx; hy = cyy; hz = cz;
            }
            int col = -1, rowb = 0;
            if (face >= 0) {
                // where the ray enters the cell, in the cell's own unit coordinates
                const float lx = px0 + th * dx - (lox + (float)hx), ly = py0 + th * dy - (loy + (float)hy),
                            lz = pz0 + th * dz - (loz + (float)hz);
                // u / v of each face: vertex order of cube_vertices against corner order of tex_coord
                // (gridworld/utils.py:26-43, 82-123); sub-tile (cx, cy) per face: top (0, 1/8), bottom (1/8, 0),
                // left / right (0, 0), front / back (1/8, 1/8)
                float u, v;
                int cu, cv;
                switch (face) {
                    case kTop: u = lz; v = lx; cu = 0; cv = 1; break;
                    case kBottom: u = lx; v = lz; cu = 1; cv = 0; break;
                    case kLeft: u = lz; v = ly; cu = 0; cv = 0; break;
                    case kRight: u = 1.f - lz; v = ly; cu = 0; cv = 0; break;
                    case kFront: u = lx; v = ly; cu = 1; cv = 1; break;
                    default: u = 1.f - lx; v = ly; cu = 1; cv = 1; break;
                }
                const int cell = hy * 121 + hx * 11 + hz;
                int id = s_grid[cell];
                id = id < 1 ? 1 : id > 6 ? 6 : id;   // BLUE .. YELLOW (world grids hold no other id)
                if constexpr (kAux) { depth = th; label = id; surface = face * kCells + cell; }
                const int tile = id + 1;            // tiles (2,0) (3,0) (0,1) (1,1) (2,1) (3,1), utils.py:139-146
                col = (tile & 3) * 2 * sub + cu * sub + texel_index(u, sub);
                rowb = (tile >> 2) * 2 * sub + cv * sub + texel_index(v, sub);
            } else if (dy < 0.f && py0 > ground) {
                // the ground: top faces of the 37 x 37 quads centred on x, z in [-18, 18] at y = -1.5 (world.py:60-71)
                const float t = (ground - py0) * iy;
                if (t >= kNear && t <= kFar) {
                    const float gx = px0 + t * dx + 0.5f, gz = pz0 + t * dz + 0.5f;
                    const float fgx = floorf(gx), fgz = floorf(gz);
                    const int qx = ox + (int)fgx, qz = oz + (int)fgz;   // centre of the quad hit
                    if (qx >= -18 && qx <= 18 && qz >= -18 && qz <= 18) {
                        const int tile = (qx >= -5 && qx <= 5 && qz >= -5 && qz <= 5) ? 0 : 1;   // WHITE : GREY
                        col = tile * 2 * sub + texel_index(gz - fgz, 2 * sub);   // top face: u = z, v = x
                        rowb = texel_index(gx - fgx, 2 * sub);
                        if constexpr (kAux) {
                            depth = t; label = kLabelWhite + tile;
                            surface = 6 * kCells + (qx + 18) * kGroundSpan + (qz + 18);
                        }
                    }
                }
            }
            if (shade && col >= 0) rgba = atlas[(side - 1 - rowb) * side + col];   // v = 0 is the bottom image row
        }
        if constexpr (kAux) {
            const int64_t at = frame * (int64_t)wh + pix;
            if (pl.depth) pl.depth[at] = depth;
            if (pl.label) pl.label[at] = (uint8_t)label;
            if (pl.surface) pl.surface[at] = (int16_t)surface;
            if (!shade) continue;
        }
        if (C == 4) {
            reinterpret_cast<uint32_t*>(stage)[q] = rgba;
        } else {
            stage[3 * q] = (uint8_t)rgba;
            stage[3 * q + 1] = (uint8_t)(rgba >> 8);
            stage[3 * q + 2] = (uint8_t)(rgba >> 16);
        }
    }
    if (!shade) return;   // block-uniform
    __syncthreads();
    // the chunk's bytes are contiguous in the frame: 16-byte stores where the alignment allows
    const int nbytes = len * C;
    uint8_t* dst = out + (frame * (int64_t)wh + c0) * C;
    if (((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)nbytes) & 15) == 0) {
        for (int k = tid; k < nbytes / 16; k += kThreads) reinterpret_cast<uint4*>(dst)[k] = s_stage4[k];
    } else if (((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)nbytes) & 3) == 0) {
        for (int k = tid; k < nbytes / 4; k += kThreads)
            reinterpret_cast<uint32_t*>(dst)[k] = reinterpret_cast<const uint32_t*>(stage)[k];
    } else {
        for (int k = tid; k < nbytes; k += kThreads) dst[k] = stage[k];
    }
}

}  // namespace

#endif
