// igw_voxel_stage.h -- the staging loop of the two voxel writers: statements, included inside the kernel body by
// igw_vox.hip and igw_recall.hip (no include guard).  Each lane walks output cells o = (y, u, w) of the S x S window, maps
// them to the world cell they show (in the agent's frame: `s` cells ahead and `t` to the right of the head cell) and
// leaves one byte per plane in `cells`, already in the output frame: 0 (empty, or outside the grid), 1..6 (the colour)
// or kOther for a one-hot plane, [v != 0] for an occupancy plane and for the agent's body.
// In scope: `tid`, `R`, `S`, `SS` = S * S, `P9` = kLevels * SS, the Frame `fr`, the LDS planes `cells`, igw_voxel.h, the
// macros of igw_voxel_table.h and
//   VOXEL_EGO             whether the window is the agent's
//   VOXEL_READ(k, c, v)   statements that declare `int v`, plane k's value at world cell c; run for cells inside the grid
//   VOXEL_GUARD_CELL      1: c is 0 for a cell outside the grid; 0: c is computed for it too (and not used).  Each
//                         kernel keeps the form it was written with, so that it compiles to the instructions it had.
#pragma unroll 1
for (int o = tid; o < P9; o += kThreads) {
    const int y = o / SS, rem = o - y * SS, u = rem / S, w = rem - u * S;
    int x = u, z = w;
    if (VOXEL_EGO) {
        const int s = R - u, t = w - R;
        x = fr.hx + s * fr.fx + t * fr.rx;
        z = fr.hz + s * fr.fz + t * fr.rz;
    }
    const bool inside = (unsigned)x < 11u && (unsigned)z < 11u;
    const int c = !VOXEL_GUARD_CELL || inside ? y * 121 + x * 11 + z : 0;
#pragma unroll
    for (int k = 0; k < kMaxSources; k++) {
        if (k < VOXEL_PLANES) {
            int code = 0;
            if (inside) {
                VOXEL_READ(k, c, v)
                code = VOXEL_ENCODING(k) == kOcc ? v != 0 : v >= 1 && v <= 6 ? v : v != 0 ? kOther : 0;
            }
            cells[k * kMaxPlane + o] = (uint8_t)code;
        }
    }
    if (VOXEL_AGENT)
        cells[VOXEL_PLANES * kMaxPlane + o] = (uint8_t)(inside && x == fr.hx && z == fr.hz && (y == fr.hy || y == fr.hy - 1));
}
