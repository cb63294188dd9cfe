// igw_voxel_table.h -- the channel table of the two voxel writers: statements, included inside the kernel body by
// igw_vox.hip and igw_recall.hip (no include guard).  channel -> (plane, test): lane tid < kTable leaves which plane its
// channel reads in ch_plane[tid] and which code it compares with in ch_match[tid]; a one-hot plane is six channels
// (codes 1..6), an occupancy plane and the agent's are one (code 1).
// In scope: `tid`, the LDS arrays `ch_plane` and `ch_match`, igw_voxel.h, and the including file's macros
//   VOXEL_PLANES        the number of planes besides the agent's      VOXEL_AGENT   whether the agent's plane is there
//   VOXEL_ENCODING(k)   plane k's encoding (kOneHot / kOcc)
if (tid < kTable) {
    int plane = 0, match = 0, first = 0;
#pragma unroll
    for (int k = 0; k < kMaxSources; k++) {
        if (k < VOXEL_PLANES) {
            const int count = VOXEL_ENCODING(k) == kOneHot ? 6 : 1;
            if (tid >= first && tid < first + count) {
                plane = k;
                match = VOXEL_ENCODING(k) == kOneHot ? tid - first + 1 : 1;
            }
            first += count;
        }
    }
    if (VOXEL_AGENT && tid == first) {
        plane = VOXEL_PLANES;
        match = 1;
    }
    ch_plane[tid] = (uint8_t)plane;
    ch_match[tid] = (uint8_t)match;
}
