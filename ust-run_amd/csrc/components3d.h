// The third axis of connected-component labelling (components3d.hip: ustrun_post_process_3d), host and device alike, beside
// components.h, whose find / unite / tiles / border pairs are used as they are: the 26-neighbourhood restricted to one slice is the
// 8-neighbourhood and the 6-neighbourhood restricted to one slice is the cross, so inside a slice a volume is labelled as a plane is,
// and only the pairs between adjacent slices are new.  tests/host/components3d_check.hip replays all of it on the CPU.
//
// A volume's voxel e = (z * H + y) * W + x is node e + 1 of a forest P[0 .. D*H*W]; node 0 is the outside, which every background
// voxel on a face of the volume joins when holes are searched.  The invariants are components.h's: parents only decrease, a root is
// its component's smallest node, the result does not depend on the order of the unions.
#pragma once
#include "components.h"

namespace ustrun {
namespace cc {

CC_HD int vnode(int z, int y, int x, int H, int W) { return node(((long)z * H + y) * W + x); }
// a voxel on a face of the volume: its neighbour outside is background that leads away
CC_HD bool on_face(int z, int y, int x, int D, int H, int W) {
    return z == 0 || y == 0 || x == 0 || z == D - 1 || y == H - 1 || x == W - 1;
}

// ---- neighbour pairs between adjacent slices.  fan 1 (6 neighbours): (z, y, x) - (z - 1, y, x).  fan 9 (26 neighbours):
// (z, y, x) - (z - 1, y + dy, x + dx), dy, dx in -1 .. 1.  Each undirected pair is named once, from its voxel in the upper slice z:
// slot = (((z - 1) * H + y) * W + x) * fan + k, k = (dy + 1) * 3 + (dx + 1) for fan 9.
CC_HD long z_slots(int fan, int D, int H, int W) { return (long)fan * (D - 1) * H * W; }
// false: the neighbour lies outside the volume
CC_HD bool z_pair(int fan, int H, int W, long slot, int* z, int* y, int* x, int* dy, int* dx) {
    const int k = (int)(slot % fan);
    const long e = slot / fan;
    *x = (int)(e % W); *y = (int)(e / W % H); *z = (int)(e / W / H) + 1;
    *dy = fan == 9 ? k / 3 - 1 : 0; *dx = fan == 9 ? k % 3 - 1 : 0;
    return *y + *dy >= 0 && *y + *dy < H && *x + *dx >= 0 && *x + *dx < W;
}

// A pair both of whose voxels are members need not be united when other pairs of the same enumeration, together with the
// neighbours inside each slice (joined in the final forest, whatever the order: the slice-local labelling and the in-plane merge
// are launches of their own), connect its voxels anyway.  mem(z, y, x): membership, asked only inside the volume.
//   direct (dy = dx = 0): the left neighbours of both voxels are members -- the direct pair one step left joins the same two runs.
//                         It leans only on direct pairs further left in its row: the leftmost pair of a stretch always unites.
//   diagonal:             (z - 1, y, x) is a member -- it lies beside (z - 1, y + dy, x + dx) in that slice and makes a direct pair
//                         with (z, y, x) --, or (z, y + dy, x + dx) is one: it lies beside (z, y, x) and makes a direct pair with
//                         the voxel below it.  A diagonal pair leans only on direct pairs; no direct pair leans on a diagonal one.
// No pair is dropped because of a pair that is dropped because of it.  (fan 1 has only direct pairs, and "beside" there means the
// cross: left neighbours are in it.)
template <class M>
CC_HD bool z_pair_redundant(int z, int y, int x, int dy, int dx, const M& mem) {
    if (dy == 0 && dx == 0) return x > 0 && mem(z, y, x - 1) && mem(z - 1, y, x - 1);
    return mem(z - 1, y, x) || mem(z, y + dy, x + dx);
}

// ---- largest only: the winner of a volume is the maximum of this key over its roots -- the largest size, and among equal sizes
// the smallest root, i.e. the component whose smallest voxel index is smallest.  size <= 2^27, root <= 2^27: no bit is lost.
CC_HD unsigned long long largest_key(int size, int root) {
    return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xffffffffu - (unsigned)root);
}
CC_HD int key_root(unsigned long long key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

}  // namespace cc
}  // namespace ustrun
