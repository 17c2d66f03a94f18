// splat2_internal.hpp - what the stream (splat2.hip) and the schedule build (splat2_sched.hip) of k_splat2 share.
#pragma once
#include "splat2.hpp"

namespace unires {

struct S2Tile {
  static constexpr int TX = 8, TY = 4, TZ = 30, L = 32;
  static constexpr int SX = TX + 2, SY = TY + 2, SZ = TZ + 2, N = SX * SY * SZ;
  static constexpr int XS = SY * SZ, YS = SZ;
};
constexpr int kS2Waves = 4;   // waves (= independent tiles in flight) per workgroup
constexpr int kS2MaxSeg = 8;  // segments per instruction

#define S2_FENCE() asm volatile("" ::: "memory")

inline int s2_ntiles(Dim3i dd) { return tile_count(dd, S2Tile::TX, S2Tile::TY, S2Tile::TZ); }

// (splat2.hip) The launch a schedule is laid out for: workgroups of the persistent grid (share_cap:
// PushEpilogue::grid_cap), and those of them that take tiles - as many as the device holds at once of k_splat2<axis>.
int s2_grid(Dim3i dd, int share_cap = 0);
int s2_active(int axis, int grid);

}  // namespace unires
