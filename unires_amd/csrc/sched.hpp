// sched.hpp - what the schedule builds of k_splat2 (splat2_sched.hip) and k_ata1 (ata1.hip) share.
//
// Both kernels stream a per-operator schedule: per output tile (one wave owns it, with a one-cell apron) the segments
// of grid rows whose points land in the tile, packed into 64-lane instructions.  A build kernel makes it - one wave
// per tile - and a host routine fixes the order the tiles are processed in.  The part of that which does not depend
// on the kernel's record format is stated here once: the tile geometry, the coordinate of a row's point, the scan of
// a tile's rows into segments, the processing order and the host's bookkeeping.  The packing loops - with the exact
// rule's footprint test, which is each stream kernel's own cell arithmetic - and the records stay with their kernels.
//
// Every constant of the scan decides which points a tile accepts.  It must stay a SUPERSET test followed by the exact
// one in the stream kernel's own arithmetic: that is what makes A^T the exact adjoint of A (a point is pushed to
// exactly the cells it was pulled from) and what makes the packed instructions race-free.
#pragma once
#include "fused.hpp"

#include <stddef.h>

namespace unires {

// --------------------------------------------------------------------------
// tile geometry
// --------------------------------------------------------------------------
struct TileBox {
  int x0, y0, z0, ex, ey, ez;  // first cell and extent (clipped to the volume) of an output tile
};
// tile t of a volume cut into TX x TY x TZ tiles, z fastest (host too: ata1_build tabulates the origins)
template <int TX, int TY, int TZ>
__host__ __device__ __forceinline__ TileBox tile_box(int t, const Dim3i &dd) {
  const int nty = (dd.y + TY - 1) / TY, ntz = (dd.z + TZ - 1) / TZ;
  const int tzi = t % ntz, tyi = (t / ntz) % nty, txi = t / (ntz * nty);
  TileBox g;
  g.x0 = txi * TX, g.y0 = tyi * TY, g.z0 = tzi * TZ;
  g.ex = min(TX, dd.x - g.x0), g.ey = min(TY, dd.y - g.y0), g.ez = min(TZ, dd.z - g.z0);
  return g;
}
inline int tile_count(Dim3i dd, int tx, int ty, int tz) {
  return ((dd.x + tx - 1) / tx) * ((dd.y + ty - 1) / ty) * ((dd.z + tz - 1) / tz);
}

// --------------------------------------------------------------------------
// device: a row's points, a tile's segments
// --------------------------------------------------------------------------
// Coordinate of grid point k of a row with base (rx, ry, rz) = affine_row(A, ui, uj): affine_along() (the pull
// kernels), bit for bit, and what k_splat2 and k_ata1 compute per lane from a segment entry.  The build decides with
// it which points a tile takes, so a point is pushed into the cell it was pulled from, and two lanes the build found
// apart are apart in the stream.
__device__ __forceinline__ void sched_point(const Affine &A, float rx, float ry, float rz, float kf, float &gx,
                                            float &gy, float &gz) {
  gx = fmaf(A.m[2], kf, rx) + A.m[3];
  gy = fmaf(A.m[6], kf, ry) + A.m[7];
  gz = fmaf(A.m[10], kf, rz) + A.m[11];
}

// Where a row is cut into segments (besides at MAXLEN points):
enum class SegCut {
  kPlaneRepeats,  // wherever two consecutive points share floor(gz): the lanes of a segment sit in DIFFERENT planes (k_splat2)
  kPlaneNotNext,  // wherever floor(gz) does not advance by exactly one: lane = z plane (k_ata1)
};

// The row scan of a build kernel (one wave, `lane` of kWave): every segment of every grid row whose points the tile
// `g` of the output `B.dd` accepts, in a deterministic order.  B has the operator (A, Ainv: grid -> output and back),
// the grid's dimensions gd and the pull's field-of-view tolerance tol.  emit(pos, ui, uj, k0, len, za, zb) stores
// segment `pos` < CAP: points k0 .. k0 + len - 1 of row (ui, uj), za / zb = floor(gz) of its first / last point.
// Returns the number of segments found (the caller reports more than CAP as an error).
template <int MAXLEN, SegCut CUT, int CAP, class Args, class Emit>
__device__ __forceinline__ int sched_scan_rows(const Args &B, const TileBox &g, int lane, Emit emit) {
  const Dim3i dd = B.dd;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  // the aproned tile: a point is the tile's if its floor cell is in [x0 - 1, x0 + ex) (its 2 x 2 x 2 footprint
  // reaches into the tile proper or its apron's far side)
  const float flx = (float)(g.x0 - 1), fly = (float)(g.y0 - 1), flz = (float)(g.z0 - 1);
  const float fhx = (float)(g.x0 + g.ex), fhy = (float)(g.y0 + g.ey), fhz = (float)(g.z0 + g.ez);
  // acceptance box of a point: floor cell inside the aproned tile AND inside the field of view, as the pull tests it
  // (g > -tol  <=>  g >= nextafter(-tol); g < n - 1 + tol)
  const float tlo = nextafterf(-B.tol, 1.f);
  const float tlx = fmaxf(flx, tlo), tly = fmaxf(fly, tlo), tlz = fmaxf(flz, tlo);
  const float thx = fminf(fhx, (float)(dd.x - 1) + B.tol), thy = fminf(fhy, (float)(dd.y - 1) + B.tol),
              thz = fminf(fhz, (float)(dd.z - 1) + B.tol);
  // grid-space bounding box of everything that can touch the tile (the affine is convex: eight corners)
  float lo0 = 1e30f, lo1 = 1e30f, lo2 = 1e30f, hi0 = -1e30f, hi1 = -1e30f, hi2 = -1e30f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float ux, uy, uz;
    affine_point(B.Ainv, (c & 4) ? fhx : flx, (c & 2) ? fhy : fly, (c & 1) ? fhz : flz, ux, uy, uz);
    lo0 = fminf(lo0, ux), hi0 = fmaxf(hi0, ux);
    lo1 = fminf(lo1, uy), hi1 = fmaxf(hi1, uy);
    lo2 = fminf(lo2, uz), hi2 = fmaxf(hi2, uz);
  }
  // 0.01: Ainv is A's inverse in float - the box is widened by far more than its rounding, the shrink below is what
  // decides; along the row one more point each way, so that the shrink starts outside
  const int bx0 = max(0, (int)floorf(lo0 - 0.01f)), bx1 = min(B.gd.x - 1, (int)ceilf(hi0 + 0.01f));
  const int by0 = max(0, (int)floorf(lo1 - 0.01f)), by1 = min(B.gd.y - 1, (int)ceilf(hi1 + 0.01f));
  const int bz0 = max(0, (int)floorf(lo2 - 0.01f) - 1), bz1 = min(B.gd.z - 1, (int)ceilf(hi2 + 0.01f) + 1);
  const int nby = by1 - by0 + 1;
  const int nrow_cand = max(bx1 - bx0 + 1, 0) * max(nby, 0);
  const float c0 = B.A.m[2], c1 = B.A.m[6], c2 = B.A.m[10];
  int nseg = 0;
  for (int rc0 = 0; rc0 < nrow_cand; rc0 += kWave) {  // candidate rows: one per lane
    const int rc = rc0 + lane;
    int ui = 0, uj = 0, k0 = 0, k1 = -1;
    RowBase rb{0.f, 0.f, 0.f};
    if (rc < nrow_cand) {
      const int a = rc / nby, b = rc - a * nby;
      ui = bx0 + a, uj = by0 + b;
      rb = affine_row(B.A, (float)ui, (float)uj);
      k0 = bz0, k1 = bz1;
      // slab clipping in real arithmetic gives a superset (with slack) of the accepted interval ...
      //   1e-6: a row that does not move along an axis is tested against that slab as a whole, 0.01 wider than the
      //         box (more than its coordinate can differ from the exact one);
      //   +-1e6: keeps the quotients of a nearly parallel row inside what converts to int;
      //   2e-3 + 1e-5 |t|: the quotient's own error - absolute for the coordinates' rounding, relative for the
      //         division's - and one more point each way on top
      const float rr[3] = {rb.x + B.A.m[3], rb.y + B.A.m[7], rb.z + B.A.m[11]}, cc[3] = {c0, c1, c2};
      const float lw[3] = {flx, fly, flz}, hg[3] = {fhx, fhy, fhz};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (fabsf(cc[d]) > 1e-6f) {
          float ta = (lw[d] - rr[d]) / cc[d], tb = (hg[d] - rr[d]) / cc[d];
          const float tmin = fminf(ta, tb), tmax = fmaxf(ta, tb);
          ta = fmaxf(tmin, -1e6f), tb = fminf(tmax, 1e6f);
          k0 = max(k0, (int)ceilf(ta - 2e-3f - 1e-5f * fabsf(ta)) - 1);
          k1 = min(k1, (int)floorf(tb + 2e-3f + 1e-5f * fabsf(tb)) + 1);
        } else if (rr[d] < lw[d] - 0.01f || rr[d] >= hg[d] + 0.01f) {
          k1 = k0 - 1;
        }
      }
      // ... then exactly: the accepted points of a row form an interval (every rounding in sched_point is monotone
      // in k), so shrinking from both ends finds it
      auto accept = [&](int k) {
        float gx, gy, gz;
        sched_point(B.A, rb.x, rb.y, rb.z, (float)k, gx, gy, gz);
        return gx >= tlx && gx < thx && gy >= tly && gy < thy && gz >= tlz && gz < thz;
      };
      while (k0 <= k1 && !accept(k0)) ++k0;
      while (k1 >= k0 && !accept(k1)) --k1;
    }
    // cut into segments of <= MAXLEN points by CUT's rule; a round of the loop places one segment of every lane that
    // has one left, in lane order (ballot / popcount)
    int cur = k0;
    bool more = k1 >= k0;
    while (__any(more)) {
      int e = cur;
      float za = 0.f, zb = 0.f;
      if (more) {
        float gx, gy, gz;
        sched_point(B.A, rb.x, rb.y, rb.z, (float)cur, gx, gy, gz);
        float plz = floorf(gz);
        za = plz;
        while (e + 1 <= k1 && e + 1 - cur < MAXLEN) {
          sched_point(B.A, rb.x, rb.y, rb.z, (float)(e + 1), gx, gy, gz);
          const float lz = floorf(gz);
          if (CUT == SegCut::kPlaneRepeats ? lz == plz : lz != plz + 1.f) break;
          plz = lz;
          ++e;
        }
        zb = plz;
      }
      const unsigned long long m = __ballot(more);
      const int pos = nseg + __popcll(m & lt_mask);
      if (more && pos < CAP) emit(pos, ui, uj, cur, e - cur + 1, za, zb);
      nseg += __popcll(m);
      cur = e + 1;
      more = more && cur <= k1;
    }
  }
  return nseg;
}

// --------------------------------------------------------------------------
// host
// --------------------------------------------------------------------------
// How hard the schedule builders (splat2_build, ata1_build) of the calling thread try: thorough = rows closer than
// row_sep are tested point by point (a better lane fill, 2 - 4 x the build time); quick = kept apart wholesale.
// The plan builds thoroughly once (unires_plan_create) and quickly whenever an operator changes under a running
// reconstruction (unires_plan_set_repeat: every rigid Gauss-Newton step).
void sched_set_thorough(bool on);
bool sched_thorough();
// the `exact` flag of a build: what the kernel's environment switch forces (>= 0), else as the thread asks
inline int sched_exact(int forced) { return forced >= 0 ? forced : (sched_thorough() ? 1 : 0); }

// What both stream kernels ask of an operator: 32-bit indexing with room to spare (tile coordinates are packed into
// 10 - 16 bits, byte offsets into 32), and a splat that is race-free without atomics.
inline bool sched_in_domain(Dim3i gd, Dim3i dd, const SplatSafety &safe) {
  if (safe.use_atomics) return false;
  if (dd.x > 4000 || dd.y > 4000 || dd.z > 4000 || gd.x > 4000 || gd.y > 4000 || gd.z > 4000) return false;
  return fits_fast_index(gd) && fits_fast_index(dd) && dd.numel() < (1ull << 30);
}

// The processing order of a schedule's tiles.  ni[t] = instructions of tile t (index order: z fastest, then y, then
// x), a tile costs ni[t] + tile_cost (staging and epilogue).
//  (1) part_lo[0 .. np]: np contiguous runs of tiles of equal COST, one per partition (an XCD when the launch has
//      >= 8 workgroups) - with equal tile COUNTS the XCD that holds the volume's first x slabs had a third less to do.
//  (2) geom[0 .. nt): the tiles of each run, those with (next to) no instructions - at most half the maximum: the part
//      of the volume the observation does not see - LAST, emptiest at the very end: a wave's last round is as long
//      as its longest tile.  The others keep their index order (neighbours share halos and schedule lines in the
//      XCD's L2), or
//  (3) strip > 0: walk the run in strips of `strip` tiles along y (z fastest, then y inside the strip, then x, then
//      the next strip; nty, ntz = tiles along y and z), which puts a tile's x neighbour a strip-slab away instead of
//      a whole yz slab of tiles.
// keep_order: index order throughout (diagnostic).  geom[nt] = 0.
void sched_order(const unsigned *ni, int nt, double tile_cost, int np, int *part_lo, int *geom, int nty = 0,
                 int ntz = 0, int strip = 0, bool keep_order = false);

// Grow a device array to hold need + pad elements: nothing if it does; else free it and allocate an eighth more than
// asked (rebuilds of a moving operator need a little more or less each time).  False: out of memory, p = nullptr.
template <class T>
inline bool sched_grow(T *&p, size_t &cap, size_t need, size_t pad) {
  if (need + pad <= cap) return true;
  if (p) (void)hipFree(p);
  p = nullptr, cap = 0;
  const size_t n = need + need / 8 + pad;
  if (hipMalloc((void **)&p, n * sizeof(T)) != hipSuccess) return false;
  cap = n;
  return true;
}

// A schedule's scratch words on the device, {error flags, points, instructions}: made on first use and cleared for a
// build; read back after it.  False: no memory / the copy failed.
constexpr int kSchedScratchWords = 4;
bool sched_scratch_clear(unsigned long long *&scratch);
bool sched_scratch_read(const unsigned long long *scratch, int &err, unsigned long long stats[2]);

// Workgroups of the persistent launch of a kernel with `waves` tiles in flight per workgroup.  cap_env: the kernel's
// environment override; share_cap > 0: the caller runs other work next to it (channels of a y-update on streams of
// their own) and wants room left on the CUs - see unires_plan_set_concurrency (api_plan.hip).
inline int persistent_grid(int ntiles, int waves, int cap_env, int share_cap) {
  const int cap = cap_env > 0 ? cap_env : (share_cap >= 8 ? share_cap : 1024);
  const int want = (ntiles + waves - 1) / waves;
  return want < cap ? want : cap;
}

// Of a persistent grid of `grid` workgroups, those that take tiles: as many as the device holds AT ONCE (asked of
// the runtime once per kernel `fn`, `threads` per workgroup; force > 0 overrides the answer per CU), rounded down to
// whole rounds over the 8 XCDs.  *asked = the workgroups per CU, set only by the call that asked.
int resident_workgroups(const void *fn, int threads, int grid, int force, int *asked = nullptr);

}  // namespace unires
