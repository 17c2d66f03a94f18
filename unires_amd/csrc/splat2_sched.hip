// splat2_sched.hip - the schedule of k_splat2 (see splat2.hpp): the build kernels, the compaction of the one-pass
// build, its staging arrays and the host's splat2_build.  The row scan and the processing order are sched.hpp's.
#include "splat2_internal.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace unires {

#ifndef S2_INTERLEAVE
#define S2_INTERLEAVE 1
#endif

// --------------------------------------------------------------------------
// schedule build
// --------------------------------------------------------------------------
struct S2BuildArgs {
  Affine A, Ainv;
  Dim3i gd, dd;
  float tol;
  int row_sep;
  int axis, rows_y;
  const float4 *xtab, *ytab;  // axis 3
  Dim3i xd;
  int exact;  // close rows tested point by point (aligned schedules) instead of kept apart wholesale
};

struct S2Seg {
  short ui, uj, k0;
  unsigned char len, lzmin, lzmax, pad;  // local z planes touched: [lzmin, lzmax + 1]
};

__device__ __forceinline__ unsigned s2_rowcode(const S2BuildArgs &B, int ui, int uj) {
  return (B.axis == 0 || B.axis == 1 || B.axis == 3) ? ((unsigned)ui << 9) | (unsigned)uj
                                      : (unsigned)ui * (unsigned)B.rows_y + (unsigned)uj;
}

// One wave per tile.  MODE 0: counts[t] = {entries, instructions}; MODE 1: counts holds the exclusive prefix
// sums (of the instruction counts padded to whole batches) and the entries / masks / batch words are written where they belong (the two-pass build of rounds 2-4, kept as the
// fallback); MODE 2 (round 5): ONE pass - counts[t] as in MODE 0 AND the tile's entries / masks into its staging
// slot (kS2StageE entries, 64 masks per tile: entries, ext and masks point at the staging arrays), from where
// k_splat2_compact moves them once the host has fixed the processing order.  A tile with more entries than a slot
// holds raises bit 1 of *err: the caller falls back to MODE 1.
constexpr int kS2StageE = 128;
template <int MODE>
__global__ void __launch_bounds__(kWave)
    k_splat2_build(S2BuildArgs B, uint2 *__restrict__ counts, const int *__restrict__ geom,
                   S2Entry *__restrict__ entries, S2Ext *__restrict__ ext, ulonglong2 *__restrict__ masks,
                   unsigned *__restrict__ bwords, int *__restrict__ err, unsigned long long *__restrict__ stats) {
  using T = S2Tile;
  constexpr int kSegs = 384;
  __shared__ S2Seg segs[kSegs];
  __shared__ unsigned short member[kWave][kS2MaxSeg];
  const int lane = threadIdx.x;
  const int slot = blockIdx.x;                  // where this tile's counts / offsets live
  const int t = geom ? geom[slot] : slot;       // the output tile (FILL: processing order -> tile)
  const TileBox g = tile_box<T::TX, T::TY, T::TZ>(t, B.dd);
  const float c2 = B.A.m[10];
  // segments: <= L points, no two consecutive points in the same z plane
  int nseg = sched_scan_rows<T::L, SegCut::kPlaneRepeats, kSegs>(B, g, lane, [&](int pos, int ui, int uj, int k0, int len, float za, float zb) {
    const int la = (int)za - (g.z0 - 1), lb = (int)zb - (g.z0 - 1);
    segs[pos] = S2Seg{(short)ui, (short)uj, (short)k0, (unsigned char)len, (unsigned char)min(la, lb), (unsigned char)max(la, lb), 0};
  });
  if (nseg > kSegs) {
    if (lane == 0) atomicExch(err, 1);
    nseg = kSegs;
  }
  S2_FENCE();
  __syncthreads();
  // (r6) the slice of the conv_up table this tile needs: 64 consecutive entries from `kb` on - the tile's first grid
  // index along the table's axis (grid z for axis 2 / 3, ui / uj for axis 0 / 1).  The splat keeps one slice per wave in
  // LDS instead of the whole table per workgroup (6 - 8 KB: config 4's 385 entries pushed four 4-wave workgroups over
  // a CU's 160 KB).  Axis 2 / 3 entries carry k0 relative to kb.  A tile that spans more than 64: general kernels.
  int kb = 0;
  if (B.axis >= 0) {
    int lo = 1 << 30, hi = -(1 << 30);
    for (int s0 = 0; s0 < nseg; s0 += kWave) {
      const int s = s0 + lane;
      if (s < nseg) {
        const S2Seg q = segs[s];
        const int a = B.axis == 0 ? (int)q.ui : (B.axis == 1 ? (int)q.uj : (int)q.k0);
        const int b = (B.axis == 0 || B.axis == 1) ? a : a + (int)q.len - 1;
        lo = min(lo, a), hi = max(hi, b);
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off, kWave)), hi = max(hi, __shfl_xor(hi, off, kWave));
    if (nseg > 0) {
      kb = lo;
      if (hi - lo >= kWave && lane == 0) atomicOr(err, 1);
    }
  }
  const int kb_k = (B.axis == 2 || B.axis == 3) ? kb : 0;  // what the entries' k field is relative to
  // ---- packing into 64-lane instructions: lane b is instruction b of the tile ----
  // ALIGNED mode (every segment walks one z plane per point, i.e. |dz/dk| <= 1): within each
  // 32-lane half, lane position = z plane (31 - plane when z decreases along the row).  The
  // accumulator's x / y strides are multiples of 32 words, so the LDS bank of an update is its z
  // plane: lanes of one half then never collide on a bank, whatever rows they come from.
  // Otherwise segments are simply laid end to end.  Either way a segment joins the first
  // instruction that has room, fewer than kS2MaxSeg members and no member it could collide with
  // (rows closer than row_sep whose plane ranges touch).
  __shared__ unsigned short order[kSegs];
  // (lane 0's work arrays and the lanes' start lists live in LDS - the block is one wave; indexed at run time they
  // sat in scratch memory: 928 bytes per lane, build kernels 494 + 678 -> 454 + 556 us at 256^3)
  __shared__ int cnt[33];
  __shared__ unsigned short tmp[kSegs];
  __shared__ int start_all[kWave][kS2MaxSeg];
  bool al = true;
  for (int s0 = 0; s0 < nseg; s0 += kWave) {
    const int s = s0 + lane;
    if (s < nseg) al = al && ((int)segs[s].lzmax - (int)segs[s].lzmin + 1 == (int)segs[s].len);
  }
  const bool aligned = __all(al) && T::SZ == 32;
  const bool zdown = c2 < 0.f;
  auto seg_pos = [&](const S2Seg q) { return aligned ? (zdown ? 31 - (int)q.lzmax : (int)q.lzmin) : 0; };
  // stable counting sort by first lane position (one lane: deterministic schedule)
  if (lane == 0) {
    for (int i = 0; i < 33; ++i) cnt[i] = 0;
    for (int s = 0; s < nseg; ++s) ++cnt[seg_pos(segs[s]) + 1];
    for (int i = 0; i < 32; ++i) cnt[i + 1] += cnt[i];
    for (int s = 0; s < nseg; ++s) order[cnt[seg_pos(segs[s])]++] = (unsigned short)s;
#if S2_INTERLEAVE
    // ... offered to the first-fit below as 0, h, 1, h + 1, ... (h = half the count).  Most segments are
    // whole rows of the tile's ~9 x 5 cross-section - one per 32-lane half - and two rows share an
    // instruction only if they are >= row_sep apart: in scan order a row's successors are its
    // neighbours, the partner had to be found among rows offered much later, and the last ones found
    // none (26 instructions per config-3 tile for 44 segments).  Offered in this order the row half the
    // cross-section away - 4 to 5 rows over - comes right behind its partner.
    {
      const int h = (nseg + 1) / 2;
      for (int s = 0; s < nseg; ++s) tmp[s] = order[s];
      for (int s = 0; s < nseg; ++s) order[s] = tmp[(s & 1) ? h + (s >> 1) : (s >> 1)];
    }
#endif
  }
  S2_FENCE();
  __syncthreads();
  unsigned occ0 = 0u, occ1 = 0u;  // aligned: occupied lanes of each half; else: lanes used so far in occ0
  int nmem = 0, nbins = 0;
  for (int si = 0; si < nseg; ++si) {
    const int s = order[si];
    const S2Seg q = segs[s];
    const int a = seg_pos(q);
    const unsigned pm = (q.len >= 32 ? 0xffffffffu : ((1u << q.len) - 1u)) << a;
    bool free = true;
    for (int j = 0; j < nmem && free; ++j) {
      const S2Seg m = segs[member[lane][j] & 0x7fff];
      const bool rows_close = max(abs(m.ui - q.ui), abs(m.uj - q.uj)) < B.row_sep;
      const bool planes_touch = (int)m.lzmin <= (int)q.lzmax + 1 && (int)q.lzmin <= (int)m.lzmax + 1;
      if (!(rows_close && planes_touch)) continue;
      // (adjacent rows - at most one apart in both indices - overlap wherever they share a plane: no need to look)
      if (!(B.exact && aligned && !zdown) || max(abs(m.ui - q.ui), abs(m.uj - q.uj)) < 2) {
        free = false;
        break;
      }
      // (r5, as ata1.hip's packing) ... else exactly: two lanes meet only in the same read-add-write group on the
      // same z plane - two points with the same floor plane whose 2 x 2 cell footprints overlap.  Aligned segments
      // walk one plane per point, so the points that share plane pl are known: their floor cells are compared, in
      // the kernel's own arithmetic.  Rows two apart, which the blanket rule (row_sep 3 for a rotated operator)
      // keeps out of each other's instructions, almost always pass.
      const int lo = max((int)m.lzmin, (int)q.lzmin), hi = min((int)m.lzmax, (int)q.lzmax);
      const RowBase ra = affine_row(B.A, (float)m.ui, (float)m.uj), rq = affine_row(B.A, (float)q.ui, (float)q.uj);
      for (int pl = lo; pl <= hi; ++pl) {
        float ax, ay, az, bx, by, bz;
        sched_point(B.A, ra.x, ra.y, ra.z, (float)((int)m.k0 + pl - (int)m.lzmin), ax, ay, az);
        sched_point(B.A, rq.x, rq.y, rq.z, (float)((int)q.k0 + pl - (int)q.lzmin), bx, by, bz);
        // (The cells are floored as the STREAM kernel floors them, which differs between the two schedules on purpose.
        // k_splat2 floors the global coordinate - the tile's base enters as an integer offset of the accumulator's
        // address since round 6 took the subtraction in front of v_fract out - so this test floors that.  k_ata1
        // floors g - (tile0 - 1), and ata1.hip's test does: on the volume's low faces the two can differ.)
        if (fabsf(floorf(ax) - floorf(bx)) < 2.f && fabsf(floorf(ay) - floorf(by)) < 2.f) {
          free = false;
          break;
        }
      }
    }
    free = free && lane <= nbins && nmem < kS2MaxSeg;
    bool ok0, ok1;
    if (aligned) {
      ok0 = free && (occ0 & pm) == 0u, ok1 = free && (occ1 & pm) == 0u;
    } else {
      ok0 = free && (int)occ0 + q.len <= kWave, ok1 = false;
    }
    const unsigned long long m = __ballot(ok0 || ok1);
    if (m == 0ull) {  // more than 64 instructions in one tile
      if (lane == 0) atomicOr(err, 1);
      break;
    }
    const int chosen = __ffsll((long long)m) - 1;
    if (lane == chosen) {
      const int half = ok0 ? 0 : 1;
      member[lane][nmem++] = (unsigned short)(s | (half << 15));
      if (aligned) {
        if (half == 0) occ0 |= pm; else occ1 |= pm;
      } else {
        occ0 += q.len;
      }
    }
    nbins = max(nbins, chosen + 1);
  }
  const int nent = lane < nbins ? nmem : 0;
  // inclusive prefix sum of nent over lanes
  int incl = nent;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int v = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += v;
  }
  const int total_ent = __shfl(incl, kWave - 1, kWave);
  if (MODE != 1) {
    if (lane == 0) counts[slot] = make_uint2((unsigned)total_ent, (unsigned)nbins | ((unsigned)kb << 8));
    if (MODE == 0) return;
    if (total_ent > kS2StageE) {
      if (lane == 0) atomicOr(err, 2);
      return;
    }
  }
  const uint2 base = MODE == 1 ? counts[slot] : make_uint2((unsigned)slot * (unsigned)kS2StageE, (unsigned)slot * 64u);
  // The batch words (splat2.hpp): the ring slot of every instruction's first entry, and where the stream's segment ring
  // moves on - the rule the stream used to apply at run time: before batch b it advances by one chunk if the batch
  // reaches past the two chunks it holds.  Instructions past the tile's last (the padding) start at its end.
  {
    const int nb = (nbins + kS2Batch - 1) / kS2Batch;
    const int fe = lane < nbins ? incl - nent : total_ent;
    unsigned adv = 0u;
    int chunk_lo = 0;
    for (int b = 0; b < nb; ++b) {
      const int nx = kS2Batch * (b + 1);
      const int need = nx < nbins ? __shfl(fe, nx, kWave) : total_ent;
      if (need > 32 * (chunk_lo + 2)) adv |= 1u << b, ++chunk_lo;
    }
    unsigned w = 0u;
#pragma unroll
    for (int u = 0; u < kS2Batch; ++u) w |= ((unsigned)__shfl(fe, min(kS2Batch * lane + u, kWave - 1), kWave) & 63u) << (6 * u);
    if (lane < nb) bwords[base.y / kS2Batch + lane] = w | (((adv >> lane) & 1u) ? kS2BatchAdv : 0u);
    // padding: empty instructions
    if (lane >= nbins && lane < kS2Batch * nb) masks[base.y + lane] = make_ulonglong2(0ull, 0ull);
  }
  unsigned long long pts = 0;
  if (lane < nbins) {
    S2Entry *out = entries + base.x + (incl - nent);
    // members in lane order (aligned: by half, then position; else: as packed)
    int *start_of = start_all[lane];
    int run = 0;
    for (int j = 0; j < nmem; ++j) {
      const S2Seg q = segs[member[lane][j] & 0x7fff];
      start_of[j] = aligned ? 32 * (member[lane][j] >> 15) + seg_pos(q) : run;
      run += q.len;
    }
    for (int i = 1; i < nmem; ++i)  // insertion sort of (start, member) pairs
      for (int j = i; j > 0 && start_of[j] < start_of[j - 1]; --j) {
        const int ts = start_of[j];
        start_of[j] = start_of[j - 1], start_of[j - 1] = ts;
        const unsigned short tm = member[lane][j];
        member[lane][j] = member[lane][j - 1], member[lane][j - 1] = tm;
      }
    unsigned long long starts = 0ull, active = 0ull;
    for (int j = 0; j < nmem; ++j) {
      const S2Seg q = segs[member[lane][j] & 0x7fff];
      const int start = start_of[j];
      const RowBase rb = affine_row(B.A, (float)q.ui, (float)q.uj);
      S2Entry e;
      e.rx = rb.x, e.ry = rb.y, e.rz = rb.z;
      e.pk = s2_rowcode(B, q.ui, q.uj) | ((unsigned)(q.k0 - kb_k - start + 64) << kS2RowBits);
      out[j] = e;
      if (B.axis == 3) {  // x / y part of the conv_up of this row: 2 x 2 x-space columns
        const float4 tx = B.xtab[q.ui], ty = B.ytab[q.uj];
        S2Ext x;
        x.base4 = 4u * (((unsigned)__float_as_int(tx.x) * (unsigned)B.xd.y + (unsigned)__float_as_int(ty.x)) *
                        (unsigned)B.xd.z);
        x.w00 = tx.y * ty.y, x.w01 = tx.y * ty.z, x.w10 = tx.z * ty.y, x.w11 = tx.z * ty.z;
        x.pad[0] = x.pad[1] = x.pad[2] = 0u;
        ext[base.x + (incl - nent) + j] = x;
      }
      if (j > 0) starts |= 1ull << (start - 1);  // lanes >= start count it: slot = popcount below lane
      active |= (q.len >= 64 ? ~0ull : ((1ull << q.len) - 1ull)) << start;
      pts += q.len;
    }
    masks[base.y + lane] = make_ulonglong2(starts, active);
  }
  if (stats) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) pts += __shfl_down(pts, off, kWave);
    if (lane == 0) {
      atomicAdd(stats, pts);
      atomicAdd(stats + 1, (unsigned long long)nbins);
    }
  }
}

// Staging slot of tile geom[u] -> the schedule's arrays at processing slot u's offsets.
__global__ void __launch_bounds__(kWave)
    k_splat2_compact(const uint2 *__restrict__ stage_cnt, const S2Entry *__restrict__ stage_e,
                     const S2Ext *__restrict__ stage_x, const ulonglong2 *__restrict__ stage_m,
                     const unsigned *__restrict__ stage_b, const int *__restrict__ geom, const uint2 *__restrict__ tile_off,
                     S2Entry *__restrict__ entries, S2Ext *__restrict__ ext, ulonglong2 *__restrict__ masks,
                     unsigned *__restrict__ bwords) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int t = geom[u];
  const uint2 c = stage_cnt[t], o = tile_off[u];
  const uint4 *se = reinterpret_cast<const uint4 *>(stage_e) + (size_t)t * kS2StageE;
  uint4 *de = reinterpret_cast<uint4 *>(entries) + o.x;
  for (unsigned i = lane; i < c.x; i += kWave) de[i] = se[i];
  if (stage_x) {
    const uint4 *sx = reinterpret_cast<const uint4 *>(stage_x) + 2 * (size_t)t * kS2StageE;  // 32 bytes per entry
    uint4 *dx = reinterpret_cast<uint4 *>(ext) + 2 * (size_t)o.x;
    for (unsigned i = lane; i < 2u * c.x; i += kWave) dx[i] = sx[i];
  }
  const unsigned nb = ((c.y & 0xffu) + kS2Batch - 1) / kS2Batch;  // (.y: instructions | table base << 8)
  if ((unsigned)lane < kS2Batch * nb) masks[o.y + lane] = stage_m[(size_t)t * 64 + lane];
  if ((unsigned)lane < nb) bwords[o.y / kS2Batch + lane] = stage_b[(size_t)t * (64 / kS2Batch) + lane];
}

// Staging arrays of the single-pass build: one set per device, grown on demand, shared by every schedule built on it
// (a build holds the lock from its first kernel to its last: builds synchronise with the host anyway).
struct S2Stage {
  uint2 *cnt = nullptr;
  S2Entry *e = nullptr;
  S2Ext *x = nullptr;
  ulonglong2 *m = nullptr;
  unsigned *b = nullptr;  // 64 / kS2Batch batch words per tile
  size_t tiles = 0, tiles_x = 0;
};
static std::mutex g_stage_mu;
static std::map<int, S2Stage> g_stage;

static S2Stage *s2_stage(int nt, bool want_ext) {  // (call with g_stage_mu held) nullptr: use the two-pass build
  static const bool two_pass = getenv("UNIRES_S2_BUILD_2PASS") != nullptr;
  if (two_pass) return nullptr;
  const size_t bytes = (size_t)nt * (kS2StageE * (sizeof(S2Entry) + (want_ext ? sizeof(S2Ext) : 0)) + 64 * sizeof(ulonglong2) +
                                     (64 / kS2Batch) * sizeof(unsigned));
  if (bytes > (512ull << 20)) return nullptr;  // (a 1 000^3 volume: two passes rather than half a gigabyte of staging)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  S2Stage &G = g_stage[dev];
  if ((size_t)nt > G.tiles) {
    if (G.cnt) (void)hipFree(G.cnt);
    if (G.e) (void)hipFree(G.e);
    if (G.m) (void)hipFree(G.m);
    if (G.b) (void)hipFree(G.b);
    G.cnt = nullptr, G.e = nullptr, G.m = nullptr, G.b = nullptr, G.tiles = 0;
    const size_t n = (size_t)nt + nt / 8;
    if (hipMalloc((void **)&G.cnt, n * sizeof(uint2)) != hipSuccess ||
        hipMalloc((void **)&G.e, n * kS2StageE * sizeof(S2Entry)) != hipSuccess ||
        hipMalloc((void **)&G.m, n * 64 * sizeof(ulonglong2)) != hipSuccess ||
        hipMalloc((void **)&G.b, n * (64 / kS2Batch) * sizeof(unsigned)) != hipSuccess) {
      (void)hipGetLastError();
      if (G.cnt) (void)hipFree(G.cnt);
      if (G.e) (void)hipFree(G.e);
      if (G.m) (void)hipFree(G.m);
      if (G.b) (void)hipFree(G.b);
      G.cnt = nullptr, G.e = nullptr, G.m = nullptr, G.b = nullptr;
      return nullptr;
    }
    G.tiles = n;
  }
  if (want_ext && (size_t)nt > G.tiles_x) {
    if (G.x) (void)hipFree(G.x);
    G.x = nullptr, G.tiles_x = 0;
    const size_t n = (size_t)nt + nt / 8;
    if (hipMalloc((void **)&G.x, n * kS2StageE * sizeof(S2Ext)) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    G.tiles_x = n;
  }
  return &G;
}


void splat2_free(SplatSched &S) {
  if (S.entries) (void)hipFree(S.entries);
  if (S.ext) (void)hipFree(S.ext);
  if (S.masks) (void)hipFree(S.masks);
  if (S.bwords) (void)hipFree(S.bwords);
  if (S.tile_off) (void)hipFree(S.tile_off);
  if (S.tile_geom) (void)hipFree(S.tile_geom);
  if (S.recs) (void)hipFree(S.recs);
  if (S.scratch) (void)hipFree(S.scratch);
  S = SplatSched();
}

int splat2_build(SplatSched &S, const Affine &A, const Affine &Ainv, Dim3i gd, Dim3i dd, float tol,
                 const SplatSafety &safe, int axis, int rows_y, const float4 *xtab, const float4 *ytab,
                 Dim3i xd) {
  S.valid = false;
  static const bool off = getenv("UNIRES_NO_SPLAT2") != nullptr;
  static const bool verbose = getenv("UNIRES_SPLAT2_VERBOSE") != nullptr;
  if (off) return 1;
  if (!sched_in_domain(gd, dd, safe)) return 1;
  // the row code must fit its 19 bits (all ones is reserved)
  if (axis == 3 && (!xtab || !ytab)) return 1;
  if (axis == 0 || axis == 1 || axis == 3) {
    if (gd.x > 1023 || gd.y > 511) return 1;
  } else if ((long long)gd.x * rows_y >= (long long)kS2RowIdle || rows_y < gd.y) {
    return 1;
  }
  const int nt = s2_ntiles(dd);
  if ((size_t)nt + 1 > S.cap_tiles) {
    if (S.tile_off) (void)hipFree(S.tile_off);
    S.tile_off = nullptr;
    if (hipMalloc((void **)&S.tile_off, ((size_t)nt + 1) * sizeof(uint2)) != hipSuccess) return 1;
    if (S.tile_geom) (void)hipFree(S.tile_geom);
    S.tile_geom = nullptr;
    if (hipMalloc((void **)&S.tile_geom, ((size_t)nt + 1) * sizeof(int)) != hipSuccess) return 1;
    S.cap_tiles = (size_t)nt + 1;
  }
  if (!sched_scratch_clear(S.scratch)) return 1;
  int *err_dev = (int *)S.scratch;
  unsigned long long *stats_dev = S.scratch + 1;
  S2BuildArgs B;
  B.A = A, B.Ainv = Ainv, B.gd = gd, B.dd = dd, B.tol = tol, B.row_sep = safe.row_sep;
  B.axis = axis, B.rows_y = rows_y;
  B.xtab = xtab, B.ytab = ytab, B.xd = xd;
  static const int exact = getenv("UNIRES_S2_EXACT") ? atoi(getenv("UNIRES_S2_EXACT")) : -1;  // (-1: as the plan asks)
  B.exact = sched_exact(exact);
  // One pass into per-tile staging slots + a compaction once the order is known (round 5; the schedule is the
  // two-pass build's, bit for bit - tests/test_gpu_selection.py); two passes where there is no staging or a tile
  // does not fit its slot.  unires_plan_set_repeat runs this for every channel after every rigid update.
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);
  S2Stage *stage = s2_stage(nt, axis == 3);
  std::vector<uint2> cnt((size_t)nt), h((size_t)nt + 1);
  if (stage) {
    hipLaunchKernelGGL(k_splat2_build<2>, dim3(nt), dim3(kWave), 0, 0, B, stage->cnt, (const int *)nullptr, stage->e,
                       axis == 3 ? stage->x : (S2Ext *)nullptr, stage->m, stage->b, err_dev, stats_dev);
    int e0 = 0;
    if (hipMemcpy(cnt.data(), stage->cnt, (size_t)nt * sizeof(uint2), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (hipMemcpy(&e0, err_dev, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (e0 & 2) {  // a tile overflowed its slot: two passes (the counts are good)
      stage = nullptr;
      (void)sched_scratch_clear(S.scratch);
      if (e0 & 1) (void)hipMemset(err_dev, 1, 1);
    }
  } else {
    hipLaunchKernelGGL(k_splat2_build<0>, dim3(nt), dim3(kWave), 0, 0, B, S.tile_off, (const int *)nullptr,
                       (S2Entry *)nullptr, (S2Ext *)nullptr, (ulonglong2 *)nullptr, (unsigned *)nullptr, err_dev,
                       (unsigned long long *)nullptr);
    if (hipMemcpy(cnt.data(), S.tile_off, (size_t)nt * sizeof(uint2), hipMemcpyDeviceToHost) != hipSuccess)
      return 1;
  }
  // (the build kernel packs the tile's table base above its instruction count)
  std::vector<int> kbv((size_t)nt);
  std::vector<unsigned> ni((size_t)nt);
  for (int i = 0; i < nt; ++i) kbv[i] = (int)(cnt[i].y >> 8), cnt[i].y &= 0xffu, ni[i] = cnt[i].y;
  // Processing order (sched_order: (1) runs of equal cost per partition, (2) cheap tiles last, (3) y strips).  A tile
  // costs its instructions + 11 for the epilogue (~5 us against ~0.45 us per instruction, tools/s2_timeline.py); the
  // tiles with (next to) no instructions are 14 % of config 3, and a wave gets 4.5 tiles, so the last round is half
  // empty and as long as its longest tile: made of 5 us tiles instead of 16 us ones the kernel's tail shrinks by two
  // thirds.
  constexpr double kEpilogueCost = 11.0;
  std::vector<int> geom((size_t)nt + 1);
  // the launch this schedule is laid out for: `nwg` workgroups take tiles, partition x (an XCD when there are >= 8)
  // is served by the workgroups b with b % np == x
  const int nwg = s2_active(axis, s2_grid(dd));
  const int np = std::min(8, std::max(nwg, 1));
  std::vector<int> part_lo((size_t)np + 1, nt);
  using T = S2Tile;
  const int nty = (dd.y + T::TY - 1) / T::TY, ntz = (dd.z + T::TZ - 1) / T::TZ;
  {
    static const bool keep_order = getenv("UNIRES_SPLAT2_INDEX_ORDER") != nullptr;
    // The y strips.  In index order (z fastest, then y, then x) a tile's x neighbour comes a whole yz slab of
    // tiles later: 8 x 256 x 256 floats of p = 2.1 MB at 256^3, 4.7 MB at 384^3 - with q, the x-space rows and the
    // schedule lines that go by in between, more than the XCD's 4 MB of L2 keeps: the x halos of the epilogue's
    // stencil window came from the fabric again.  Strips put the x neighbour one strip-slab (~1 MB) away; only
    // the strips' border rows are fetched twice.  Measured (channel 1, PMC): k_splat2 fetches 169.7 -> 143.4 MB
    // per launch at config 3, 677 -> 561 MB at 384^3; its time does not move (it is not bandwidth-bound) - this is
    // about not wasting fabric traffic.  (The same walk on k_ata1's 4 x 4 tiles: no change, 1 MB slabs fit anyway.)
    static const int strip_env = getenv("UNIRES_S2_STRIP") ? atoi(getenv("UNIRES_S2_STRIP")) : -1;
    const int strip = strip_env >= 0 ? strip_env
                                     : (int)std::max<long long>(4, (1ll << 20) / ((long long)T::TX * T::TY * dd.z * 8));
    sched_order(ni.data(), nt, kEpilogueCost, np, part_lo.data(), geom.data(), nty, ntz, strip, keep_order);
  }
  // (4) Who takes which tile: wave slot s of a partition (S slots) walks positions s, s + S, s + 2 S, ... of the order
  // above - waves sweep the run together, and a wave knows its next tile a tile ahead (its header is prefetched).
  // Round 6 measured two ways of levelling the waves' ends (4.33 tiles per wave at config 3: a third of the waves have a
  // fifth 14 us tile, the rest end at 59 of 72 us, and a wave's end follows the predicted sum of its tiles' costs,
  // correlation 0.94 over 4 096 waves - tools/s2_timeline.py) and dropped both:
  //  * dealing the last (partial, or also the last whole) round AT BUILD TIME to the slots with the least predicted
  //    work, longest first: 72.2 us where round-robin has 70.2 on the unrotated channel, no change on the rotated ones;
  //  * a ticket queue for the tiles that do not fill a round (one L2 atomic per draw, 16 counters per XCD - atomics on
  //    ONE address are served ~30 ns apart: 512 waves drawing from one counter cost the kernel 17 - 50 us): 72.1 / 72.4 us
  //    against 71.2 / 68.7 static.
  // A CU's 16 waves share its issue slots: what a wave does not use the others get, so what counts is the work per CU -
  // which round-robin over workgroups that the dispatcher deals over the CUs levels by itself.
  std::vector<int> pos_tile(geom.begin(), geom.begin() + nt);  // position -> tile
  for (int xc = 0; xc <= 8; ++xc) S.pos_lo[xc] = part_lo[(size_t)std::min(xc, np)];
  S.nwg = nwg;
  // offsets in position order (geom: the u-th tile in that order, for the compaction / fill kernels)
  std::vector<uint4> recs(pos_tile.size() + 1, make_uint4(0xffffffffu, 0u, 0u, 0u));
  unsigned re = 0, ri = 0;
  {
    int u = 0;
    for (size_t pp = 0; pp < pos_tile.size(); ++pp) {
      const int g = pos_tile[pp];
      if (g < 0) continue;
      const uint2 cg = cnt[g];
      const unsigned tzi = (unsigned)(g % ntz), tyi = (unsigned)((g / ntz) % nty), txi = (unsigned)(g / (ntz * nty));
      const unsigned npad = (cg.y + kS2Batch - 1) / kS2Batch * kS2Batch;  // (whole batches: empty instructions)
      recs[pp] = make_uint4(txi | (tyi << 10) | (tzi << 20), re, ri, cg.y | ((unsigned)kbv[g] << 8));
      geom[u] = g;
      h[u] = make_uint2(re, ri);
      re += cg.x, ri += npad;
      ++u;
    }
    if (u != nt) return 1;  // (every tile exactly once)
    h[nt] = make_uint2(re, ri);
    geom[nt] = 0;
  }
  constexpr size_t kPad = 160;  // entries read (never used) past the end by the ring prefetch
  {
    const size_t cap_was = S.cap_entries;
    if (!sched_grow(S.entries, S.cap_entries, (size_t)re, kPad)) return 1;
    if (S.cap_entries != cap_was && S.ext) {  // (as long as the entries)
      (void)hipFree(S.ext);
      S.ext = nullptr;
    }
  }
  if (axis == 3 && !S.ext) {
    if (hipMalloc((void **)&S.ext, S.cap_entries * sizeof(S2Ext)) != hipSuccess) return 1;
    (void)hipMemset(S.ext, 0, S.cap_entries * sizeof(S2Ext));
  }
  if (!sched_grow(S.masks, S.cap_instr, (size_t)ri, 8)) return 1;
  if (!sched_grow(S.bwords, S.cap_batches, (size_t)ri / kS2Batch, 8)) return 1;
  if (hipMemcpy(S.tile_off, h.data(), ((size_t)nt + 1) * sizeof(uint2), hipMemcpyHostToDevice) != hipSuccess)
    return 1;
  if (hipMemcpy(S.tile_geom, geom.data(), ((size_t)nt + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return 1;
  if (!sched_grow(S.recs, S.cap_recs, recs.size(), 0)) return 1;
  if (hipMemcpy(S.recs, recs.data(), recs.size() * sizeof(uint4), hipMemcpyHostToDevice) != hipSuccess) return 1;
  (void)hipMemset(S.entries + re, 0xff, kPad * sizeof(S2Entry));
  (void)hipMemset(S.masks + ri, 0, 8 * sizeof(ulonglong2));
  (void)hipMemset(S.bwords + ri / kS2Batch, 0, 8 * sizeof(unsigned));
  if (stage)
    hipLaunchKernelGGL(k_splat2_compact, dim3(nt), dim3(kWave), 0, 0, (const uint2 *)stage->cnt, (const S2Entry *)stage->e,
                       axis == 3 ? (const S2Ext *)stage->x : (const S2Ext *)nullptr, (const ulonglong2 *)stage->m,
                       (const unsigned *)stage->b, (const int *)S.tile_geom, (const uint2 *)S.tile_off, S.entries, S.ext,
                       S.masks, S.bwords);
  else
    hipLaunchKernelGGL(k_splat2_build<1>, dim3(nt), dim3(kWave), 0, 0, B, S.tile_off, (const int *)S.tile_geom,
                       S.entries, S.ext, S.masks, S.bwords, err_dev, stats_dev);
  int herr = 0;
  unsigned long long hs[2] = {0, 0};
  if (!sched_scratch_read(S.scratch, herr, hs)) return 1;
  if (herr & 1) {
    if (verbose) fprintf(stderr, "[splat2] a tile exceeds the segment / instruction lists: general kernel used\n");
    return 1;
  }
  S.ntiles = nt;
  S.axis = axis;
  S.fill = hs[1] ? (double)hs[0] / (64.0 * (double)hs[1]) : 0.0;
  S.valid = true;
  if (verbose) {
    // (also: which build ran - one pass through the staging slots or, a tile overflowing its slot, two - the most
    // instructions in one tile, and how many tiles end at each residue mod 4 of their instruction count)
    unsigned imax = 0, res4[4] = {0, 0, 0, 0};
    for (int i = 0; i < nt; ++i) imax = std::max(imax, cnt[i].y), ++res4[cnt[i].y & 3u];
    fprintf(stderr, "[splat2] %d tiles, %llu instructions, %u segments, %llu points (%.2f per output voxel), "
            "lane fill %.3f, schedule %.1f MB, row_sep %d, build %s, max instructions per tile %u, "
            "tiles by instructions mod 4 %u %u %u %u\n", nt, hs[1], re, hs[0],
            (double)hs[0] / (double)dd.numel(), S.fill, (re * sizeof(S2Entry) + ri * 16.0) / 1e6, safe.row_sep,
            stage ? "one-pass" : "two-pass", imax, res4[0], res4[1], res4[2], res4[3]);
  }
  return 0;
}

void splat2_convtab(const Taps &T, const Scaling &S, int axis, int gn, int xdn, float *out) {
  const int K = T.n[axis], s = T.s[axis];
  const float se = S.dim == axis ? S.e : 1.f, so = S.dim == axis ? S.o : 1.f;
  for (int u = 0; u < gn; ++u) {
    int khi = u / s;
    if (khi > xdn - 1) khi = xdn - 1;
    const int tt = u - K + 1;
    const int klo = tt <= 0 ? 0 : (tt + s - 1) / s;
    const int n = khi - klo + 1;
    float w0 = 0.f, w1 = 0.f;
    if (n >= 1) w0 = T.t[axis][u - s * klo] * ((klo & 1) ? so : se);
    if (n >= 2) w1 = T.t[axis][u - s * (klo + 1)] * (((klo + 1) & 1) ? so : se);
    int koff = n < 1 ? 0 : klo;
    if (koff > xdn - 2) {  // last slice: the pair (xdn-2, xdn-1), weight on the second
      koff = xdn - 2;
      w1 = w0, w0 = 0.f;
    }
    memcpy(&out[4 * u], &koff, 4);
    out[4 * u + 1] = w0, out[4 * u + 2] = w1, out[4 * u + 3] = 0.f;
  }
}

}  // namespace unires
