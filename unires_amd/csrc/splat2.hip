// splat2.hip - schedule-driven owner-computes push (see splat2.hpp).
//
// Race freedom without atomics (LDS float atomics cost ~190 clocks per wave-instruction on
// gfx950, tools/mb_lds.hip): a tile is owned by ONE wave, whose LDS operations execute in
// order; inside one read-add-write group
//   * the lanes of a segment sit in DIFFERENT z planes (the build kernel cuts a row wherever two
//     consecutive points share floor(gz)), and a group touches one plane per lane: the lower
//     plane of every point first, the upper plane second;
//   * the segments packed into one instruction either come from rows >= row_sep apart
//     (host-checked for the affine: some coordinate of any two of their points differs by >= 2)
//     or occupy z-plane ranges that do not touch.
// The schedule is fixed, so results are bit-reproducible.
//
// What the hardware charges (tools/mb_valu.hip, tools/mb_lds.hip, MI355X): a wave64 add / mul
// issues in 2 clocks, FMA / convert / shift / compare in 4; an 8-cell read-add-write costs the CU's
// LDS ~43 clocks; every VMEM wave-instruction costs the texture addresser ~16 clocks however
// well it coalesces.  Hence: segment descriptors go through an LDS ring (one coalesced global load
// per 32 segments), not per-lane global loads; ONE 8-byte source load per lane and instruction.
#include "splat2_internal.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace unires {

// phase-ablation switches: compiled in only with -DUNIRES_ABLATE (then UNIRES_S2_DBG selects bits:
// 1 no splat, 2 no epilogue, 4 no LDS updates, 8 no source loads); product builds carry none of it
#ifdef UNIRES_ABLATE
#define S2_ABL(bit) ((P.dbg & (bit)) != 0)
#else
#define S2_ABL(bit) (false)
#endif

int s2_grid(Dim3i dd, int share_cap) {
  static const int cap_env = getenv("UNIRES_SPLAT2_BLOCKS") ? atoi(getenv("UNIRES_SPLAT2_BLOCKS")) : 0;
  return persistent_grid(s2_ntiles(dd), kS2Waves, cap_env, share_cap);
}

// --------------------------------------------------------------------------
// the splat
// --------------------------------------------------------------------------
struct S2Args {
  const float *src;
  size_t src_bytes;
  const float4 *tab;     // conv_up table (AXIS >= 0)
  int gn;                // entries in it
  unsigned row_stride4;  // bytes per unit of the row code (see launch_splat2)
  unsigned tab_step4;    // bytes between the two x-space values of a grid voxel
  const S2Entry *entries;
  size_t ent_bytes;      // (bytes behind it: LDS-DMA goes through a buffer resource)
  const S2Ext *ext;      // AXIS 3
  unsigned xs_sy4, xs_sx4;  // AXIS 3: bytes between x-space rows / slabs
  const ulonglong2 *masks;  // per instruction: {segment starts, active lanes}
  const unsigned *bwords;   // per batch of kS2Batch instructions: ring slots, ring advance (splat2.hpp)
  const uint4 *recs;     // per position of the walk: {tile, entry offset, instruction offset, instructions | table base << 8}
  int ntiles;
  Affine A;
  float alpha;
  const float *p;
  float a0, cx, cy, cz;
  float *dst;
  Dim3i dd;
  int accumulate;
  double *partials;
  const float *objb;
  int dbg;  // UNIRES_S2_DBG ablation bits (read only by -DUNIRES_ABLATE builds)
  int prio_rot;  // rotate the waves' issue priority per tile (UNIRES_S2_PRIO=0 switches it off)
  int xlo[9];  // position range [xlo[x], xlo[x + 1]) of partition x (an XCD when the grid has >= 8 workgroups)
  int active;  // workgroups that take tiles (the rest of the grid only clears its partials)
  unsigned long long *prof;  // -DUNIRES_S2_PROF builds: per-wave timeline (100 MHz ticks)
  // residual mode (PushEpilogue::res_r; objb = b, OBJK kernels only): r = b - q to res_r, z = r [/ res_M] to res_p,
  // partials = sum r z; q is not stored.  Last in the struct: every other field sits where it sat.
  float *res_r, *res_p;
  const float *res_M;
  double *partials2;  // residual mode, nullable: sum obj_term(q, b, p), the start's objective, in the slots of `partials`
};

// OBJK: the launch evaluates the CG objective (P.objb set: q is not stored) - a kernel of its own since r6, so that the
// sixteen extra rows its epilogue holds do not decide the register allocation of the form every CG iteration runs.
// The same kernel serves the start of a CG solve (P.res_r set): with A(x0) in registers and b in its rows it writes the
// residual and the first direction and sums r.z, where k_residual_init read A(x0) and b back.
template <int AXIS, int NW, bool OBJK>
__global__ void __launch_bounds__(kWave *NW) __attribute__((amdgpu_waves_per_eu(4, 4))) k_splat2(S2Args P, const int *__restrict__ done) {
  if (done && *done) return;
  using T = S2Tile;
  constexpr int TX = T::TX, TY = T::TY, L = T::L, G = kWave / L;
  constexpr int SY = T::SY, SZ = T::SZ, N = T::N, XS = T::XS, YS = T::YS;
  constexpr bool CONV = AXIS >= 0;
  // (one struct, so that the layout is the one written: each wave's ring and table slice are 1 KB on a 1 KB boundary,
  // and slot (i & 63) of either is  base | ((i << 4) & 0x3f0)  - an add-shift and an and-or where the indexed form costs
  // an and, a shift-add and, for the ring, an add)
  struct __align__(1024) Lds {
    uint4 ring[NW][kWave];  // 2 chunks of 32 segment entries
    // CONV: the 64 entries of the conv_up table from the tile's base on, {grid coordinate as a float, byte offset,
    // alpha w0, alpha w1}, one slice per wave, refilled per tile (r6; was the whole table per workgroup)
    float4 tabs[CONV ? NW : 1][kWave];
    float acc[NW][N];
    uint4 ring2[AXIS == 3 ? NW : 1][AXIS == 3 ? 2 * kWave : 1];  // AXIS 3: the entries' S2Ext
  };
  __shared__ Lds lds;
  static_assert(sizeof(uint4) * kWave == 1024, "ring / table slices are addressed as 1 KB blocks");
  auto &acc_all = lds.acc;
  auto &ring_all = lds.ring;
  auto &ring2_all = lds.ring2;
  auto &tabs_all = lds.tabs;
  const int lane = threadIdx.x & (kWave - 1), grp = lane / L, gl = lane & (L - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *acc = acc_all[wave];
  uint4 *ring = ring_all[wave];
  uint4 *ring2 = ring2_all[AXIS == 3 ? wave : 0];
  float4 *tabs = tabs_all[CONV ? wave : 0];
  const Dim3i dd = P.dd;
  // (r6) What only a tile's header and epilogue want - pointers, buffer ranges, the stencil's coefficients - is NOT held
  // in scalar registers through the instruction stream: held, it did not fit (96 scalar values parked in the lanes of
  // two VGPRs, ~75 v_readlane + their hazard waits per tile - VALU issues, what this kernel runs out of).  It is read
  // again from the kernel-argument segment, by scalar load, through a pointer laundered per tile (S2Args is the
  // kernel's first parameter: offset 0 of the segment).
  typedef const __attribute__((address_space(4))) S2Args *KArgs;
  auto kargs = [&]() {
    KArgs k = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
#ifndef UNIRES_S2_NO_KARG
    asm volatile("" : "+s"(k));
#endif
    return k;
  };
  const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(P.src, P.src_bytes);
  // XCD-aware persistent schedule: workgroup b sits on XCD b % 8; each XCD walks one contiguous
  // run of tiles so that neighbouring tiles (shared stencil halos, schedule lines) share an L2.
  // (Tried and dropped: a contiguous, cost-balanced range of tiles per wave - 103 us instead of
  // 95 us: waves that sweep the run together share cache lines, waves far apart do not.)
  // Only as many workgroups as the chip holds AT ONCE take tiles (P.active, a multiple of 8): the table
  // above is part of the workgroup's LDS, and with 384 + 128 entries a CU holds three workgroups, not
  // four - the fourth quarter of a 1024-workgroup grid then started when the first three were done and
  // the kernel took twice a workgroup's time (config 4: 424 us where 16.5 M points cost 81 us in config 3).
  if ((int)blockIdx.x >= P.active) {
    if (P.partials && lane == 0) P.partials[blockIdx.x * NW + wave] = 0.0;
    if (OBJK && P.partials2 && lane == 0) P.partials2[blockIdx.x * NW + wave] = 0.0;
    return;
  }
  const int nwg = P.active;
  const int nxcd = min(8, nwg);
  const int xcd = blockIdx.x % nxcd;
  const int t_lo = P.xlo[xcd], t_hi = P.xlo[xcd + 1];
  const int slot = (blockIdx.x / nxcd) * NW + wave;
  const int slots = ((nwg + nxcd - 1 - xcd) / nxcd) * NW;
  const float c0 = P.A.m[2], c1 = P.A.m[6], c2 = P.A.m[10];
  const float t0 = P.A.m[3], t1 = P.A.m[7], t2 = P.A.m[11];
  const int lane_m64 = lane - 64;
  typedef unsigned u4r __attribute__((ext_vector_type(4)));
  typedef float f4r __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(3))) u4r *LdsU4;
  typedef const __attribute__((address_space(3))) f4r *LdsF4;
  const unsigned ring_b = (unsigned)(__UINTPTR_TYPE__)(LdsU4)(const void *)ring, tabs_b = (unsigned)(__UINTPTR_TYPE__)(LdsF4)(const void *)tabs;
  unsigned m3f0 = 0x3f0u;  // (in a register: with the base in a scalar register the literal would be a second constant)
  asm volatile("" : "+v"(m3f0));
  typedef float v2k __attribute__((ext_vector_type(2)));
  v2k k_one0 = {1.f, 0.f};  // (likewise: the packed weight pairs' second constant, else re-made in front of every use)
  asm volatile("" : "+v"(k_one0));
  double dot = 0.0;
  double dot2 = 0.0;  // (residual mode with the objective; OBJK kernels only)
#ifdef UNIRES_S2_PROF
  unsigned long long *pw = P.prof ? P.prof + (size_t)(blockIdx.x * NW + wave) * 32 : nullptr;
  int ptile = 0;
  if (pw && lane == 0) pw[0] = wall_clock64();
#endif
  // The SIMD's arbiter issues from its OLDEST wave first: of the four waves that share a SIMD the
  // first to arrive ran its instruction stream at 0.43 us per instruction, the last at 0.62 us - same
  // work, and the youngest waves set the kernel time.  User priority beats age, so every wave walks
  // through the four priorities, one per tile, starting from its slot on the SIMD: over a wave's 4.5
  // tiles the four of a SIMD are each first, second, third and last once: 81.8 -> 76.8 us.  (Rotating
  // every 8 instructions instead: 80.7 us - strict priorities are the efficient way to run, it is
  // the fixed ranking that unbalances.)
  const int hw_slot = (int)(__builtin_amdgcn_s_getreg(6148) & 3u);  // HW_ID.wave_id
  int round = 0;
  // (r6) The walk.  A tile's 16-byte record comes by SCALAR load (constant address space: the schedule is read-only),
  // the next tile's one is requested as a tile starts and travels under its stream.  What a tile needs per LANE before
  // its first instruction - the masks of instruction `lane`, the first 64 segment entries, its slice of the conv_up
  // table - is requested at the head of the PREVIOUS tile's epilogue and lands under it: three dependent trips to
  // memory (tile -> offsets -> masks / entries) stood at the head of every tile, 1.6 of its 14 us.
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  const __attribute__((address_space(4))) u4v *recs = (const __attribute__((address_space(4))) u4v *)P.recs;
  const u4v rec_none = {0xffffffffu, 0u, 0u, 0u};
  int t = t_lo + slot;
  u4v rec = t < t_hi ? recs[t] : rec_none;
  // The entries and the table slice go straight into LDS (LDS-DMA: lane l's 16 bytes land on bytes 16 l of the ring /
  // the slice - no register carried through the epilogue); the masks' load is issued AFTER them, so that the wait
  // the compiler puts in front of the masks' first use covers both (loads return in order).
  ulonglong2 h_mk = make_ulonglong2(0ull, 0ull);
  unsigned h_bw = 0u;
  struct Hdr {  // what a header request wants of the kernel arguments
    const S2Entry *entries;
    size_t ent_bytes;
    const float4 *tab;
    int gn;
    const ulonglong2 *masks;
    const unsigned *bwords;
  };
  auto load_hdr = [&](KArgs K) { return Hdr{K->entries, K->ent_bytes, K->tab, K->gn, K->masks, K->bwords}; };
  auto issue_header = [&](const Hdr &H, const u4v &rc, int ln) {
    const int ni = (int)(rc.w & 0xffu);
    const int np = AXIS == 2 ? (ni + kS2Batch - 1) / kS2Batch * kS2Batch : ni;  // (AXIS 2 streams the padding too)
    const int gn = H.gn;
    const __amdgpu_buffer_rsrc_t rs_ent = make_rsrc(H.entries, H.ent_bytes);
    S2_FENCE();
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_ent, (__attribute__((address_space(3))) void *)ring, 16,
                                             16u * (rc.y + (unsigned)ln), 0, 0, 0);
    if (CONV) {
      const __amdgpu_buffer_rsrc_t rs_tab = make_rsrc(H.tab, (size_t)gn * sizeof(float4));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_tab, (__attribute__((address_space(3))) void *)tabs, 16,
                                               16u * (unsigned)min(max((int)(rc.w >> 8) + ln, 0), gn - 1), 0, 0, 0);
    }
    S2_FENCE();
    // (every lane loads - lanes past the tile's last instruction read the zero padding or a later tile's masks, never
    // used: an unconditional load is always issued, and the wait on it is what orders the DMA above)
    h_mk = H.masks[rc.z + (unsigned)min(ln, max(np - 1, 0))];
    if (AXIS == 2) h_bw = H.bwords[rc.z / (unsigned)kS2Batch + (unsigned)min(ln, max(np / kS2Batch - 1, 0))];
  };
  if (rec.x != 0xffffffffu) issue_header(load_hdr(kargs()), rec, lane);
  for (; rec.x != 0xffffffffu; ++round) {
    if (P.prio_rot) {
      switch ((hw_slot + round) & 3) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
      }
    }
    const int x0 = (int)(rec.x & 1023u) * TX, y0 = (int)((rec.x >> 10) & 1023u) * TY, z0 = (int)(rec.x >> 20) * T::TZ;
    const int ex = min(TX, dd.x - x0), ey = min(TY, dd.y - y0), ez = min(T::TZ, dd.z - z0);
    // (AXIS 2: whole batches, the build's empty instructions included)
    const int ninstr = AXIS == 2 ? ((int)(rec.w & 0xffu) + kS2Batch - 1) / kS2Batch * kS2Batch : (int)(rec.w & 0xffu);
    const int tab_base = (int)(rec.w >> 8);
    const unsigned ent0 = rec.y;
    const uint4 *E = reinterpret_cast<const uint4 *>(P.entries) + ent0;  // (used through the stream: stays in registers)
    const int t_next = t + slots;
    const u4v rec_next = t_next < t_hi ? recs[t_next] : rec_none;
    // lane l keeps the masks of instruction l (a tile has at most 64 of them) and the word of batch l
    int lp = lane;  // (laundered per tile, as in the epilogue: the prologue's addresses are not held through the stream)
    asm volatile("" : "+v"(lp));
    const ulonglong2 mymask = h_mk;
    const int mlo_v = (int)(unsigned)mymask.x, mhi_v = (int)(unsigned)(mymask.x >> 32);
    const int alo_v = (int)(unsigned)mymask.y, ahi_v = (int)(unsigned)(mymask.y >> 32);
    const int bw_v = (int)h_bw;
    // the batch words (AXIS 2) / the masks are here => so are the ring's chunks 0 and 1 and the table slice (issued before them)
    if (AXIS == 2)
      asm volatile("" ::"v"(mlo_v), "v"(mhi_v), "v"(alo_v), "v"(ahi_v), "v"(bw_v) : "memory");
    else
      asm volatile("" ::"v"(mlo_v), "v"(mhi_v), "v"(alo_v), "v"(ahi_v) : "memory");
    // segment ring: chunk 2 in flight in registers
    uint4 pre = make_uint4(0u, 0u, 0u, 0u);
    if (lp < 32) pre = E[64 + lp];
    if (CONV) {
      // (.x = the grid coordinate the entry belongs to, as a float: the z-profile kernels take k from the table
      // instead of converting it, and the 16-byte read costs the LDS 4 cycles where the 12-byte one costs 8)
      const unsigned step4 = (AXIS == 2 || AXIS == 3) ? 4u : P.tab_step4;  // the per-lane table runs along z
      const float4 raw = tabs[lp];
      // (as the stream reads it: {grid coordinate, byte offset, alpha w0, alpha w1} - the coordinate FIRST, in the even
      // register of the 16-byte read, where the packed coordinate arithmetic takes it without a move)
      tabs[lp] = make_float4((float)(tab_base + lp), __int_as_float((int)(step4 * (unsigned)__float_as_int(raw.x))),
                             P.alpha * raw.y, P.alpha * raw.z);
    }
#ifdef UNIRES_S2_PROF
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // per tile: {header here, stream end, p window here, end, instructions}
    if (pw && lane == 0 && ptile < 5) pw[3 + 5 * ptile] = wall_clock64();
#endif
    const uint4 *X = reinterpret_cast<const uint4 *>(P.ext) + 2 * (size_t)ent0;  // AXIS 3: 2 uint4 per entry
    uint4 pre2 = make_uint4(0u, 0u, 0u, 0u);
    if (AXIS == 3) {
      ring2[lane] = X[lane], ring2[kWave + lane] = X[kWave + lane];
      pre2 = X[2 * kWave + lane];  // chunk 2 = 32 entries = 64 uint4
    }
    {
      // (the zeros and the lane's address are made HERE, per tile: kept live across the instruction stream as loop
      // invariants they cost five of its 128 registers, and the allocator parked them in scratch memory)
      int lz = lane;
      float zr = 0.f;
      asm volatile("" : "+v"(lz), "+v"(zr));
      for (int i = lz; i < N / 4; i += kWave) reinterpret_cast<float4 *>(acc)[i] = make_float4(zr, zr, zr, zr);
    }
    // accumulator cell of global floor cell (fx, fy, fz): acc_t[(fx * SY + fy) * SZ + fz]
    // (the offset is laundered: left to itself the compiler folds its constant part, XS + YS + 1, into the immediate
    // offsets of the eight LDS accesses, which then no longer fit their 8 bits - two more address additions per
    // splat instruction; opaque, the four cells sit at 0 / YS / XS / XS + YS (+ 1) <= 225 dwords from ONE address)
    // (... and the accumulator's own LDS address goes in with it: one scalar byte address per tile)
    typedef __attribute__((address_space(3))) float *LdsF1;
    unsigned acc_addr = (unsigned)(__UINTPTR_TYPE__)(LdsF1)(void *)acc - 4u * (unsigned)(((x0 - 1) * SY + (y0 - 1)) * SZ + (z0 - 1));
    asm volatile("" : "+s"(acc_addr));
    int chunk_lo = 0;  // the ring holds chunks chunk_lo and chunk_lo + 1 (32 entries each)
    int eb = 0;        // (running decode, AXIS != 2) first entry of the next instruction, relative to the tile
    S2_FENCE();
    constexpr int kU = kS2Batch;
    // (Tried and dropped: a schedule whose groups of 2 / 4 consecutive instructions are mutually
    // conflict-free, so that their LDS updates run as two rounds with all reads of a round in
    // flight - the extra packing constraint costs lane fill (0.75 -> 0.65 / 0.40) and the round form
    // 20-30 more VGPRs (occupancy 4 -> 3 waves per SIMD): 155 us instead of 88 us.)
    // A batch = kU instructions (the build pads a tile to whole batches with empty instructions).  Its word (splat2.hpp)
    // says where each instruction's entries start in the ring and whether the ring moves on first: advance(), then
    // fetch(): segment-start masks -> mbcnt -> segment entry (LDS ring) -> conv_up table -> ONE source load per lane and
    // instruction, all issued back to back; splat(): coordinates, weights and the two LDS update groups.  Two batches
    // are in flight: the source loads of batch b + 1 travel while batch b is splatted.
    struct Batch {
      float w0[kU], w1[kU], s0[kU], s1[kU], gx[kU], gy[kU], gz[kU];  // (coordinates, not their four ingredients: a register less per slot)
      unsigned long long amask[kU];
    };
    auto advance = [&](unsigned bw) {
      if (bw & kS2BatchAdv) {  // advance the ring by one chunk (the oldest one is dead)
        S2_FENCE();
        if (lane < 32) ring[(chunk_lo & 1) * 32 + lane] = pre;
        if (AXIS == 3) ring2[(chunk_lo & 1) * 64 + lane] = pre2;
        ++chunk_lo;
        int la = lane;  // (laundered: 16 * lane is not to be held through the tile loop - it ended up in scratch memory)
        asm volatile("" : "+v"(la));
        if (la < 32) pre = E[32 * (chunk_lo + 2) + la];
        if (AXIS == 3) pre2 = X[64 * (chunk_lo + 2) + lane];
        S2_FENCE();
      }
    };
    // slot u of a batch from ring slot `sl` (mod 64) of the lane's segment entry: entry -> conv_up table -> source load
    auto load = [&](Batch &Bt, int u, int sl) {
      {
        const u4r e = *(LdsU4)(__UINTPTR_TYPE__)((((unsigned)sl << 4) & m3f0) | ring_b);
        const float rx = __uint_as_float(e.x), ry = __uint_as_float(e.y), rz = __uint_as_float(e.z);
        float kf;
        const unsigned code = e.w & kS2RowIdle;
        // (idle lanes in front of an instruction's first segment see k < its k0: the tables carry 64
        // zero entries in front for them)
        // (axis 2 / 3: k relative to the tile's table base - the index into its slice for every active lane)
        const int k = (int)(e.w >> kS2RowBits) + lane_m64;
        kf = (float)k;
        Bt.w0[u] = P.alpha, Bt.w1[u] = 0.f, Bt.s0[u] = 1.f, Bt.s1[u] = 0.f;
        if (S2_ABL(8)) {
        } else if (AXIS == 3) {
          // conv_up along x, y and z: 2 x 2 x-space columns (per segment) x the z pair (per lane)
          const uint4 xa = ring2[2 * (sl & 63)], xb = ring2[2 * (sl & 63) + 1];
          const f4r tb = *(LdsF4)(__UINTPTR_TYPE__)((((unsigned)k << 4) & m3f0) | tabs_b);
          const unsigned a = xa.x + (unsigned)__float_as_int(tb.y);
          const uint2 p00 = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, a, 0, 0));
          const uint2 p01 = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, a + P.xs_sy4, 0, 0));
          const uint2 p10 = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, a + P.xs_sx4, 0, 0));
          const uint2 p11 =
              __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, a + P.xs_sx4 + P.xs_sy4, 0, 0));
          const float z00 = tb.z * __uint_as_float(p00.x) + tb.w * __uint_as_float(p00.y);
          const float z01 = tb.z * __uint_as_float(p01.x) + tb.w * __uint_as_float(p01.y);
          const float z10 = tb.z * __uint_as_float(p10.x) + tb.w * __uint_as_float(p10.y);
          const float z11 = tb.z * __uint_as_float(p11.x) + tb.w * __uint_as_float(p11.y);
          Bt.w0[u] = 1.f;
          kf = tb.x;
          Bt.s0[u] = __uint_as_float(xa.y) * z00 + __uint_as_float(xa.z) * z01 + __uint_as_float(xa.w) * z10 +
                     __uint_as_float(xb.x) * z11;
          (void)code;
        } else if (AXIS == 2) {
          const f4r tb = *(LdsF4)(__UINTPTR_TYPE__)((((unsigned)k << 4) & m3f0) | tabs_b);
          kf = tb.x;
          const unsigned a = __umul24(code, P.row_stride4) + (unsigned)__float_as_int(tb.y);
          const uint2 pr = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, a, 0, 0));
          Bt.w0[u] = tb.z, Bt.w1[u] = tb.w, Bt.s0[u] = __uint_as_float(pr.x), Bt.s1[u] = __uint_as_float(pr.y);
        } else if (AXIS == 0 || AXIS == 1) {
          const unsigned ui = code >> 9, uj = code & 511u;
          const float4 tb = tabs[((int)(AXIS == 0 ? ui : uj) - tab_base) & 63];
          const unsigned a = __umul24(AXIS == 0 ? uj : ui, P.row_stride4) + (unsigned)__float_as_int(tb.y) +
                             4u * (unsigned)k;
          Bt.w0[u] = tb.z, Bt.w1[u] = tb.w;
          Bt.s0[u] = buf_load(rsrc, a, 0), Bt.s1[u] = buf_load(rsrc, a + P.tab_step4, 0);
        } else {
          Bt.s0[u] = buf_load(rsrc, __umul24(code, P.row_stride4) + 4u * (unsigned)k, 0);
        }
#ifndef UNIRES_S2_NO_PKXY
        {
          // x and y as ONE packed pair per instruction (the entry's {rx, ry} arrive adjacent from the ring): left to
          // itself the vectoriser pairs the same coordinate of two batch slots and pays eleven moves per batch for it
          typedef float v2f __attribute__((ext_vector_type(2)));
          const v2f cxy = {c0, c1}, txy = {t0, t1}, rxy = {rx, ry}, kk = {kf, kf};
          const v2f gxy = __builtin_elementwise_fma(cxy, kk, rxy) + txy;
          Bt.gx[u] = gxy.x, Bt.gy[u] = gxy.y;
        }
#else
        Bt.gx[u] = fmaf(c0, kf, rx) + t0;
        Bt.gy[u] = fmaf(c1, kf, ry) + t1;
#endif
        Bt.gz[u] = fmaf(c2, kf, rz) + t2;
      }
    };
    // AXIS 2: the batch word's ring slots
    auto fetch = [&](Batch &Bt, int p0, unsigned bw) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int pi = p0 + u;
        const unsigned mlo = (unsigned)__builtin_amdgcn_readlane(mlo_v, pi), mhi = (unsigned)__builtin_amdgcn_readlane(mhi_v, pi);
        Bt.amask[u] = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(ahi_v, pi) << 32) |
                      (unsigned)__builtin_amdgcn_readlane(alo_v, pi);
        // ring slot of the lane's entry: the instruction's first slot (the batch word) + segments started below the lane
        // (added after mbcnt, not as its accumulator: a second scalar operand of one VOP3 costs a move on gfx9)
        load(Bt, u, (int)((bw >> (6 * u)) & 63u) + (int)__builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u)));
      }
    };
    // the other forms: a running count of the segments, slots past the tile's last instruction replay it switched off
    auto fetch_run = [&](Batch &Bt, int p0) {
      unsigned mlo[kU], mhi[kU];
      int ebu[kU];
      int need = eb;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int pi = min(p0 + u, ninstr - 1);
        mlo[u] = (unsigned)__builtin_amdgcn_readlane(mlo_v, pi);
        mhi[u] = (unsigned)__builtin_amdgcn_readlane(mhi_v, pi);
        Bt.amask[u] = p0 + u < ninstr ? ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(ahi_v, pi) << 32) |
                                            (unsigned)__builtin_amdgcn_readlane(alo_v, pi)
                                      : 0ull;
        ebu[u] = (p0 + u < ninstr || u == 0) ? need : ebu[u > 0 ? u - 1 : 0];
        if (p0 + u < ninstr) need += __popc(mlo[u]) + __popc(mhi[u]) + 1;
      }
      advance(need > 32 * (chunk_lo + 2) ? kS2BatchAdv : 0u);
      eb = need;
#pragma unroll
      for (int u = 0; u < kU; ++u)
        load(Bt, u, ebu[u] + (int)__builtin_amdgcn_mbcnt_hi(mhi[u], __builtin_amdgcn_mbcnt_lo(mlo[u], 0u)));
    };
    // (Tried and dropped: the four weight products and the eight accumulate FMAs as v_pk_mul_f32 /
    // v_pk_fma_f32 on the (y, y + 1) pairs the ds_read2 / ds_write2 carry - 6 VALU instructions less
    // per splat instruction, 129 VGPRs (128 when forced), and 79-83 us where this form has 76-83.)
    auto splat = [&](const Batch &Bt, auto second_tag) {
      constexpr bool SECOND = decltype(second_tag)::value;  // bb, the second batch of the loop
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float gx = Bt.gx[u], gy = Bt.gy[u], gz = Bt.gz[u];
        // floor cell and weights exactly as the pull computes them (floor, then g - floor: the build kernel's
        // collision tests floor the same global coordinate); the tile's base enters once, as an integer offset of
        // the accumulator pointer (r6: was a subtraction per coordinate in front of v_fract - three instructions
        // more, and exact only for tiles off the volume's low faces)
#ifndef UNIRES_S2_NO_PKW
        // (r6, with the registers the build without the SLP vectoriser left free - packed, this form needed 129 of 128 in
        // round 3.)  The weights as PAIRS: {wx0, wx1} and {wy0, wy1} come out of one packed fma each ({-1, 1} w + {1, 0}: the
        // same single rounding as 1 - w, and w itself), v {wx0, wx1}, then {a00, a01} = vx0 {wy0, wy1} and {a10, a11} = vx1
        // {wy0, wy1} are packed multiplies, and the accumulator's (y, y + 1) pairs arrive from ds_read2_b32 as register
        // pairs: one packed fma per pair where there were two.  21 vector instructions per splat instruction instead of 29,
        // every product and sum rounded exactly as before.
        typedef float v2f __attribute__((ext_vector_type(2)));
        const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
        const v2f gxy = {gx, gy}, fxy = {fx, fy};
        const v2f w1 = gxy - fxy;  // {wx1, wy1}
        const float wz1 = gz - fz, wz0 = 1.f - wz1;
        const v2f m11 = {-1.f, 1.f}, one0 = k_one0;
        const v2f wx = __builtin_elementwise_fma(m11, (v2f){w1.x, w1.x}, one0);  // {wx0, wx1}
        const v2f wy = __builtin_elementwise_fma(m11, (v2f){w1.y, w1.y}, one0);  // {wy0, wy1}
        // cell index in float (exact: integers below 2^24), one conversion
        const float cf = fmaf(fx, (float)XS, fmaf(fy, (float)YS, fz));
        const int cell = (int)cf;
        // (AXIS 0 / 1 / 2: the contraction spelled out, as the previous form of this kernel was compiled - slot 0 of the
        // first batch and every slot of the second one fma(w1, s1, w0 s0), slots 1 - 3 of the first fma(w0, s0, w1 s1) -
        // so that results stay bit-identical; left to itself the compiler picks per slot, and picked differently.  For
        // AXIS -1 / 3 one of the two products is 0 x 0 and the order does not matter.)
        float v;
        if (AXIS < 0 || AXIS == 3)
          v = Bt.w0[u] * Bt.s0[u] + Bt.w1[u] * Bt.s1[u];
        else if (!SECOND && u > 0)
          v = fmaf(Bt.w0[u], Bt.s0[u], Bt.w1[u] * Bt.s1[u]);
        else
          v = fmaf(Bt.w1[u], Bt.s1[u], Bt.w0[u] * Bt.s0[u]);
        const v2f vx = (v2f){v, v} * wx;                 // {vx0, vx1}
        const v2f a0 = (v2f){vx.x, vx.x} * wy, a1 = (v2f){vx.y, vx.y} * wy;  // {a00, a01}, {a10, a11}
        S2_FENCE();
        if (S2_ABL(4)) dot += (double)(a0.x + a0.y + a1.x + a1.y + (float)cell);
        if (__builtin_amdgcn_inverse_ballot_w64(Bt.amask[u]) && !S2_ABL(4)) {
          const LdsF1 q = (LdsF1)(__UINTPTR_TYPE__)(acc_addr + 4u * (unsigned)cell);
          {
            const v2f o0 = {q[0], q[YS]}, o1 = {q[XS], q[XS + YS]};
            const v2f r0 = __builtin_elementwise_fma(a0, (v2f){wz0, wz0}, o0), r1 = __builtin_elementwise_fma(a1, (v2f){wz0, wz0}, o1);
            q[0] = r0.x, q[YS] = r0.y, q[XS] = r1.x, q[XS + YS] = r1.y;
          }
          S2_FENCE();
          {
            const v2f o0 = {q[1], q[YS + 1]}, o1 = {q[XS + 1], q[XS + YS + 1]};
            const v2f r0 = __builtin_elementwise_fma(a0, (v2f){wz1, wz1}, o0), r1 = __builtin_elementwise_fma(a1, (v2f){wz1, wz1}, o1);
            q[1] = r0.x, q[YS + 1] = r0.y, q[XS + 1] = r1.x, q[XS + YS + 1] = r1.y;
          }
        }
#else
        const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
        const float wx1 = gx - fx, wy1 = gy - fy, wz1 = gz - fz;
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1, wz0 = 1.f - wz1;
        // cell index in float (exact: integers below 2^24), one conversion
        const float cf = fmaf(fx, (float)XS, fmaf(fy, (float)YS, fz));
        const int cell = (int)cf;
        const float v = Bt.w0[u] * Bt.s0[u] + Bt.w1[u] * Bt.s1[u];
        const float vx0 = v * wx0, vx1 = v * wx1;
        const float a00 = vx0 * wy0, a01 = vx0 * wy1, a10 = vx1 * wy0, a11 = vx1 * wy1;
        S2_FENCE();
        if (S2_ABL(4)) dot += (double)(a00 + a01 + a10 + a11 + (float)cell);
        if (__builtin_amdgcn_inverse_ballot_w64(Bt.amask[u]) && !S2_ABL(4)) {
          const LdsF1 q = (LdsF1)(__UINTPTR_TYPE__)(acc_addr + 4u * (unsigned)cell);
          {
            const float o00 = q[0], o01 = q[YS], o10 = q[XS], o11 = q[XS + YS];
            q[0] = o00 + a00 * wz0, q[YS] = o01 + a01 * wz0, q[XS] = o10 + a10 * wz0,
            q[XS + YS] = o11 + a11 * wz0;
          }
          S2_FENCE();
#ifdef S2_EXP_MASKB
          if ((lane & (S2_EXP_MASKB - 1)) == 0)  // (measurement only, wrong results: what a mostly-masked second group costs)
#endif
          {
            const float o00 = q[1], o01 = q[YS + 1], o10 = q[XS + 1], o11 = q[XS + YS + 1];
            q[1] = o00 + a00 * wz1, q[YS + 1] = o01 + a01 * wz1, q[XS + 1] = o10 + a10 * wz1,
            q[XS + YS + 1] = o11 + a11 * wz1;
          }
        }
#endif
        S2_FENCE();
      }
    };
    if (ninstr > 0 && !S2_ABL(1)) {
      // (Measured, r2: the branches around the fetches make the compiler's wait-count pass put
      // s_waitcnt vmcnt(0) in front of every splat, so a batch also waits for the source loads of
      // the next one.  A branch-free body - fetch / splat / fetch / splat with slots past the end
      // switched off - gets vmcnt(4..7) there and is no faster, 92 vs 90 us: the stream is not bound
      // by that latency but by VALU issue (~58 % of a SIMD) and LDS (~57 % of a CU) together, see
      // tools/s2_timeline.py.  Same outcome for a dynamic tile queue (also on top of the cheap-tiles-last
      // order: ends bunch up, 64 .. 80 us, but the ticket in front of the epilogue's loads costs each
      // epilogue 1 us), a staggered start of half the waves and a prefetch of the next tile's schedule.)
      Batch ba, bb;
      auto step = [&](Batch &Bt, int p0) {
        if (AXIS == 2) {
          const unsigned bw = (unsigned)__builtin_amdgcn_readlane(bw_v, p0 / kU);
          advance(bw);
          fetch(Bt, p0, bw);
        } else {
          fetch_run(Bt, p0);
        }
      };
      step(ba, 0);
      for (int p0 = 0; p0 < ninstr; p0 += 2 * kU) {
        const bool more = p0 + kU < ninstr;
        if (more) step(bb, p0 + kU);
        splat(ba, std::false_type{});
        if (more) {
          if (p0 + 2 * kU < ninstr) step(ba, p0 + 2 * kU);
          splat(bb, std::true_type{});
        }
      }
    }
    S2_FENCE();
#ifdef UNIRES_S2_PROF
    if (pw && lane == 0 && ptile < 5) pw[4 + 5 * ptile] = wall_clock64(), pw[7 + 5 * ptile] = (unsigned long long)ninstr;
#endif
    // ---- epilogue: q = [q +] acc + a0 p + c DtD p ; dot += p*q  (one row per lane group) ----
    // the next tile's per-lane header: requested now, it lands under this epilogue
    // (ALL of the epilogue's scalars are requested here, ahead of the branch around the header request, and pinned: one
    // trip to the scalar cache per tile - they came in two, the second one behind the header's loads)
    const KArgs K = kargs();
    const Hdr H = load_hdr(K);
    const float *__restrict__ pin = K->p;
    float *__restrict__ dst = K->dst;
    const float *objb = OBJK ? K->objb : nullptr;
    const int accumulate = K->accumulate;
    const float kcx = K->cx, kcy = K->cy, kcz = K->cz, ka0 = K->a0;
    asm volatile("" ::"s"(H.entries), "s"(H.ent_bytes), "s"(H.tab), "s"(H.gn), "s"(H.masks), "s"(H.bwords), "s"(pin), "s"(dst), "s"(objb),
                 "s"(accumulate), "s"(kcx), "s"(kcy), "s"(kcz), "s"(ka0));
    float *res_r = OBJK ? K->res_r : nullptr, *res_p = OBJK ? K->res_p : nullptr;
    const float *res_M = OBJK ? K->res_M : nullptr;
    const bool res_obj = OBJK && K->partials2 != nullptr;
    if (OBJK) asm volatile("" ::"s"(res_r), "s"(res_p), "s"(res_M));
    {
      // (the ring's chunk in flight may never have been used: let it land NOW, or the compiler waits for everything -
      // the header included - the first time the epilogue writes one of its registers)
      asm volatile("" ::"v"(pre.x), "v"(pre.y), "v"(pre.z), "v"(pre.w));
      if (AXIS == 3) asm volatile("" ::"v"(pre2.x), "v"(pre2.y), "v"(pre2.z), "v"(pre2.w));
      int lh = lane;
      asm volatile("" : "+v"(lh));
      if (rec_next.x != 0xffffffffu) issue_header(H, rec_next, lh);
    }
    double dtile = 0.0;  // this tile's part of the dot
    double dtile2 = 0.0;
    const bool fast_xy = !S2_ABL(2) && pin != nullptr && !accumulate && ex == TX && ey == TY && dd.numel() < (1ull << 29);
    if (fast_xy) {
      // Whole tiles, wherever they lie: x / y stencil neighbours outside the volume read as zeros
      // through an out-of-range buffer offset (the volume's first and last x slabs are a quarter of
      // the tiles of the XCDs that own them, and a wave whose stride lands it on the first or last
      // y row of tiles got four 12 us generic epilogues in a row).  Lane gl of a group holds
      // z plane z0 - 1 + gl of the aproned tile; group g owns x slabs 4g .. 4g + 3.  Every row of p
      // the group's stencils touch is loaded ONCE (32 loads per tile instead of 7 per output row);
      // the z neighbours come from the adjacent lanes (DPP wave shifts), the x / y neighbours from
      // the other registers.  Buffer addressing: a per-lane byte offset computed once per tile +
      // scalar row offsets.
      static_assert(TX == 8 && TY == 4 && G == 2, "epilogue register window is written for 8 x 4 tiles");
      // (r6) Instruction count is what this kernel runs out of, so the epilogue is written to be short:
      //  * no selects for the volume's faces: a neighbour that the reference's forward differences do not see is
      //    loaded from the CENTRE's own address (c - c = 0: the absent backward term of the first slab / row / plane),
      //    a neighbour beyond the last slab / row / plane from an out-of-range offset (0: the zero bound);
      //  * every difference once: p[s + 1] - p[s] is the forward term of s and the backward term of s + 1; along z the
      //    difference of adjacent lanes is one DPP subtraction, and (backward - forward) a second one;
      //  * the 16 accumulator reads issued together, ahead of the arithmetic; no branch per output row (lanes of the
      //    z apron store to an out-of-range offset and add nothing to the dot).
      // (lane-dependent values of the epilogue are derived from a laundered copy of the lane index, so that none of
      // them is hoisted out of the tile loop and held in a register through the instruction stream)
      int le = lane;
      asm volatile("" : "+v"(le));
      const int gl = le & (L - 1), grp = le / L;
      const int kz = z0 - 1 + gl;
      const bool out_z = gl >= 1 && gl <= ez;
      // (the 24 row offsets below are scalar sums of these two: as loop invariants of the tile loop they were computed
      // once, could not all be held through the stream and came back from VGPR lanes - 58 v_readlane + their hazard
      // waits per epilogue; laundered per tile they are made here by the scalar unit)
      unsigned sxb = 4u * (unsigned)(dd.y * dd.z), syb = 4u * (unsigned)dd.z;
      asm volatile("" : "+s"(sxb), "+s"(syb));
      constexpr unsigned kOob = 0x80000000u;
      const int xg = x0 + 4 * grp;
      // byte offset of (first owned slab, first owned row, plane kz): plane -1 reads plane 0 (so that the backward
      // difference of plane 0 comes out as zero), planes >= dd.z read zeros
      const unsigned e0 = 4u * (unsigned)((xg * dd.y + y0) * dd.z + max(kz, 0));
      const unsigned e1 = kz < dd.z ? e0 : kOob;
      const unsigned elo = xg > 0 ? e1 - sxb : e1, ehi = xg + 4 < dd.x ? e1 : kOob;
      const unsigned eyl = y0 > 0 ? e1 - syb : e1, eyh = y0 + TY < dd.y ? e1 : kOob;
      const unsigned est = out_z ? e0 : kOob;
      const __amdgpu_buffer_rsrc_t rp = make_rsrc(pin, dd.numel() * 4),
                                   rd = make_rsrc(dst, dd.numel() * 4),
                                   rb = make_rsrc(objb ? objb : pin, dd.numel() * 4);
      // (residual mode: out-of-range lanes store nowhere, as with q; a mode without the diagonal never loads through rm)
      const __amdgpu_buffer_rsrc_t rrr = make_rsrc(res_r ? res_r : dst, dd.numel() * 4),
                                   rrp = make_rsrc(res_p ? res_p : dst, dd.numel() * 4),
                                   rm = make_rsrc(res_M ? res_M : pin, dd.numel() * 4);
      const float *arow = acc + ((4 * grp + 1) * SY + 1) * SZ + gl;
      float pv[6][6];  // pv[s + 1][ly + 1]: x slab s = -1 .. 4, row ly = -1 .. 4 (corners unused)
#pragma unroll
      for (int sa = 0; sa < 6; ++sa)
#pragma unroll
        for (int la = 0; la < 6; ++la) {
          const bool halo_x = sa == 0 || sa == 5, halo_y = la == 0 || la == 5;
          // (the low halos sit at the centre's own row offsets when they alias it: first slab / first row)
          pv[sa][la] = (halo_x && halo_y) ? 0.f
                       : sa == 0 ? buf_load(rp, elo, (unsigned)(la - 1) * syb)
                       : sa == 5 ? buf_load(rp, ehi, 4u * sxb + (unsigned)(la - 1) * syb)
                       : la == 0 ? buf_load(rp, eyl, (unsigned)(sa - 1) * sxb)
                       : la == 5 ? buf_load(rp, eyh, (unsigned)(sa - 1) * sxb + 4u * syb)
                                 : buf_load(rp, e1, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
        }
#ifdef UNIRES_S2_PROF
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (pw && lane == 0 && ptile < 5) pw[5 + 5 * ptile] = wall_clock64();
#endif
      auto rows = [&](auto obj_tag) {
        constexpr bool OBJ = decltype(obj_tag)::value;
        // x and y differences, each once: p[s + 1][l] - p[s][l] is the forward term of slab s and the backward term of s + 1
        float dxp[4];
#pragma unroll
        for (int la = 1; la <= 4; ++la) dxp[la - 1] = pv[1][la] - pv[0][la];
        double dt = 0.0, dt2 = 0.0;
#pragma unroll
        for (int sa = 1; sa <= 4; ++sa) {
          float dy[5], av[4];  // (the slab's four accumulator reads issued together, ahead of its arithmetic)
#pragma unroll
          for (int la = 1; la <= 4; ++la) av[la - 1] = arow[((sa - 1) * SY + (la - 1)) * SZ];
          float ob[4];  // (objective form: b of the slab's rows, requested per slab - all sixteen up front did not fit the registers)
          if (OBJ) {
#pragma unroll
            for (int la = 1; la <= 4; ++la) ob[la - 1] = buf_load(rb, e1, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
          }
          float om[4] = {1.f, 1.f, 1.f, 1.f};  // (residual mode with the Jacobi diagonal: M of the slab's rows)
          if (OBJ && res_M) {
#pragma unroll
            for (int la = 1; la <= 4; ++la) om[la - 1] = buf_load(rm, e1, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
          }
#pragma unroll
          for (int la = 0; la <= 4; ++la) dy[la] = pv[sa][la + 1] - pv[sa][la];
#pragma unroll
          for (int la = 1; la <= 4; ++la) {
            const float c = pv[sa][la];
            // zf = p[k + 1] - p[k] (lane + 1 minus this lane); zbk = the same difference one lane down
            const float vzp = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(c), 0x130, 0xf, 0xf, true));
            const float zf = vzp - c;
            const float zbk = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(zf), 0x138, 0xf, 0xf, true));
            const float xf = pv[sa + 1][la] - c, xbk = dxp[la - 1];
            dxp[la - 1] = xf;
            const float yf = dy[la], ybk = dy[la - 1];
            const float st = kcx * (xbk - xf) + kcy * (ybk - yf) + kcz * (zbk - zf);
            const float q = av[la - 1] + (ka0 * c + st);
            if (OBJ && res_r) {
              const float r = __fsub_rn(ob[la - 1], q);
              const float z = res_M ? __fdiv_rn(r, om[la - 1]) : r;
              buf_store(r, rrr, est, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
              buf_store(z, rrp, est, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
              dt += (double)__fmul_rn(r, z);
              if (res_obj) dt2 += (double)obj_term(q, ob[la - 1], c);
            } else if (OBJ) {
              dt += (double)obj_term(q, ob[la - 1], c);
            } else {
              buf_store(q, rd, est, (unsigned)(sa - 1) * sxb + (unsigned)(la - 1) * syb);
              dt += (double)__fmul_rn(c, q);
            }
          }
        }
        dtile = out_z ? dt : 0.0;
        if (OBJ) dtile2 = out_z ? dt2 : 0.0;
      };
      rows(std::integral_constant<bool, OBJK>{});
    } else if (!S2_ABL(2)) {
      int lg = lane;  // (laundered: see the fast form)
      asm volatile("" : "+v"(lg));
      const int gl = lg & (L - 1), grp = lg / L;
#pragma unroll 2
      for (int r = grp; r < TX * TY; r += G) {
        const int lx = r / TY, ly = r % TY, lz = gl;
        if (lx >= ex || ly >= ey || lz >= ez) continue;
        const int i = x0 + lx, j = y0 + ly, k = z0 + lz;
        const size_t idx = ((size_t)i * dd.y + j) * dd.z + k;
        float q = acc[((lx + 1) * SY + ly + 1) * SZ + lz + 1];
        float pc = 0.f;
        if (pin) {
          const float st = dtd_at(pin, idx, i, j, k, dd, kcx, kcy, kcz, pc);
          q += ka0 * pc + st;
        }
        if (accumulate) q += dst[idx];
        if (OBJK && res_r) {
          const float r = __fsub_rn(objb[idx], q);
          const float z = res_M ? __fdiv_rn(r, res_M[idx]) : r;
          res_r[idx] = r, res_p[idx] = z;
          dtile += (double)__fmul_rn(r, z);
          if (res_obj) dtile2 += (double)obj_term(q, objb[idx], pc);
          continue;
        }
        matvec_emit(dst, idx, q, pc, objb, P.partials != nullptr, dtile);
      }
    }
#ifdef UNIRES_S2_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (pw && lane == 0 && ptile < 5) pw[6 + 5 * ptile] = wall_clock64();
    ++ptile;
#endif
    dot += dtile;
    if (OBJK) dot2 += dtile2;
    t = t_next, rec = rec_next;
  }
#ifdef UNIRES_S2_PROF
  if (pw && lane == 0) pw[1] = wall_clock64(), pw[2] = (unsigned long long)ptile;
#endif
  if (P.partials) {
    const double tot = wave_sum(dot);
    if (lane == 0) P.partials[blockIdx.x * NW + wave] = tot;
  }
  if (OBJK && P.partials2) {
    const double tot2 = wave_sum(dot2);
    if (lane == 0) P.partials2[blockIdx.x * NW + wave] = tot2;
  }
}

int splat2_blocks(Dim3i dd, int grid_cap) { return s2_grid(dd, grid_cap) * kS2Waves; }  // partials written

// Workgroups of k_splat2<axis> that take tiles (sched.hpp).  (All LDS is static since r6: four 4-wave workgroups per CU
// for every axis but 3, whose per-segment x / y tables make it three.)
int s2_active(int axis, int grid) {
  const void *fn = axis == 0   ? (const void *)k_splat2<0, kS2Waves, false>
                   : axis == 1 ? (const void *)k_splat2<1, kS2Waves, false>
                   : axis == 2 ? (const void *)k_splat2<2, kS2Waves, false>
                   : axis == 3 ? (const void *)k_splat2<3, kS2Waves, false>
                               : (const void *)k_splat2<-1, kS2Waves, false>;
  static const int force = getenv("UNIRES_SPLAT2_RESIDENT") ? atoi(getenv("UNIRES_SPLAT2_RESIDENT")) : 0;
  return resident_workgroups(fn, kWave * kS2Waves, grid, force);
}

int launch_splat2(const SplatSched &S, const float *src, size_t src_numel, const float4 *tab_dev, int gn,
                  unsigned row_stride, unsigned tab_step, unsigned xs_sy, unsigned xs_sx, const Affine &A,
                  float alpha,
                  const PushEpilogue &ep, float *dst, Dim3i dd, const int *done, hipStream_t st) {
  if (!S.valid || S.ntiles != s2_ntiles(dd) || !S.recs || !S.bwords) return 1;
  if (S.axis >= 0 && (!tab_dev || gn < 1)) return 1;
  if (S.axis == 3 && !S.ext) return 1;
  if (src_numel >= (1ull << 30)) return 1;  // 32-bit byte offsets into the source
  if ((unsigned long long)row_stride * 4ull >= (1ull << 24)) return 1;  // 24-bit multiply
  S2Args P;
  P.src = src;
  P.src_bytes = src_numel * sizeof(float);  // buffer range check: idle lanes may point anywhere
  P.tab = tab_dev, P.gn = gn;
  P.row_stride4 = 4u * row_stride, P.tab_step4 = 4u * tab_step;
  P.entries = S.entries, P.ent_bytes = S.cap_entries * sizeof(S2Entry), P.ext = S.ext, P.xs_sy4 = 4u * xs_sy, P.xs_sx4 = 4u * xs_sx, P.masks = S.masks, P.bwords = S.bwords, P.recs = S.recs, P.ntiles = S.ntiles;
  P.A = A, P.alpha = alpha;
  P.p = ep.p, P.a0 = ep.a0, P.cx = ep.cx, P.cy = ep.cy, P.cz = ep.cz;
  P.dst = dst, P.dd = dd, P.accumulate = ep.accumulate, P.partials = ep.partials, P.objb = ep.objb;
  P.res_r = nullptr, P.res_p = nullptr, P.res_M = nullptr, P.partials2 = nullptr;
  if (ep.res_r) {
    if (!ep.res_b || !ep.res_p || !ep.partials || ep.objb) return 1;
    P.objb = ep.res_b, P.res_r = ep.res_r, P.res_p = ep.res_p, P.res_M = ep.res_M, P.partials2 = ep.res_obj;
  }
  static const int dbg = getenv("UNIRES_S2_DBG") ? atoi(getenv("UNIRES_S2_DBG")) : 0;
  P.dbg = dbg;
  const dim3 grid(s2_grid(dd, ep.grid_cap)), block(kWave * kS2Waves);
  P.active = s2_active(S.axis, (int)grid.x);
  // (the walk's layout depends on the launch only through the number of partitions, min(8, workgroups): a smaller
  // persistent grid - ep.grid_cap - walks the same records with fewer wave slots per partition)
  if (std::min(8, P.active) != std::min(8, S.nwg) || (P.active >= 8 && P.active % 8)) return 1;
  for (int x = 0; x <= 8; ++x) P.xlo[x] = S.pos_lo[x];
  static const int prio_rot = getenv("UNIRES_S2_PRIO") ? atoi(getenv("UNIRES_S2_PRIO")) : 1;
  P.prio_rot = prio_rot;
  P.prof = nullptr;
#ifdef UNIRES_S2_PROF
  static unsigned long long *prof_dev = nullptr;
  const size_t nprof = (size_t)grid.x * kS2Waves * 32;
  if (!prof_dev) (void)hipMalloc((void **)&prof_dev, 4096 * 4 * 32 * sizeof(unsigned long long));
  (void)hipMemsetAsync(prof_dev, 0, nprof * sizeof(unsigned long long), st);
  P.prof = prof_dev;
#endif
#define S2_LAUNCH(AX)                                                                          \
  do {                                                                                         \
    if (P.objb)                                                                                \
      hipLaunchKernelGGL((k_splat2<AX, kS2Waves, true>), grid, block, 0, st, P, done);         \
    else                                                                                       \
      hipLaunchKernelGGL((k_splat2<AX, kS2Waves, false>), grid, block, 0, st, P, done);        \
  } while (0)
  switch (S.axis) {
    case 0: S2_LAUNCH(0); break;
    case 1: S2_LAUNCH(1); break;
    case 2: S2_LAUNCH(2); break;
    case 3: S2_LAUNCH(3); break;
    default: S2_LAUNCH(-1); break;
  }
#undef S2_LAUNCH
#ifdef UNIRES_S2_PROF
  {
    static int shots = 0;
    if (++shots == 12 && getenv("UNIRES_S2_PROF_OUT")) {  // one warmed-up launch
      std::vector<unsigned long long> h(nprof);
      (void)hipStreamSynchronize(st);
      (void)hipMemcpy(h.data(), prof_dev, nprof * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      FILE *f = fopen(getenv("UNIRES_S2_PROF_OUT"), "w");
      for (size_t w = 0; w < nprof / 32; ++w) {
        for (int i = 0; i < 32; ++i) fprintf(f, "%llu ", h[w * 32 + i]);
        fprintf(f, "\n");
      }
      fclose(f);
    }
  }
#endif
  return 0;
}

}  // namespace unires
