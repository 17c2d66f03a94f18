// sched.hip - the host side of what the schedule builds of k_splat2 and k_ata1 share (see sched.hpp).
#include "sched.hpp"

#include <algorithm>
#include <map>
#include <mutex>

namespace unires {

static thread_local bool t_thorough = true;
void sched_set_thorough(bool on) { t_thorough = on; }
bool sched_thorough() { return t_thorough; }

void sched_order(const unsigned *ni, int nt, double tile_cost, int np, int *part_lo, int *geom, int nty, int ntz,
                 int strip, bool keep_order) {
  double total = 0.0;
  unsigned imax = 0;
  for (int i = 0; i < nt; ++i) total += (double)ni[i] + tile_cost, imax = std::max(imax, ni[i]);
  int x = 1;
  double cum = 0.0;
  part_lo[0] = 0;
  for (int i = 0; i < nt && x < np; ++i) {
    cum += (double)ni[i] + tile_cost;
    while (x < np && cum >= total * x / (double)np) part_lo[x++] = i + 1;
  }
  for (; x <= np; ++x) part_lo[x] = nt;
  const unsigned cheap = keep_order ? 0u : imax / 2u;
  if (strip <= 0 || strip >= nty || keep_order) strip = nty;  // (= index order)
  for (int xc = 0; xc < np; ++xc) {
    const int lo = part_lo[xc], hi = part_lo[xc + 1];
    int u = lo;
    if (strip < nty && hi > lo) {
      // (generated, not sorted: this runs inside every unires_plan_set_repeat - a rigid update per channel and
      // ADMM iteration - and a comparison sort of 17 k tiles cost 1.5 ms there)
      const int tx_lo = lo / (ntz * nty), tx_hi = (hi - 1) / (ntz * nty);
      for (int s0 = 0; s0 < nty; s0 += strip)
        for (int txi = tx_lo; txi <= tx_hi; ++txi)
          for (int tyi = s0; tyi < std::min(s0 + strip, nty); ++tyi) {
            const int base = (txi * nty + tyi) * ntz;
            for (int g = std::max(base, lo); g < std::min(base + ntz, hi); ++g)
              if (ni[g] > cheap) geom[u++] = g;
          }
    } else {
      for (int g = lo; g < hi; ++g)
        if (keep_order || ni[g] > cheap) geom[u++] = g;
    }
    const int first_cheap = u;
    for (int g = lo; g < hi; ++g)
      if (!keep_order && ni[g] <= cheap) geom[u++] = g;
    std::stable_sort(geom + first_cheap, geom + hi, [&](int a, int b) { return ni[a] > ni[b]; });
  }
  geom[nt] = 0;
}

bool sched_scratch_clear(unsigned long long *&scratch) {
  if (!scratch && hipMalloc((void **)&scratch, kSchedScratchWords * sizeof(unsigned long long)) != hipSuccess) return false;
  (void)hipMemset(scratch, 0, kSchedScratchWords * sizeof(unsigned long long));
  return true;
}

bool sched_scratch_read(const unsigned long long *scratch, int &err, unsigned long long stats[2]) {
  if (hipMemcpy(&err, scratch, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return false;
  return hipMemcpy(stats, scratch + 1, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
}

int resident_workgroups(const void *fn, int threads, int grid, int force, int *asked) {
  static std::map<const void *, int> cache;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(fn);
  if (it == cache.end()) {
    int per_cu = 0, dev = 0, ncu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0) != hipSuccess) per_cu = 0;
    if (force > 0) per_cu = force;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 0;
    const int n = per_cu > 0 && ncu > 0 ? per_cu * ncu : 1 << 30;
    if (asked) *asked = per_cu;
    it = cache.emplace(fn, n).first;
  }
  int n = std::min(grid, it->second);
  if (n >= 8) n -= n % 8;
  return n;
}

}  // namespace unires
