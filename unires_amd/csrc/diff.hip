// diff.hip - the any-shape difference kernels of the regulariser: gradient, divergence, DtD (declared in
// stencil.hpp, next to the flat and line forms they are the fallback of).
//
// Layout: float32 volumes, (X,Y,Z) C-contiguous, Z fastest.  Every kernel puts
// the 64 lanes of a wave along Z so that HBM/L2 requests are coalesced.
// Launch shape: block (64,4,1) -> grid (ceil(Z/64), ceil(Y/4), X).
#include "stencil.hpp"

namespace unires {

// --------------------------------------------------------------------------
// differences, zero bound; W: forward (the reference's default), backward, central
// --------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kBlock)
    k_grad(const float *__restrict__ src, Dim3i d, float ivx, float ivy, float ivz,
           float *__restrict__ dst) {
  const int k = blockIdx.x * kWave + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  if (k >= d.z || j >= d.y) return;
  const size_t n = d.numel();
  const size_t idx = ((size_t)i * d.y + j) * d.z + k;
  const float c = src[idx];
  if (W != kDiffForward) {
    // backward: y[i] - y[i-1]; central: y[i+1] - y[i-1], its 1/2 folded into the scale (exact)
    const size_t sx = (size_t)d.y * d.z, sy = d.z;
    const float xm = i > 0 ? src[idx - sx] : 0.f, ym = j > 0 ? src[idx - sy] : 0.f, zm = k > 0 ? src[idx - 1] : 0.f;
    float xu = c, yu = c, zu = c;
    if (W == kDiffCentral) {
      xu = i + 1 < d.x ? src[idx + sx] : 0.f, yu = j + 1 < d.y ? src[idx + sy] : 0.f;
      zu = k + 1 < d.z ? src[idx + 1] : 0.f;
    }
    const float h = diff_grad_scale(W);
    dst[idx] = (xu - xm) * (ivx * h);
    dst[n + idx] = (yu - ym) * (ivy * h);
    dst[2 * n + idx] = (zu - zm) * (ivz * h);
    return;
  }
  const float xn = i + 1 < d.x ? src[idx + (size_t)d.y * d.z] : 0.f;
  const float yn = j + 1 < d.y ? src[idx + d.z] : 0.f;
  const float zn = k + 1 < d.z ? src[idx + 1] : 0.f;
  dst[idx] = (xn - c) * ivx;
  dst[n + idx] = (yn - c) * ivy;
  dst[2 * n + idx] = (zn - c) * ivz;
}

// dst = [add +] scale * Dt(u), u = a*src_a (+ b*src_b if src_b != NULL)
template <int W>
__global__ void __launch_bounds__(kBlock)
    k_div(const float *__restrict__ ua, const float *__restrict__ ub, float ca, float cb, Dim3i d,
          float ivx, float ivy, float ivz, float scale, const float *__restrict__ add,
          float *__restrict__ dst) {
  const int k = blockIdx.x * kWave + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  const int i = blockIdx.z;
  if (k >= d.z || j >= d.y) return;
  const size_t n = d.numel();
  const size_t idx = ((size_t)i * d.y + j) * d.z + k;
  const size_t sx = (size_t)d.y * d.z, sy = d.z;
  // unconditional (clamped) loads so all of them are in flight together
  const bool lx = i > 0, ly = j > 0, lz = k > 0;
  const size_t ox = idx, oy = n + idx, oz = 2 * n + idx;
  if (W != kDiffForward) {
    // backward: (g[i] - g[i+1]) / vx; central: (g[i-1] - g[i+1]) / 2 vx.  lo: the minuend, hi: the subtrahend
    const bool hx = i + 1 < d.x, hy = j + 1 < d.y, hz = k + 1 < d.z;
    const bool cen = W == kDiffCentral;
    const size_t oxl = cen ? (lx ? ox - sx : ox) : ox, oyl = cen ? (ly ? oy - sy : oy) : oy, ozl = cen ? (lz ? oz - 1 : oz) : oz;
    const size_t oxh = hx ? ox + sx : ox, oyh = hy ? oy + sy : oy, ozh = hz ? oz + 1 : oz;
    float xl = ca * ua[oxl], xh = ca * ua[oxh], yl = ca * ua[oyl], yh = ca * ua[oyh];
    float zl = ca * ua[ozl], zh = ca * ua[ozh];
    if (ub) {
      xl += cb * ub[oxl], xh += cb * ub[oxh], yl += cb * ub[oyl], yh += cb * ub[oyh];
      zl += cb * ub[ozl], zh += cb * ub[ozh];
    }
    const float h = diff_grad_scale(W);
    float acc = (((!cen || lx) ? xl : 0.f) - (hx ? xh : 0.f)) * (ivx * h);
    acc += (((!cen || ly) ? yl : 0.f) - (hy ? yh : 0.f)) * (ivy * h);
    acc += (((!cen || lz) ? zl : 0.f) - (hz ? zh : 0.f)) * (ivz * h);
    dst[idx] = (add ? add[idx] : 0.f) + scale * acc;
    return;
  }
  const size_t oxm = lx ? ox - sx : ox, oym = ly ? oy - sy : oy, ozm = lz ? oz - 1 : oz;
  float vx = ca * ua[ox], vxm = ca * ua[oxm], vy = ca * ua[oy], vym = ca * ua[oym];
  float vz = ca * ua[oz], vzm = ca * ua[ozm];
  if (ub) {
    vx += cb * ub[ox], vxm += cb * ub[oxm], vy += cb * ub[oy], vym += cb * ub[oym];
    vz += cb * ub[oz], vzm += cb * ub[ozm];
  }
  float acc = ((lx ? vxm : 0.f) - vx) * ivx;
  acc += ((ly ? vym : 0.f) - vy) * ivy;
  acc += ((lz ? vzm : 0.f) - vz) * ivz;
  dst[idx] = (add ? add[idx] : 0.f) + scale * acc;
}

// dst = a*src + c*DtD(src): 7-point stencil with Neumann row at 0 and Dirichlet
// row at n-1 along every axis.  Optional fused float64 partial of sum(src*dst).
// W: the difference of D (weights already times diff_dtd_scale(W)).  ACC: dst += c*DtD(src) instead (a unused):
// the closing pass of a non-forward matvec where the flat kernel does not serve the shape.
template <bool DOT, int W, bool ACC>
__global__ void __launch_bounds__(kBlock)
    k_dtd(const float *__restrict__ src, Dim3i d, float cx, float cy, float cz, float a,
          float *__restrict__ dst, double *__restrict__ partials,
          const float *__restrict__ objb, const int *__restrict__ done) {
  if (done && *done) return;
  // tiles of 4 y-rows x 64 z; a bounded grid (<= kMaxPartials blocks) strides over them
  const int tz = (d.z + kWave - 1) / kWave, ty = (d.y + 3) / 4;
  const long long ntiles = (long long)tz * ty * d.x;
  double prod = 0.0;
  for (long long t = xcd_chunked_block(blockIdx.x, gridDim.x); t < ntiles; t += gridDim.x) {
    const int kc = (int)(t % tz);
    const long long t2 = t / tz;
    const int jq = (int)(t2 % ty);
    const int i = (int)(t2 / ty);
    const int k = kc * kWave + threadIdx.x;
    const int j = jq * 4 + threadIdx.y;
    if (k < d.z && j < d.y) {
      const size_t idx = ((size_t)i * d.y + j) * d.z + k;
      float c;
      const float st = dtd_at<W>(src, idx, i, j, k, d, cx, cy, cz, c);
      const float q = ACC ? dst[idx] + st : a * c + st;
      if (W != kDiffForward || ACC)  // (the closing pass of a non-forward matvec: exact products in the dot)
        matvec_emit_w(dst, idx, q, c, DOT ? objb : nullptr, DOT, prod);
      else
        matvec_emit(dst, idx, q, c, DOT ? objb : nullptr, DOT, prod);
    }
  }
  if (DOT) {
    const double tot = block_sum(prod);
    if (threadIdx.x == 0 && threadIdx.y == 0) partials[blockIdx.x] = tot;
  }
}

// (one instantiation per difference, by_diff(): forward's is the code it always was)
void launch_grad(const float *src, Dim3i d, const float vx[3], float *dst3, hipStream_t st, int which) {
  by_diff(which, [&](auto W) {
    hipLaunchKernelGGL(k_grad<W()>, vol_grid(d), vol_block(), 0, st, src, d, 1.f / vx[0], 1.f / vx[1], 1.f / vx[2], dst3);
  });
}

void launch_div(const float *ua, const float *ub, float ca, float cb, Dim3i d, const float vx[3],
                float scale, const float *add, float *dst, hipStream_t st, int which) {
  by_diff(which, [&](auto W) {
    hipLaunchKernelGGL(k_div<W()>, vol_grid(d), vol_block(), 0, st, ua, ub, ca, cb, d, 1.f / vx[0], 1.f / vx[1],
                       1.f / vx[2], scale, add, dst);
  });
}

int dtd_num_blocks(Dim3i d) {
  const long long ntiles = (long long)((d.z + kWave - 1) / kWave) * ((d.y + 3) / 4) * d.x;
  return (int)(ntiles < kMaxPartials ? ntiles : kMaxPartials);
}

// partials (nullable) must hold dtd_num_blocks(d) doubles.
void launch_dtd(const float *src, Dim3i d, const float vx[3], float a, float c, float *dst,
                double *partials, const float *objb, const int *done, hipStream_t st, int which, bool accumulate) {
  const float h = diff_dtd_scale(which);
  const float cx = c / (vx[0] * vx[0]) * h, cy = c / (vx[1] * vx[1]) * h, cz = c / (vx[2] * vx[2]) * h;
  const dim3 grid(dtd_num_blocks(d));
  by_diff(which, [&](auto W) {
    if (accumulate && partials)
      hipLaunchKernelGGL((k_dtd<true, W(), true>), grid, vol_block(), 0, st, src, d, cx, cy, cz, a, dst, partials, objb, done);
    else if (accumulate)
      hipLaunchKernelGGL((k_dtd<false, W(), true>), grid, vol_block(), 0, st, src, d, cx, cy, cz, a, dst, partials, nullptr, done);
    else if (partials)
      hipLaunchKernelGGL((k_dtd<true, W(), false>), grid, vol_block(), 0, st, src, d, cx, cy, cz, a, dst, partials, objb, done);
    else
      hipLaunchKernelGGL((k_dtd<false, W(), false>), grid, vol_block(), 0, st, src, d, cx, cy, cz, a, dst, partials, nullptr, done);
  });
}

}  // namespace unires
