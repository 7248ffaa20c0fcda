// Point-cloud renderer kernels (PyTorch3D 0.4.0 rasterize_points and the three point compositors),
// forward and backward.  renderer/points.py restates every formula in torch.
//
// Rasterizer forward.  One workgroup per pixel tile of one cloud's image, one lane per pixel.  The
// cloud's points stream through the workgroup in chunks (PR_POINTS_CHUNK records, at most
// kChunkMax): every thread reads records from global memory, drops those behind the camera
// (z >= 0 fails, also for a NaN) and those whose radius-grown box misses the tile's rectangle of
// pixel centres, and appends the survivors as (x, y, z, r^2, index) records to an LDS list (an LDS
// integer counter; the list's order does not matter, see below).  Then every lane walks the list (all
// lanes read one address: a broadcast), evaluates the exact test
//     dx = xf - x, dy = yf - y, d2 = dx dx + dy dy, candidate iff d2 < r^2
// in float32 without contraction, and inserts the candidates into its K-queue, kept sorted by
// (z, packed index).  The queue lives in LDS as [slot][lane] (a register array indexed at run time
// would go to scratch; lanes of a wave hit consecutive banks).  The tile cull is conservative only
// (the box is grown by r (1 + 1e-3) + 1e-6, far above the rounding of the differences), the exact
// test is one expression per (pixel, point), and (z, index) is a total order on a cloud's points, so
// the fragments do not depend on the tile shape, the chunk size or the order of the list.  d2 is
// evaluated once more from the chosen index when the fragments are written: the same operations
// on the same operands, the same bits.
//
// Geometry.  The queue is 4096 (z, index) pairs = 32 KiB and the survivor list 20 KiB: 52 KiB of
// the CU's 160 KiB, three workgroups per CU.  K <= 16 takes 16 x 16 pixel tiles (256 lanes x 16
// slots), 16 < K <= 64 takes 8 x 8 tiles (one wave x 64 slots).  K > PR_POINTS_MAX_K = 64 is
// refused (the caller's torch composition serves it).
//
// Backward passes: gathers over the caller's point -> entries CSR (a stable device sort of idx), one
// wave per point, lane l takes entries l, l + 64, ... in ascending order, then a fixed xor tree: no
// atomics, the same bits on every call.
//   rasterizer:  d x_p = sum 2 (x_p - xf) g_dists, d y_p likewise, d z_p = sum g_zbuf.
//   compositor:  a first kernel (one lane per pixel) writes d alphas and a per-slot coefficient c
//                with d out / d f_k = a_k c_k; a second gathers d features over the CSR.
// Compositor arithmetic, G_k = sum_c g_c f_kc over the channels of valid slot k:
//   alpha     T_k = prod_{j<k valid}(1 - a_j), c_k = T_k, d a_t = T_t (G_t - R_t) with the suffix
//             R_t = sum_{k>t} a_k G_k prod_{t<j<k}(1 - a_j), by R_{t-1} = a_t G_t + (1 - a_t) R_t:
//             prefix and suffix products, never a division by (1 - a_t)
//   norm      D = max(sum a, 1e-4), c_k = 1 / D, d a_t = (G_t - [sum a >= 1e-4] sum_k a_k G_k / D) / D
//   weighted  c_k = 1, d a_t = G_t.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "pr_common.h"

namespace pr {
namespace {

constexpr int kChunkMax = 1024;   // records of the survivor list (20 KiB)
constexpr int kQueue = 4096;      // (z, index) pairs of a workgroup's queues (32 KiB)
constexpr int kWaves = kThreads / 64;
constexpr float kNormClamp = 1e-4f;
constexpr int64_t kMaxRows = 65535 * 8;  // grid.y of the forward's 8 x 8 tiles

PR_DEV float wave_sum(float v) {  // a fixed xor tree over the 64 lanes
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

PR_DEV bool key_less(float z, int i, float qz, int qi) { return z < qz || (z == qz && i < qi); }

// grid (tiles_x, tiles_y, N); T = TW * TH lanes, KCAP * T = kQueue
template <int TW, int TH, int KCAP>
__global__ void __launch_bounds__(TW* TH) points_rast_fwd_kernel(PRPointsRastArgs a, int chunk) {
  constexpr int T = TW * TH;
  static_assert(KCAP * T == kQueue, "queue size");
  __shared__ float qz[kQueue];
  __shared__ int qi[kQueue];
  __shared__ float sx[kChunkMax], sy[kChunkMax], sz[kChunkMax], sr2[kChunkMax];
  __shared__ int si[kChunkMax];
  __shared__ int scount;
  const int tid = threadIdx.x, n = blockIdx.z, H = a.H, W = a.W, K = a.K;
  const int col0 = blockIdx.x * TW, row0 = blockIdx.y * TH;
  const int col = col0 + tid % TW, row = row0 + tid / TW;
  const bool inimg = row < H && col < W;
  const float xf = ndc(W - 1 - min(col, W - 1), W, H), yf = ndc(H - 1 - min(row, H - 1), H, W);
  // the tile's rectangle of pixel centres; +X points left, +Y up
  const int c1 = min(col0 + TW - 1, W - 1), r1 = min(row0 + TH - 1, H - 1);
  const float txmax = ndc(W - 1 - col0, W, H), txmin = ndc(W - 1 - c1, W, H);
  const float tymax = ndc(H - 1 - row0, H, W), tymin = ndc(H - 1 - r1, H, W);
  const int64_t first = std::min<int64_t>(std::max<int64_t>(a.cloud_first[n], 0), a.P);
  const int64_t count = std::min<int64_t>(std::max<int64_t>(a.cloud_count[n], 0), a.P - first);
  int cnt = 0;  // valid slots of this lane's queue
  for (int64_t c0 = 0; c0 < count; c0 += chunk) {
    __syncthreads();  // the previous list has been read
    if (tid == 0) scount = 0;
    __syncthreads();
    const int len = (int)std::min<int64_t>(chunk, count - c0);
    for (int t = tid; t < len; t += T) {
      const int64_t p = first + c0 + t;
      const float x = a.points[p * 3], y = a.points[p * 3 + 1], z = a.points[p * 3 + 2];
      const float r = a.radius ? a.radius[p] : a.radius_scalar;
      const float m = fabsf(r) * 1.001f + 1e-6f;
      bool keep = z >= 0.f;  // false for a NaN
      if (x - txmax > m || txmin - x > m || y - tymax > m || tymin - y > m) keep = false;  // a NaN is kept: the exact test drops it
      if (keep) {
        const int s = atomicAdd(&scount, 1);  // s < len <= kChunkMax
        sx[s] = x, sy[s] = y, sz[s] = z, sr2[s] = r * r, si[s] = (int)p;
      }
    }
    __syncthreads();
    const int ns = scount;
    if (inimg) {
      for (int s = 0; s < ns; ++s) {
        const float dx = xf - sx[s], dy = yf - sy[s];
        const float d2 = dx * dx + dy * dy;
        if (!(d2 < sr2[s])) continue;
        const float z = sz[s];
        const int i = si[s];
        if (cnt == K) {
          if (!key_less(z, i, qz[(K - 1) * T + tid], qi[(K - 1) * T + tid])) continue;
        } else {
          ++cnt;
        }
        int j = cnt - 1;
        while (j > 0 && key_less(z, i, qz[(j - 1) * T + tid], qi[(j - 1) * T + tid])) {
          qz[j * T + tid] = qz[(j - 1) * T + tid];
          qi[j * T + tid] = qi[(j - 1) * T + tid];
          --j;
        }
        qz[j * T + tid] = z;
        qi[j * T + tid] = i;
      }
    }
  }
  if (!inimg) return;
  const int64_t base = (((int64_t)n * H + row) * W + col) * K;
  for (int k = 0; k < K; ++k) {
    int64_t i = -1;
    float z = -1.f, d2 = -1.f;
    if (k < cnt) {
      i = qi[k * T + tid];
      z = qz[k * T + tid];
      const float dx = xf - a.points[i * 3], dy = yf - a.points[i * 3 + 1];
      d2 = dx * dx + dy * dy;
    }
    a.idx[base + k] = i;
    a.zbuf[base + k] = z;
    a.dists[base + k] = d2;
  }
}

// one wave per point
__global__ void __launch_bounds__(kThreads) points_rast_bwd_kernel(PRPointsRastArgs a, int64_t total) {
  const int lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); p < a.P; p += (int64_t)gridDim.x * kWaves) {
    const int64_t b = std::max<int64_t>(a.point_start[p], 0), e = std::min<int64_t>(a.point_start[p + 1], total);
    const float x = a.points[p * 3], y = a.points[p * 3 + 1];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (e > b) {  // uniform over the wave
      for (int64_t j = b + lane; j < e; j += 64) {
        const int64_t ent = a.point_entries[j];
        if (ent < 0 || ent >= total) continue;
        const int64_t pix = ent / a.K;
        const int col = (int)(pix % a.W), row = (int)((pix / a.W) % a.H);
        const float xf = ndc(a.W - 1 - col, a.W, a.H), yf = ndc(a.H - 1 - row, a.H, a.W);
        const float gd = a.grad_dists[ent];
        gx += 2.f * (x - xf) * gd;
        gy += 2.f * (y - yf) * gd;
        gz += a.grad_zbuf[ent];
      }
      gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz);
    }
    if (lane == 0) a.grad_points[p * 3] = gx, a.grad_points[p * 3 + 1] = gy, a.grad_points[p * 3 + 2] = gz;
  }
}

// one lane per (pixel, channel)
__global__ void __launch_bounds__(kThreads) points_composite_fwd_kernel(PRPointsCompositeArgs a, int64_t total) {
  const int K = a.K, C = a.C;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
    const int64_t pix = t / C, base = pix * K;
    const int c = (int)(t % C);
    float acc = 0.f, T = 1.f, sum = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t i = a.idx[base + k];
      if (i < 0 || i >= a.P) continue;
      const float al = a.alphas[base + k], f = a.features[i * C + c];
      if (a.mode == PR_POINTS_ALPHA) {
        acc += (al * T) * f;
        T *= 1.f - al;
      } else {
        acc += al * f;
        sum += al;
      }
    }
    if (a.mode == PR_POINTS_NORM) acc = acc / (sum < kNormClamp ? kNormClamp : sum);
    a.out[t] = acc;
  }
}

// one lane per pixel: grad_alphas, and coef (N,H,W,K) with d out / d f_k = a_k coef_k
__global__ void __launch_bounds__(kThreads) points_composite_bwd_pixel_kernel(PRPointsCompositeArgs a, float* coef,
                                                                               int64_t pixels) {
  const int K = a.K, C = a.C;
  for (int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x; pix < pixels; pix += (int64_t)gridDim.x * kThreads) {
    const int64_t base = pix * K;
    const float* g = a.grad_out + pix * C;
    float T = 1.f, sum = 0.f, sum_g = 0.f;
    for (int k = 0; k < K; ++k) {  // G_k into grad_alphas, the prefix product into coef
      const int64_t i = a.idx[base + k];
      float G = 0.f, cf = 0.f;
      if (i >= 0 && i < a.P) {
        const float* f = a.features + i * C;
        for (int c = 0; c < C; ++c) G += g[c] * f[c];
        const float al = a.alphas[base + k];
        cf = T;
        T *= 1.f - al;
        sum += al;
        sum_g += al * G;
      }
      a.grad_alphas[base + k] = G;
      coef[base + k] = cf;
    }
    if (a.mode == PR_POINTS_ALPHA) {
      float R = 0.f;
      for (int k = K - 1; k >= 0; --k) {
        const int64_t i = a.idx[base + k];
        if (i < 0 || i >= a.P) continue;  // grad_alphas and coef are 0 already
        const float al = a.alphas[base + k], G = a.grad_alphas[base + k];
        a.grad_alphas[base + k] = coef[base + k] * (G - R);
        R = al * G + (1.f - al) * R;
      }
    } else if (a.mode == PR_POINTS_NORM) {
      const float D = sum < kNormClamp ? kNormClamp : sum;
      const float q = sum >= kNormClamp ? sum_g / D : 0.f;
      for (int k = 0; k < K; ++k) {
        const int64_t i = a.idx[base + k];
        if (i < 0 || i >= a.P) continue;
        a.grad_alphas[base + k] = (a.grad_alphas[base + k] - q) / D;
        coef[base + k] = 1.f / D;
      }
    } else {
      for (int k = 0; k < K; ++k) {
        const int64_t i = a.idx[base + k];
        if (i >= 0 && i < a.P) coef[base + k] = 1.f;
      }
    }
  }
}

// one wave per point: grad_features (P,C)
__global__ void __launch_bounds__(kThreads) points_composite_bwd_feature_kernel(PRPointsCompositeArgs a, const float* coef,
                                                                                 int64_t total) {
  const int lane = threadIdx.x & 63, C = a.C;
  for (int64_t p = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); p < a.P; p += (int64_t)gridDim.x * kWaves) {
    const int64_t b = std::max<int64_t>(a.point_start[p], 0), e = std::min<int64_t>(a.point_start[p + 1], total);
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
      if (e > b) {  // uniform over the wave
        for (int64_t j = b + lane; j < e; j += 64) {
          const int64_t ent = a.point_entries[j];
          if (ent < 0 || ent >= total) continue;
          acc += (a.alphas[ent] * coef[ent]) * a.grad_out[(ent / a.K) * C + c];
        }
        acc = wave_sum(acc);
      }
      if (lane == 0) a.grad_features[p * C + c] = acc;
    }
  }
}

int grid_of(int64_t n, int64_t per, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap)); }

// records per chunk of the forward; PR_POINTS_CHUNK overrides (read per call)
int pick_chunk() {
  if (const char* e = getenv("PR_POINTS_CHUNK")) {
    const int c = atoi(e);
    if (c > 0) return std::min(c, kChunkMax);
  }
  return kChunkMax;
}

bool image_ok(int64_t N, int64_t H, int64_t W, int64_t K) {
  return N > 0 && H > 0 && W > 0 && K > 0 && N <= 65535 && H <= kMaxRows && N * H * W <= INT32_MAX / K;
}

int image_check(const std::string& w, int64_t N, int64_t H, int64_t W, int64_t K, int64_t P) {
  if (N <= 0 || H <= 0 || W <= 0 || K <= 0 || P <= 0) return set_error(PR_ERR_ARG, w + ": N, H, W, K and P must be positive");
  if (N > 65535) return set_error(PR_ERR_ARG, w + ": N must fit the grid (65535)");
  if (H > kMaxRows) return set_error(PR_ERR_ARG, w + ": H must fit the grid (" + std::to_string(kMaxRows) + " rows)");
  if (N * H * W > INT32_MAX / K || P > INT32_MAX) return set_error(PR_ERR_ARG, w + ": N H W K and P must fit int32");
  return PR_OK;
}

int rast_check(const PRPointsRastArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (int e = image_check(w, a->N, a->H, a->W, a->K, a->P)) return e;
  if (a->K > PR_POINTS_MAX_K) return set_error(PR_ERR_ARG, w + ": K exceeds PR_POINTS_MAX_K (" + std::to_string(PR_POINTS_MAX_K) + ")");
  if (!a->points || !a->idx) return set_error(PR_ERR_ARG, w + ": points / idx missing");
  if (fwd && (!a->cloud_first || !a->cloud_count)) return set_error(PR_ERR_ARG, w + ": cloud_first / cloud_count missing");
  if (fwd && (!a->zbuf || !a->dists)) return set_error(PR_ERR_ARG, w + ": zbuf / dists missing");
  if (!fwd && (!a->point_start || !a->point_entries)) return set_error(PR_ERR_ARG, w + ": point -> entries CSR missing");
  if (!fwd && (!a->grad_zbuf || !a->grad_dists || !a->grad_points)) return set_error(PR_ERR_ARG, w + ": grads missing");
  return PR_OK;
}

int composite_check(const PRPointsCompositeArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (int e = image_check(w, a->N, a->H, a->W, a->K, a->P)) return e;
  if (a->C <= 0) return set_error(PR_ERR_ARG, w + ": C must be positive");
  if ((int64_t)a->N * a->H * a->W > INT32_MAX / a->C || a->P > INT32_MAX / a->C)
    return set_error(PR_ERR_ARG, w + ": N H W C and P C must fit int32");
  if (a->mode != PR_POINTS_ALPHA && a->mode != PR_POINTS_NORM && a->mode != PR_POINTS_WEIGHTED)
    return set_error(PR_ERR_ARG, w + ": mode must be 0 (alpha), 1 (norm) or 2 (weighted), got " + std::to_string(a->mode));
  if (!a->idx || !a->alphas || !a->features) return set_error(PR_ERR_ARG, w + ": idx / alphas / features missing");
  if (fwd && !a->out) return set_error(PR_ERR_ARG, w + ": out missing");
  if (!fwd && (!a->point_start || !a->point_entries)) return set_error(PR_ERR_ARG, w + ": point -> entries CSR missing");
  if (!fwd && (!a->grad_out || !a->grad_alphas || !a->grad_features)) return set_error(PR_ERR_ARG, w + ": grads missing");
  if (!fwd) {
    const size_t need = (size_t)a->N * a->H * a->W * a->K * sizeof(float);
    if (!a->workspace || a->workspace_bytes < need)
      return set_error(PR_ERR_ARG, w + ": workspace missing or smaller than pr_points_workspace (" + std::to_string(need) + " bytes)");
  }
  return PR_OK;
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_points_workspace(int32_t N, int32_t H, int32_t W, int32_t K) {
  if (!image_ok(N, H, W, K)) return 0;
  return (size_t)N * H * W * K * sizeof(float);
}

extern "C" int pr_points_rast_fwd(const PRPointsRastArgs* args, void* stream) {
  if (int e = rast_check(args, "points_rast_fwd", true)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const PRPointsRastArgs& a = *args;
  const int chunk = pick_chunk();
  if (a.K <= 16) {
    points_rast_fwd_kernel<16, 16, 16><<<dim3((a.W + 15) / 16, (a.H + 15) / 16, a.N), 256, 0, st>>>(a, chunk);
  } else {
    points_rast_fwd_kernel<8, 8, 64><<<dim3((a.W + 7) / 8, (a.H + 7) / 8, a.N), 64, 0, st>>>(a, chunk);
  }
  return check_launch("points_rast_fwd");
}

extern "C" int pr_points_rast_bwd(const PRPointsRastArgs* args, void* stream) {
  if (int e = rast_check(args, "points_rast_bwd", false)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)args->N * args->H * args->W * args->K;
  points_rast_bwd_kernel<<<grid_of(args->P, kWaves, 16384), kThreads, 0, st>>>(*args, total);
  return check_launch("points_rast_bwd");
}

extern "C" int pr_points_composite_fwd(const PRPointsCompositeArgs* args, void* stream) {
  if (int e = composite_check(args, "points_composite_fwd", true)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)args->N * args->H * args->W * args->C;
  points_composite_fwd_kernel<<<grid_of(total, kThreads, 16384), kThreads, 0, st>>>(*args, total);
  return check_launch("points_composite_fwd");
}

extern "C" int pr_points_composite_bwd(const PRPointsCompositeArgs* args, void* stream) {
  if (int e = composite_check(args, "points_composite_bwd", false)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t pixels = (int64_t)args->N * args->H * args->W;
  float* coef = static_cast<float*>(args->workspace);
  points_composite_bwd_pixel_kernel<<<grid_of(pixels, kThreads, 16384), kThreads, 0, st>>>(*args, coef, pixels);
  if (int e = check_launch("points_composite_bwd_pixel")) return e;
  points_composite_bwd_feature_kernel<<<grid_of(args->P, kWaves, 16384), kThreads, 0, st>>>(*args, coef, pixels * args->K);
  return check_launch("points_composite_bwd");
}
