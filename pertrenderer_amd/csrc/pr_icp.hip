// Rigid / similarity alignment of padded point clouds (PyTorch3D 0.4.0 corresponding_points_alignment
// and iterative_closest_point), float32 points, D = 3, row vectors (x R ~ y).  A whole ICP iteration
// runs on the device with no host read.
//
// Search: one lane per query of the initial cloud x.  The lane reads its cloud's current (R, T, s)
// and forms Xt_i = s (x_i R) + T in registers; the database y goes through LDS in tiles of kTile
// points that every lane walks in index order (an LDS broadcast, 3 ds_read_b128 per 4 points),
// keeping a running (min, argmin) of dist2_3 under a strict <: the lowest index wins on equal d^2 and
// a NaN point is never chosen (pr_chamfer.hip's walk).  With few queries the database is cut into
// S ranges over gridDim.y and a merge pass walks the partial pairs in range order with the same <.
//
// Moments: fused into the search when it is unsplit, into the merge otherwise.  With c = Xmu (the
// centroid of x, formed once per run), xc = x - Xmu and d = nn - c, every workgroup writes one
// float64 record of its queries: sum w, sum w d, sum w^2 xc (x) d, sum w^2 |xc|^2, sum w |d|^2,
// sum w^2 xc.  The lanes of a wave are added by a shuffle tree and the four waves in order.
//
// Solve: one workgroup, a wave per cloud.  Lanes 0..17 add the cloud's records in index order, one
// component each; the 3 x 3 SVD is a cyclic one-sided Jacobi in float64 (a fixed sweep count, the
// rotation skipped when the columns are orthogonal to rounding), singular values descending.  The
// rmse of the new transform against the neighbours it was solved from comes in closed form from the
// centred moments (the clouds' coordinates are float32, the moments float64).  No atomics anywhere:
// the same bits on every call, whatever the number of iterations enqueued per call.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "pr_common.h"

namespace pr {
namespace {

constexpr int kTile = 512;           // database points per LDS tile (6 KiB); a multiple of 4
constexpr int kTargetBlocks = 2048;  // workgroups wanted on a 256-CU part (8 per CU)
constexpr int kMaxSplits = 64;
constexpr int kWaves = kThreads / 64;
constexpr int kSweeps = 12;          // Jacobi sweeps: a 3 x 3 matrix is orthogonal to rounding after 5 or 6
constexpr double kIcpEps = 1e-9;     // corresponding_points_alignment's default eps, which ICP uses
constexpr int kS = PR_ICP_STATE;

// a record's components
constexpr int mW = 0, mY = 1, mC = 4, mX2 = 13, mY2 = 14, mWX = 15, kRec = PR_ALIGN_RECORD;
static_assert(kRec == 18, "the record layout of include/pertrender.h");

struct Partial {
  float d;
  int32_t idx;
};

struct IcpLaunch {
  const float* x;
  const float* y;
  const int64_t* x_len;
  const int64_t* y_len;
  int64_t N, P, Q;
  int max_iterations, estimate_scale, allow_reflection;
  float thr;
  float* state;
  float* history;
  float* rmse;
  int32_t* idx;
  int32_t* idx_history;
  int32_t* flags;
  int splits;
  int64_t chunk;  // database points per split
  int64_t nblk;   // query workgroups (records) per cloud
  double* xmu;    // (N,4): Xmu, sum w
  float* prev;    // (N) the previous iteration's rmse
  double* rec;    // (N, nblk, kRec)
  Partial* part;  // (N, splits, P) when splits > 1
};

struct AlignLaunch {
  const float* x;
  const float* y;
  const float* w;
  const int64_t* x_len;
  int64_t N, P, nblk;
  int estimate_scale, allow_reflection;
  double eps;
  float* R;
  float* T;
  float* s;
  double* xmu;
  double* rec;
};

PR_DEV int64_t cloud_len(const int64_t* len, int64_t n, int64_t full) {
  if (!len) return full;
  const int64_t l = len[n];
  return l < 0 ? 0 : (l > full ? full : l);
}

PR_DEV void consider(float qx, float qy, float qz, float px, float py, float pz, int32_t j, float& best, int32_t& arg) {
  const float d = dist2_3(qx, qy, qz, px, py, pz);
  if (d < best) {
    best = d;
    arg = j;
  }
}

// iteration `it` runs unless the batch has converged or max_iterations have been executed
PR_DEV bool icp_done(const IcpLaunch& L, int& it) {
  it = L.flags[1];
  return L.flags[0] != 0 || it >= L.max_iterations;
}

// per component: the wave's lanes by a shuffle tree, then the waves in order; thread c < K returns component c
template <int K>
PR_DEV double block_sum(const double (&m)[K], double (*red)[K]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    double v = m[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < K) {
    t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += red[w][threadIdx.x];
  }
  return t;
}

// one correspondence's terms: weight w, the point x, its partner y, c = Xmu
PR_DEV void moments(double (&m)[kRec], double w, float x0, float x1, float x2, float y0, float y1, float y2,
                    const double* xmu) {
  const double a[3] = {(double)x0 - xmu[0], (double)x1 - xmu[1], (double)x2 - xmu[2]};
  const double d[3] = {(double)y0 - xmu[0], (double)y1 - xmu[1], (double)y2 - xmu[2]};
  const double w2 = w * w;
  m[mW] = w;
#pragma unroll
  for (int k = 0; k < 3; ++k) m[mY + k] = w * d[k];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[mC + 3 * j + k] = w2 * a[j] * d[k];
    m[mWX + j] = w2 * a[j];
  }
  m[mX2] = w2 * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  m[mY2] = w * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// grid (N): Xmu = sum w x / max(sum w, eps) over the rows below the cloud's length
__global__ void __launch_bounds__(kThreads) centroid_kernel(const float* x, const float* w, const int64_t* x_len, int64_t P,
                                                            double eps, double* xmu, float* prev, int32_t* flags) {
  __shared__ double red[kWaves][4];
  const int64_t n = blockIdx.x, len = cloud_len(x_len, n, P);
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < len; i += kThreads) {
    const float* p = x + (n * P + i) * 3;
    const double wi = w ? (double)w[n * P + i] : 1.0;
    m[0] += wi * (double)p[0], m[1] += wi * (double)p[1], m[2] += wi * (double)p[2], m[3] += wi;
  }
  const double t = block_sum<4>(m, red);
  if (threadIdx.x < 4) red[0][threadIdx.x] = t;  // every thread has read red in block_sum
  __syncthreads();
  if (threadIdx.x < 3) xmu[n * 4 + threadIdx.x] = red[0][threadIdx.x] / fmax(red[0][3], eps);
  if (threadIdx.x == 3) xmu[n * 4 + 3] = red[0][3];
  if (threadIdx.x == 0 && prev) prev[n] = 0.f;
  if (threadIdx.x == 0 && n == 0 && flags) flags[0] = 0, flags[1] = 0;
}

// The end of a query of iteration `it`: its neighbour's index is stored and the workgroup's record
// written.  Called by every thread of the workgroup.
PR_DEV void finish_query(const IcpLaunch& L, int it, int64_t n, int64_t i, bool live, int32_t arg, float x0, float x1,
                         float x2, double (*red)[kRec]) {
  if (i < L.P) {
    L.idx[n * L.P + i] = arg;
    if (L.idx_history) L.idx_history[((int64_t)it * L.N + n) * L.P + i] = arg;
  }
  double m[kRec];
#pragma unroll
  for (int c = 0; c < kRec; ++c) m[c] = 0.0;
  if (live) {
    float y0 = NAN, y1 = NAN, y2 = NAN;  // a live query without a neighbour: its cloud's moments are NaN
    if (arg >= 0) {
      const float* p = L.y + (n * L.Q + arg) * 3;
      y0 = p[0], y1 = p[1], y2 = p[2];
    }
    moments(m, 1.0, x0, x1, x2, y0, y1, y2, L.xmu + n * 4);
  }
  const double t = block_sum<kRec>(m, red);
  if (threadIdx.x < kRec) L.rec[(n * L.nblk + blockIdx.x) * kRec + threadIdx.x] = t;
}

// grid (query blocks, splits, N)
__global__ void __launch_bounds__(kThreads) icp_search_kernel(IcpLaunch L) {
  __shared__ __attribute__((aligned(16))) float tile[kTile * 3];
  __shared__ double red[kWaves][kRec];
  int it;
  if (icp_done(L, it)) return;
  const int64_t n = blockIdx.z;
  const int s = blockIdx.y;
  const int64_t qlen = cloud_len(L.x_len, n, L.P), dlen = cloud_len(L.y_len, n, L.Q);
  const int64_t lo = std::min<int64_t>((int64_t)s * L.chunk, dlen), hi = std::min<int64_t>(lo + L.chunk, dlen);
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < qlen;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    const float* p = L.x + (n * L.P + i) * 3;
    x0 = p[0], x1 = p[1], x2 = p[2];
    const float* t = L.state + n * kS;
    qx = t[12] * (x0 * t[0] + x1 * t[3] + x2 * t[6]) + t[9];
    qy = t[12] * (x0 * t[1] + x1 * t[4] + x2 * t[7]) + t[10];
    qz = t[12] * (x0 * t[2] + x1 * t[5] + x2 * t[8]) + t[11];
  }
  float best = INFINITY;
  int32_t arg = -1;
  const float* db = L.y + n * L.Q * 3;
  for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
    const int cnt = (int)std::min<int64_t>(kTile, hi - t0), cnt4 = (cnt + 3) & ~3;
    __syncthreads();  // the previous tile has been read
    for (int k = threadIdx.x; k < cnt4 * 3; k += kThreads) tile[k] = k < cnt * 3 ? db[t0 * 3 + k] : INFINITY;
    __syncthreads();
    const float4* t4 = reinterpret_cast<const float4*>(tile);
    const int32_t j0 = (int32_t)t0;
    for (int k = 0; k < cnt4; k += 4) {  // a padding point is at infinity: d = inf, never < best
      const float4 a = t4[(k >> 2) * 3], b = t4[(k >> 2) * 3 + 1], c = t4[(k >> 2) * 3 + 2];
      consider(qx, qy, qz, a.x, a.y, a.z, j0 + k, best, arg);
      consider(qx, qy, qz, a.w, b.x, b.y, j0 + k + 1, best, arg);
      consider(qx, qy, qz, b.z, b.w, c.x, j0 + k + 2, best, arg);
      consider(qx, qy, qz, c.y, c.z, c.w, j0 + k + 3, best, arg);
    }
  }
  if (!live) arg = -1;
  if (L.splits > 1) {
    if (i < L.P) L.part[(n * L.splits + s) * L.P + i] = Partial{best, arg};
    return;
  }
  finish_query(L, it, n, i, live, arg, x0, x1, x2, red);
}

// grid (query blocks, 1, N): the partials of a query in range order, the lowest index on a tie
__global__ void __launch_bounds__(kThreads) icp_merge_kernel(IcpLaunch L) {
  __shared__ double red[kWaves][kRec];
  int it;
  if (icp_done(L, it)) return;
  const int64_t n = blockIdx.z, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < cloud_len(L.x_len, n, L.P);
  float best = INFINITY, x0 = 0.f, x1 = 0.f, x2 = 0.f;
  int32_t arg = -1;
  if (live) {
    for (int s = 0; s < L.splits; ++s) {
      const Partial p = L.part[(n * L.splits + s) * L.P + i];
      if (p.idx >= 0 && p.d < best) {
        best = p.d;
        arg = p.idx;
      }
    }
    const float* p = L.x + (n * L.P + i) * 3;
    x0 = p[0], x1 = p[1], x2 = p[2];
  }
  finish_query(L, it, n, i, live, arg, x0, x1, x2, red);
}

// grid (query blocks, 1, N): the records of given correspondences and weights
__global__ void __launch_bounds__(kThreads) align_moments_kernel(AlignLaunch L) {
  __shared__ double red[kWaves][kRec];
  const int64_t n = blockIdx.z, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double m[kRec];
#pragma unroll
  for (int c = 0; c < kRec; ++c) m[c] = 0.0;
  if (i < cloud_len(L.x_len, n, L.P)) {
    const float* p = L.x + (n * L.P + i) * 3;
    const float* q = L.y + (n * L.P + i) * 3;
    moments(m, L.w ? (double)L.w[n * L.P + i] : 1.0, p[0], p[1], p[2], q[0], q[1], q[2], L.xmu + n * 4);
  }
  const double t = block_sum<kRec>(m, red);
  if (threadIdx.x < kRec) L.rec[(n * L.nblk + blockIdx.x) * kRec + threadIdx.x] = t;
}

// ------------------------------------------------------------------ the 3 x 3 solve
struct Mat3 {
  double a[3][3];
};

PR_HD double det3(const Mat3& M) {
  return M.a[0][0] * (M.a[1][1] * M.a[2][2] - M.a[1][2] * M.a[2][1]) -
         M.a[0][1] * (M.a[1][0] * M.a[2][2] - M.a[1][2] * M.a[2][0]) +
         M.a[0][2] * (M.a[1][0] * M.a[2][1] - M.a[1][1] * M.a[2][0]);
}

template <int P, int Q>
PR_HD void jacobi_pair(Mat3& A, Mat3& V) {
  double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) al += A.a[i][P] * A.a[i][P], be += A.a[i][Q] * A.a[i][Q], ga += A.a[i][P] * A.a[i][Q];
  if (!(fabs(ga) > 2.2e-16 * sqrt(al * be)) || ga == 0.0) return;  // orthogonal to rounding (or NaN)
  const double zeta = (be - al) / (2.0 * ga);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ap = A.a[i][P], aq = A.a[i][Q], vp = V.a[i][P], vq = V.a[i][Q];
    A.a[i][P] = c * ap - s * aq, A.a[i][Q] = s * ap + c * aq;
    V.a[i][P] = c * vp - s * vq, V.a[i][Q] = s * vp + c * vq;
  }
}

template <int P, int Q>
PR_HD void sort_pair(Mat3& A, Mat3& V, double (&S)[3]) {  // descending, stable
  if (!(S[P] < S[Q])) return;
  const double t = S[P];
  S[P] = S[Q], S[Q] = t;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = A.a[i][P], v = V.a[i][P];
    A.a[i][P] = A.a[i][Q], A.a[i][Q] = a;
    V.a[i][P] = V.a[i][Q], V.a[i][Q] = v;
  }
}

// C = U diag(S) V^T, S descending, U and V orthonormal (also for a rank-deficient C: the columns of
// U a rank leaves open are completed; the third is +-(u0 x u1), the sign from the Jacobi column)
PR_HD void svd3(const Mat3& C, Mat3& U, double (&S)[3], Mat3& V) {
  double scale = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) scale = fmax(scale, fabs(C.a[i][j]));
  Mat3 A;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A.a[i][j] = scale > 0.0 ? C.a[i][j] / scale : 0.0;
      V.a[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    jacobi_pair<0, 1>(A, V);
    jacobi_pair<0, 2>(A, V);
    jacobi_pair<1, 2>(A, V);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) S[j] = sqrt(A.a[0][j] * A.a[0][j] + A.a[1][j] * A.a[1][j] + A.a[2][j] * A.a[2][j]);
  sort_pair<0, 1>(A, V, S);
  sort_pair<1, 2>(A, V, S);
  sort_pair<0, 1>(A, V, S);
  double u0[3] = {1.0, 0.0, 0.0}, u1[3], u2[3];
  if (S[0] > 0.0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) u0[i] = A.a[i][0] / S[0];
  }
  // u1: the second column made orthogonal to u0; for a rank-1 matrix the axis least along u0 instead
  const int k = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
  const bool rank2 = S[1] > 1e-12 * S[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = rank2 ? A.a[i][1] / S[1] : (i == k ? 1.0 : 0.0);
  const double dot = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] -= dot * u0[i];
  const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] /= n1;
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
  u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
  u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  const double sgn = (u2[0] * A.a[0][2] + u2[1] * A.a[1][2] + u2[2] * A.a[2][2]) < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) U.a[i][0] = u0[i], U.a[i][1] = u1[i], U.a[i][2] = sgn * u2[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) S[j] *= scale;
}

struct Solution {
  double R[9], T[3], s, rmse;
};

// corresponding_points_alignment from a cloud's summed record m and its (Xmu, sum w); rmse: of the
// solved transform against the partners it was solved from, for 0 / 1 weights
PR_HD Solution solve_cloud(const double (&m)[kRec], const double* xmu, bool weighted, double eps, bool estimate_scale,
                            bool allow_reflection) {
  const double wsum = m[mW], wc = fmax(wsum, eps), total = weighted ? wc : fmax(wsum, 1.0);
  double ymu[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ymu[k] = (m[mY + k] + xmu[k] * wsum) / wc;
    d[k] = ymu[k] - xmu[k];
  }
  Mat3 M, C, U, V;  // M = sum w^2 xc (x) (y - Ymu)
  double check = m[mX2] + m[mY2];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      M.a[j][k] = m[mC + 3 * j + k] - m[mWX + j] * d[k];
      C.a[j][k] = M.a[j][k] / total;
      check += C.a[j][k] + ymu[k];
    }
  double S[3];
  svd3(C, U, S, V);
  const double e2 = allow_reflection ? 1.0 : (det3(U) * det3(V) < 0.0 ? -1.0 : 1.0);
  Solution o;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o.R[3 * j + k] = U.a[j][0] * V.a[k][0] + U.a[j][1] * V.a[k][1] + e2 * U.a[j][2] * V.a[k][2];
  o.s = estimate_scale ? (S[0] + S[1] + e2 * S[2]) / fmax(m[mX2] / total, eps) : 1.0;
  double tr = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.T[k] = ymu[k] - o.s * (xmu[0] * o.R[k] + xmu[1] * o.R[3 + k] + xmu[2] * o.R[6 + k]);
#pragma unroll
    for (int j = 0; j < 3; ++j) tr += o.R[3 * j + k] * M.a[j][k];
  }
  const double y2 = m[mY2] - 2.0 * (d[0] * m[mY] + d[1] * m[mY + 1] + d[2] * m[mY + 2]) +
                    wsum * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  o.rmse = sqrt(fmax(o.s * o.s * m[mX2] - 2.0 * o.s * tr + y2, 0.0) / wc);
  if (!(fabs(check) < INFINITY)) {  // a non-finite moment: nothing of this cloud is defined
#pragma unroll
    for (int k = 0; k < 9; ++k) o.R[k] = NAN;
    o.T[0] = o.T[1] = o.T[2] = o.s = o.rmse = NAN;
  }
  return o;
}

// the cloud's records in index order: lane c < kRec adds component c, then every lane gets all of them
PR_DEV void sum_records(const double* rec, int64_t nblk, double (&m)[kRec]) {
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  if (lane < kRec)
    for (int64_t b = 0; b < nblk; ++b) acc += rec[b * kRec + lane];
#pragma unroll
  for (int c = 0; c < kRec; ++c) m[c] = __shfl(acc, c, 64);
}

// grid (1): a wave per cloud
__global__ void __launch_bounds__(kThreads) icp_solve_kernel(IcpLaunch L) {
  __shared__ int ok[kWaves];
  int it;
  if (icp_done(L, it)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool all_ok = true;
  for (int64_t n = wave; n < L.N; n += kWaves) {
    double m[kRec];
    sum_records(L.rec + n * L.nblk * kRec, L.nblk, m);
    const Solution o = solve_cloud(m, L.xmu + n * 4, true, kIcpEps, L.estimate_scale != 0, L.allow_reflection != 0);
    const float rm = (float)o.rmse, prev = L.prev[n];
    const float rel = it == 0 ? 1.f : (prev - rm) / prev;
    all_ok = all_ok && rel <= L.thr;
    if (lane == 0) {
      float* st = L.state + n * kS;
      float* h = L.history + ((int64_t)it * L.N + n) * kS;
#pragma unroll
      for (int k = 0; k < 9; ++k) st[k] = h[k] = (float)o.R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) st[9 + k] = h[9 + k] = (float)o.T[k];
      st[12] = h[12] = (float)o.s;
      L.rmse[n] = rm;
      L.prev[n] = rm;
    }
  }
  if (lane == 0) ok[wave] = all_ok ? 1 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int conv = 1;
    for (int w = 0; w < kWaves; ++w) conv &= ok[w];
    L.flags[0] = conv;
    L.flags[1] = it + 1;
  }
}

// grid (1): a wave per cloud
__global__ void __launch_bounds__(kThreads) align_solve_kernel(AlignLaunch L) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t n = wave; n < L.N; n += kWaves) {
    double m[kRec];
    sum_records(L.rec + n * L.nblk * kRec, L.nblk, m);
    const Solution o = solve_cloud(m, L.xmu + n * 4, L.w != nullptr, L.eps, L.estimate_scale != 0, L.allow_reflection != 0);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) L.R[n * 9 + k] = (float)o.R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) L.T[n * 3 + k] = (float)o.T[k];
      L.s[n] = (float)o.s;
    }
  }
}

// grid (blocks of N P): xt = s (x R) + T for every row, padding included
__global__ void __launch_bounds__(kThreads) icp_apply_kernel(const float* x, const float* state, int64_t N, int64_t P, float* xt) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= N * P) return;
  const float* t = state + (e / P) * kS;
  const float x0 = x[e * 3], x1 = x[e * 3 + 1], x2 = x[e * 3 + 2];
  xt[e * 3] = t[12] * (x0 * t[0] + x1 * t[3] + x2 * t[6]) + t[9];
  xt[e * 3 + 1] = t[12] * (x0 * t[1] + x1 * t[4] + x2 * t[7]) + t[10];
  xt[e * 3 + 2] = t[12] * (x0 * t[2] + x1 * t[5] + x2 * t[8]) + t[11];
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

// database ranges for P queries per cloud against Q database points: enough workgroups to occupy
// the device, never more ranges than tiles; PR_ICP_SPLITS overrides (read per call)
int pick_splits(int64_t N, int64_t P, int64_t Q) {
  if (const char* e = getenv("PR_ICP_SPLITS")) {
    const int s = atoi(e);
    if (s > 0) return std::min(s, kMaxSplits);
  }
  const int64_t wgs = N * blocks_of(P), tiles = (Q + kTile - 1) / kTile;
  const int64_t want = (kTargetBlocks + wgs - 1) / wgs;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), kMaxSplits));
}

bool sizes_ok(int64_t N, int64_t P, int64_t Q) {
  return N > 0 && P > 0 && Q > 0 && N <= 65535 && P <= INT32_MAX && Q <= INT32_MAX && N * P <= (int64_t)INT32_MAX * kThreads;
}

// doubles ahead of the partials: (Xmu, sum w), the previous rmse (a float in a double's slot), the records
size_t head_doubles(int64_t N, int64_t P) { return (size_t)N * 5 + (size_t)N * (size_t)blocks_of(P) * kRec; }

size_t icp_bytes(int64_t N, int64_t P, int splits) {
  return head_doubles(N, P) * sizeof(double) + (splits > 1 ? (size_t)N * (size_t)splits * (size_t)P * sizeof(Partial) : 0);
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_align_workspace(int64_t N, int64_t P) {
  return sizes_ok(N, P, 1) ? head_doubles(N, P) * sizeof(double) : 0;
}

extern "C" size_t pr_icp_workspace(int64_t N, int64_t P, int64_t Q) {
  return sizes_ok(N, P, Q) ? icp_bytes(N, P, pick_splits(N, P, Q)) : 0;
}

extern "C" int pr_align_solve_host(const double* record, const double* xmu, int32_t weighted, double eps,
                                   int32_t estimate_scale, int32_t allow_reflection, double* out) {
  if (!record || !xmu || !out) return set_error(PR_ERR_ARG, "align_solve_host: record / xmu / out missing");
  if (!(eps > 0.0)) return set_error(PR_ERR_ARG, "align_solve_host: eps must be positive");
  double m[kRec];
  for (int c = 0; c < kRec; ++c) m[c] = record[c];
  const Solution o = solve_cloud(m, xmu, weighted != 0, eps, estimate_scale != 0, allow_reflection != 0);
  for (int k = 0; k < 9; ++k) out[k] = o.R[k];
  for (int k = 0; k < 3; ++k) out[9 + k] = o.T[k];
  out[12] = o.s, out[13] = o.rmse;
  return PR_OK;
}

extern "C" int pr_align_fwd(const PRAlignArgs* args, void* stream) {
  if (!args) return set_error(PR_ERR_ARG, "align_fwd: null args");
  const PRAlignArgs& a = *args;
  if (a.N <= 0 || a.P <= 0) return set_error(PR_ERR_ARG, "align_fwd: N and P must be positive");
  if (!sizes_ok(a.N, a.P, 1)) return set_error(PR_ERR_ARG, "align_fwd: P must fit int32 and N the grid (65535)");
  if (!a.x || !a.y) return set_error(PR_ERR_ARG, "align_fwd: x / y missing");
  if (!a.R || !a.T || !a.s) return set_error(PR_ERR_ARG, "align_fwd: R / T / s missing");
  if (!(a.eps > 0.0)) return set_error(PR_ERR_ARG, "align_fwd: eps must be positive");
  const size_t need = pr_align_workspace(a.N, a.P);
  if (!a.workspace || a.workspace_bytes < need)
    return set_error(PR_ERR_WORKSPACE, "align_fwd: workspace missing or smaller than pr_align_workspace (" +
                                           std::to_string(need) + " bytes)");
  double* ws = static_cast<double*>(a.workspace);
  AlignLaunch L{a.x, a.y, a.weights, a.x_len, a.N, a.P, blocks_of(a.P), a.estimate_scale, a.allow_reflection, a.eps,
                a.R, a.T, a.s, ws, ws + a.N * 5};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  centroid_kernel<<<dim3((unsigned)a.N), kThreads, 0, st>>>(a.x, a.weights, a.x_len, a.P, a.eps, L.xmu, nullptr, nullptr);
  if (int e = check_launch("align_centroid")) return e;
  align_moments_kernel<<<dim3((unsigned)L.nblk, 1, (unsigned)a.N), kThreads, 0, st>>>(L);
  if (int e = check_launch("align_moments")) return e;
  align_solve_kernel<<<dim3(1), kThreads, 0, st>>>(L);
  return check_launch("align_solve");
}

extern "C" int pr_icp_run(const PRIcpArgs* args, int32_t iterations, void* stream) {
  if (!args) return set_error(PR_ERR_ARG, "icp_run: null args");
  const PRIcpArgs& a = *args;
  if (a.N <= 0 || a.P <= 0 || a.Q <= 0) return set_error(PR_ERR_ARG, "icp_run: N, P and Q must be positive");
  if (!sizes_ok(a.N, a.P, a.Q)) return set_error(PR_ERR_ARG, "icp_run: P, Q must fit int32 and N the grid (65535)");
  if (a.max_iterations <= 0) return set_error(PR_ERR_ARG, "icp_run: max_iterations must be positive");
  if (iterations < 0 || iterations > a.max_iterations)
    return set_error(PR_ERR_ARG, "icp_run: iterations must be in [0, max_iterations]");
  if ((a.phase & ~(PR_ICP_BEGIN | PR_ICP_END)) != 0) return set_error(PR_ERR_ARG, "icp_run: phase must be PR_ICP_BEGIN | PR_ICP_END bits");
  if (!a.x || !a.y) return set_error(PR_ERR_ARG, "icp_run: x / y missing");
  if (!a.state || !a.history || !a.rmse || !a.idx || !a.flags) return set_error(PR_ERR_ARG, "icp_run: state / history / rmse / idx / flags missing");
  if ((a.phase & PR_ICP_END) && !a.xt) return set_error(PR_ERR_ARG, "icp_run: xt missing");
  const int splits = pick_splits(a.N, a.P, a.Q);
  const size_t need = icp_bytes(a.N, a.P, splits);
  if (!a.workspace || a.workspace_bytes < need)
    return set_error(PR_ERR_WORKSPACE, "icp_run: workspace missing or smaller than pr_icp_workspace (" +
                                           std::to_string(need) + " bytes)");
  double* ws = static_cast<double*>(a.workspace);
  IcpLaunch L;
  L.x = a.x, L.y = a.y, L.x_len = a.x_len, L.y_len = a.y_len;
  L.N = a.N, L.P = a.P, L.Q = a.Q;
  L.max_iterations = a.max_iterations, L.estimate_scale = a.estimate_scale, L.allow_reflection = a.allow_reflection;
  L.thr = a.relative_rmse_thr;
  L.state = a.state, L.history = a.history, L.rmse = a.rmse, L.idx = a.idx, L.idx_history = a.idx_history;
  L.flags = a.flags;
  L.splits = splits, L.chunk = (a.Q + splits - 1) / splits, L.nblk = blocks_of(a.P);
  L.xmu = ws, L.prev = reinterpret_cast<float*>(ws + a.N * 4), L.rec = ws + a.N * 5;
  L.part = reinterpret_cast<Partial*>(ws + head_doubles(a.N, a.P));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.phase & PR_ICP_BEGIN) {
    centroid_kernel<<<dim3((unsigned)a.N), kThreads, 0, st>>>(a.x, nullptr, a.x_len, a.P, kIcpEps, L.xmu, L.prev, a.flags);
    if (int e = check_launch("icp_centroid")) return e;
  }
  for (int k = 0; k < iterations; ++k) {
    icp_search_kernel<<<dim3((unsigned)L.nblk, (unsigned)splits, (unsigned)a.N), kThreads, 0, st>>>(L);
    if (int e = check_launch("icp_search")) return e;
    if (splits > 1) {
      icp_merge_kernel<<<dim3((unsigned)L.nblk, 1, (unsigned)a.N), kThreads, 0, st>>>(L);
      if (int e = check_launch("icp_merge")) return e;
    }
    icp_solve_kernel<<<dim3(1), kThreads, 0, st>>>(L);
    if (int e = check_launch("icp_solve")) return e;
  }
  if (a.phase & PR_ICP_END) {
    icp_apply_kernel<<<dim3((unsigned)blocks_of(a.N * a.P)), kThreads, 0, st>>>(a.x, a.state, a.N, a.P, a.xt);
    return check_launch("icp_apply");
  }
  return PR_OK;
}
