// Chamfer distance between padded point clouds x (N,P,3) and y (N,Q,3) (PyTorch3D 0.4.0
// chamfer_distance's nearest-neighbour core, K = 1), forward and backward, both directions per call.
//
// Forward: one lane per query point.  The other cloud (the database) is staged through LDS in tiles
// of kTile points; every lane of the workgroup walks the tile in index order (all lanes read the
// same address: an LDS broadcast, 3 ds_read_b128 per 4 points) and keeps a running (min, argmin) of
// d^2 = dx^2 + dy^2 + dz^2 formed from the coordinate differences, so a query on top of a database
// point gives exactly 0.  The comparison is a strict <, in ascending index: the lowest index wins on
// equal d^2.  There is no cross-lane reduction.  When the query grid alone would leave the device
// idle (few queries, many database points) the database is cut into S contiguous ranges over
// gridDim.y; the partial (min, argmin) pairs go to the workspace and a merge pass walks them in
// range order with the same strict <, so the tie rule holds at every level.  Lengths are read on
// the device (no host read: capturable); a query at or past its cloud's length, and every query of
// a cloud whose database is empty, gets d = 0, idx = -1.  NaN database points are never chosen
// (torch.min would propagate them); a query that can choose nothing gets a non-finite d (no_neighbour).
//
// Backward: grad_x[i] = 2 g_dx[i] (x_i - y_nn(i)) + sum over j ascending with idx_y[j] = i of
// 2 g_dy[j] (x_i - y_j), grad_y the mirror.  The second term is a scatter done as a gather: the
// other side's idx array goes through LDS tiles (with its incoming gradient and its points, so a
// match reads LDS only) and every lane compares it with its own index (4 compares per
// ds_read_b128).  The j are cut into the same ranges as the forward's database; a range sums its
// matches in ascending j and the ranges are added in order.  No atomics, a fixed order: the same
// bits on every call.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "pr_common.h"

namespace pr {
namespace {

#ifndef PR_CHAMFER_TILE
#define PR_CHAMFER_TILE 512
#endif
constexpr int kTile = PR_CHAMFER_TILE;      // database points per LDS tile (6 KiB); a multiple of 4
constexpr int kIdxTile = 512;               // backward: entries per LDS tile (idx, gradient, point: 10 KiB)
constexpr int kTargetBlocks = 2048;         // workgroups wanted on a 256-CU part (8 per CU: 8 waves per SIMD)
constexpr int kMaxSplits = 64;
static_assert(kTile % 4 == 0 && kIdxTile % 4 == 0, "tiles are read as float4 / int4");

struct Partial {
  float d;
  int32_t idx;
};

struct Dir {  // one direction of the call: queries q (n, nq, 3) against the database db (n, ndb, 3)
  const float* q;
  const float* db;
  const int64_t* q_len;
  const int64_t* db_len;
  int64_t nq, ndb;
  int splits;
  int64_t chunk;  // database points per split
  float* dist;
  int32_t* idx;
  Partial* part;  // (n, splits, nq) when splits > 1
};

struct FwdLaunch {
  Dir dir[2];
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

// The distance of a query that found no neighbour.  Padding, or an empty database: 0.  A live query
// of a non-empty database finds none only when no d^2 compared below +inf (NaN or overflowing
// coordinates, for instance after a diverged step): the distance is then not finite, NaN where the
// query itself is NaN and +inf otherwise, so the loss shows it; idx stays -1 and the gradient 0.
PR_DEV float no_neighbour(bool searched, float qx, float qy, float qz) {
  if (!searched) return 0.f;
  return (qx != qx || qy != qy || qz != qz) ? NAN : INFINITY;
}

// grid (query blocks, splits, 2 N): blockIdx.z = 2 n + direction
__global__ void __launch_bounds__(kThreads) chamfer_fwd_kernel(FwdLaunch L) {
  __shared__ __attribute__((aligned(16))) float tile[kTile * 3];
  const Dir& D = L.dir[blockIdx.z & 1];
  const int64_t n = blockIdx.z >> 1;
  const int s = blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * kThreads;
  if (q0 >= D.nq || s >= D.splits) return;  // uniform over the workgroup
  const int64_t qlen = cloud_len(D.q_len, n, D.nq), dlen = cloud_len(D.db_len, n, D.ndb);
  const int64_t lo = std::min<int64_t>((int64_t)s * D.chunk, dlen), hi = std::min<int64_t>(lo + D.chunk, dlen);
  const int64_t i = q0 + threadIdx.x;
  const bool live = i < qlen;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    const float* p = D.q + (n * D.nq + i) * 3;
    qx = p[0], qy = p[1], qz = p[2];
  }
  float best = INFINITY;
  int32_t arg = -1;
  const float* db = D.db + n * D.ndb * 3;
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
  if (i >= D.nq) return;
  if (!live) arg = -1;
  if (D.splits > 1) {
    D.part[(n * D.splits + s) * D.nq + i] = Partial{best, arg};
  } else {
    D.dist[n * D.nq + i] = arg < 0 ? no_neighbour(live && dlen > 0, qx, qy, qz) : best;
    D.idx[n * D.nq + i] = arg;
  }
}

// grid (query blocks, 1, 2 N): the partials of a query in range order, the lowest index on a tie
__global__ void __launch_bounds__(kThreads) chamfer_merge_kernel(FwdLaunch L) {
  const Dir& D = L.dir[blockIdx.z & 1];
  const int64_t n = blockIdx.z >> 1, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (D.splits <= 1 || i >= D.nq) return;
  float best = INFINITY;
  int32_t arg = -1;
  for (int s = 0; s < D.splits; ++s) {
    const Partial p = D.part[(n * D.splits + s) * D.nq + i];
    if (p.idx >= 0 && p.d < best) {
      best = p.d;
      arg = p.idx;
    }
  }
  float miss = 0.f;
  if (arg < 0 && i < cloud_len(D.q_len, n, D.nq) && cloud_len(D.db_len, n, D.ndb) > 0) {
    const float* p = D.q + (n * D.nq + i) * 3;
    miss = no_neighbour(true, p[0], p[1], p[2]);
  }
  D.dist[n * D.nq + i] = arg < 0 ? miss : best;
  D.idx[n * D.nq + i] = arg;
}

struct BwdDir {  // d / d a (n, na, 3), the other cloud b (n, nb, 3)
  const float* a;
  const float* b;
  const int64_t* a_len;
  const int64_t* b_len;
  int64_t na, nb;
  const int32_t* idx_a;  // (n, na): a's nearest in b
  const int32_t* idx_b;  // (n, nb): b's nearest in a
  const float* g_a;      // (n, na) d loss / d dist_a
  const float* g_b;
  int splits;
  int64_t chunk;         // entries of idx_b per split
  float* grad;           // (n, na, 3)
  float* part;           // (n, splits, na, 3) when splits > 1
};

struct BwdLaunch {
  BwdDir dir[2];
};

// grid (point blocks, splits, 2 N).  A tile holds kIdxTile entries of the other side: its idx, its
// incoming gradient and its points, so a match reads LDS only.
__global__ void __launch_bounds__(kThreads) chamfer_bwd_kernel(BwdLaunch L) {
  __shared__ __attribute__((aligned(16))) int32_t tile[kIdxTile];
  __shared__ float tile_g[kIdxTile];
  __shared__ float tile_b[kIdxTile * 3];
  const BwdDir& D = L.dir[blockIdx.z & 1];
  const int64_t n = blockIdx.z >> 1;
  const int s = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * kThreads;
  if (i0 >= D.na || s >= D.splits) return;  // uniform over the workgroup
  const int64_t alen = cloud_len(D.a_len, n, D.na), blen = cloud_len(D.b_len, n, D.nb);
  const int64_t lo = std::min<int64_t>((int64_t)s * D.chunk, blen), hi = std::min<int64_t>(lo + D.chunk, blen);
  const int64_t i = i0 + threadIdx.x;
  const bool live = i < alen;
  const float* b = D.b + n * D.nb * 3;
  float ax = 0.f, ay = 0.f, az = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  if (live) {
    const float* p = D.a + (n * D.na + i) * 3;
    ax = p[0], ay = p[1], az = p[2];
    const int32_t j = D.idx_a[n * D.na + i];
    if (s == 0 && j >= 0) {  // the point's own nearest neighbour: the first range's first term
      const float g = 2.f * D.g_a[n * D.na + i];
      gx = g * (ax - b[(int64_t)j * 3]), gy = g * (ay - b[(int64_t)j * 3 + 1]), gz = g * (az - b[(int64_t)j * 3 + 2]);
    }
  }
  const int32_t me = live ? (int32_t)i : -2;  // padded entries of idx_b are -1: never equal
  const int32_t* idx_b = D.idx_b + n * D.nb;
  const float* g_b = D.g_b + n * D.nb;
  for (int64_t t0 = lo; t0 < hi; t0 += kIdxTile) {
    const int cnt = (int)std::min<int64_t>(kIdxTile, hi - t0), cnt4 = (cnt + 3) & ~3;
    __syncthreads();
    for (int k = threadIdx.x; k < cnt4; k += kThreads) {
      tile[k] = k < cnt ? idx_b[t0 + k] : -1;
      if (k < cnt) tile_g[k] = g_b[t0 + k];
    }
    for (int k = threadIdx.x; k < cnt * 3; k += kThreads) tile_b[k] = b[t0 * 3 + k];
    __syncthreads();
    const int4* t4 = reinterpret_cast<const int4*>(tile);
    for (int k = 0; k < cnt4; k += 4) {
      const int4 v = t4[k >> 2];
      if (v.x == me || v.y == me || v.z == me || v.w == me) {
        const int32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (w[c] != me) continue;  // a match is below cnt: the padding is -1
          const int j = k + c;
          const float g = 2.f * tile_g[j];
          gx += g * (ax - tile_b[j * 3]), gy += g * (ay - tile_b[j * 3 + 1]), gz += g * (az - tile_b[j * 3 + 2]);
        }
      }
    }
  }
  if (i < D.na) {
    float* o = D.splits > 1 ? D.part + ((n * D.splits + s) * D.na + i) * 3 : D.grad + (n * D.na + i) * 3;
    o[0] = gx, o[1] = gy, o[2] = gz;
  }
}

// grid (point blocks, 1, 2 N): the ranges' partial gradients in range order
__global__ void __launch_bounds__(kThreads) chamfer_bwd_merge_kernel(BwdLaunch L) {
  const BwdDir& D = L.dir[blockIdx.z & 1];
  const int64_t n = blockIdx.z >> 1, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (D.splits <= 1 || i >= D.na) return;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int s = 0; s < D.splits; ++s) {
    const float* p = D.part + ((n * D.splits + s) * D.na + i) * 3;
    gx += p[0], gy += p[1], gz += p[2];
  }
  float* o = D.grad + (n * D.na + i) * 3;
  o[0] = gx, o[1] = gy, o[2] = gz;
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

// database ranges for nq queries per cloud against ndb database points: enough workgroups to
// occupy the device, never more ranges than tiles; PR_CHAMFER_SPLITS overrides (read per call)
int pick_splits(int64_t N, int64_t nq, int64_t ndb) {
  if (const char* e = getenv("PR_CHAMFER_SPLITS")) {
    const int s = atoi(e);
    if (s > 0) return std::min(s, kMaxSplits);
  }
  const int64_t wgs = N * blocks_of(nq), tiles = (ndb + kTile - 1) / kTile;
  const int64_t want = (kTargetBlocks + wgs - 1) / wgs;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), kMaxSplits));
}

// per (point, range): a (min, argmin) pair forward, a partial gradient backward; one size serves both
constexpr size_t kPartBytes = 3 * sizeof(float);
static_assert(sizeof(Partial) <= kPartBytes, "the forward's partials fit the backward's slots");
size_t part_bytes(int64_t N, int64_t nq, int splits) {
  return splits > 1 ? (size_t)N * (size_t)nq * (size_t)splits * kPartBytes : 0;
}

int chamfer_check(const PRChamferArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (a->N <= 0 || a->P <= 0 || a->Q <= 0) return set_error(PR_ERR_ARG, w + ": N, P and Q must be positive");
  if (a->P > INT32_MAX || a->Q > INT32_MAX || a->N > 32767)
    return set_error(PR_ERR_ARG, w + ": P, Q must fit int32 and N the grid (32767)");
  if (!a->x || !a->y) return set_error(PR_ERR_ARG, w + ": x / y missing");
  if (!a->idx_x || !a->idx_y) return set_error(PR_ERR_ARG, w + ": idx_x / idx_y missing");
  if (fwd && (!a->dist_x || !a->dist_y)) return set_error(PR_ERR_ARG, w + ": dist_x / dist_y missing");
  if (!fwd && (!a->grad_dist_x || !a->grad_dist_y || !a->grad_x || !a->grad_y))
    return set_error(PR_ERR_ARG, w + ": grads missing");
  return PR_OK;
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_chamfer_workspace(int64_t N, int64_t P, int64_t Q) {
  if (N <= 0 || P <= 0 || Q <= 0) return 0;
  return part_bytes(N, P, pick_splits(N, P, Q)) + part_bytes(N, Q, pick_splits(N, Q, P));
}

extern "C" int pr_chamfer_fwd(const PRChamferArgs* args, void* stream) {
  if (int e = chamfer_check(args, "chamfer_fwd", true)) return e;
  const PRChamferArgs& a = *args;
  const int sx = pick_splits(a.N, a.P, a.Q), sy = pick_splits(a.N, a.Q, a.P);
  const size_t bx = part_bytes(a.N, a.P, sx), by = part_bytes(a.N, a.Q, sy);
  if (bx + by > 0 && (!a.workspace || a.workspace_bytes < bx + by))
    return set_error(PR_ERR_ARG, "chamfer_fwd: workspace missing or smaller than pr_chamfer_workspace (" +
                                     std::to_string(bx + by) + " bytes)");
  char* ws = static_cast<char*>(a.workspace);
  FwdLaunch L;
  L.dir[0] = Dir{a.x, a.y, a.x_len, a.y_len, a.P, a.Q, sx, (a.Q + sx - 1) / sx, a.dist_x, a.idx_x,
                 reinterpret_cast<Partial*>(ws)};
  L.dir[1] = Dir{a.y, a.x, a.y_len, a.x_len, a.Q, a.P, sy, (a.P + sy - 1) / sy, a.dist_y, a.idx_y,
                 reinterpret_cast<Partial*>(ws + bx)};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned qb = (unsigned)blocks_of(std::max(a.P, a.Q));
  chamfer_fwd_kernel<<<dim3(qb, (unsigned)std::max(sx, sy), (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
  if (int e = check_launch("chamfer_fwd")) return e;
  if (sx > 1 || sy > 1) {
    chamfer_merge_kernel<<<dim3(qb, 1, (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
    return check_launch("chamfer_merge");
  }
  return PR_OK;
}

extern "C" int pr_chamfer_bwd(const PRChamferArgs* args, void* stream) {
  if (int e = chamfer_check(args, "chamfer_bwd", false)) return e;
  const PRChamferArgs& a = *args;
  const int sx = pick_splits(a.N, a.P, a.Q), sy = pick_splits(a.N, a.Q, a.P);
  const size_t bx = part_bytes(a.N, a.P, sx), by = part_bytes(a.N, a.Q, sy);
  if (bx + by > 0 && (!a.workspace || a.workspace_bytes < bx + by))
    return set_error(PR_ERR_ARG, "chamfer_bwd: workspace missing or smaller than pr_chamfer_workspace (" +
                                     std::to_string(bx + by) + " bytes)");
  char* ws = static_cast<char*>(a.workspace);
  BwdLaunch L;
  L.dir[0] = BwdDir{a.x, a.y, a.x_len, a.y_len, a.P, a.Q, a.idx_x, a.idx_y, a.grad_dist_x, a.grad_dist_y,
                    sx, (a.Q + sx - 1) / sx, a.grad_x, reinterpret_cast<float*>(ws)};
  L.dir[1] = BwdDir{a.y, a.x, a.y_len, a.x_len, a.Q, a.P, a.idx_y, a.idx_x, a.grad_dist_y, a.grad_dist_x,
                    sy, (a.P + sy - 1) / sy, a.grad_y, reinterpret_cast<float*>(ws + bx)};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned pb = (unsigned)blocks_of(std::max(a.P, a.Q));
  chamfer_bwd_kernel<<<dim3(pb, (unsigned)std::max(sx, sy), (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
  if (int e = check_launch("chamfer_bwd")) return e;
  if (sx > 1 || sy > 1) {
    chamfer_bwd_merge_kernel<<<dim3(pb, 1, (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
    return check_launch("chamfer_bwd_merge");
  }
  return PR_OK;
}
