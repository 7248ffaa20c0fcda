// Point-to-mesh distances between a packed batch of point clouds and a packed batch of meshes
// (PyTorch3D 0.4.0 point_mesh_face_distance / point_mesh_edge_distance: the squared distance of
// every point to its mesh's nearest primitive and of every primitive to its cloud's nearest point),
// forward and backward, both directions per call.  A primitive is a triangle verts[faces] (prim 0)
// or a segment verts[edges] (prim 1).
//
// Arithmetic (point_triangle / point_segment below; renderer/loss.py restates it in torch).  The
// Voronoi region of the point is classified from the signs of the edge dot products (Ericson's
// closest-point-on-triangle tests, in his order), which gives the weights w of the closest point
// q = sum w_i v_i.  In a vertex or edge region r = sum w_i (p - v_i), so a point on a vertex gives
// exactly 0.  In the interior the point is projected first: n = (v1 - v0) x (v2 - v0),
// t = n . (p - v0) / |n|^2, r = t n, and the weights come from the projected point's cross
// products against n.  d^2 = |r|^2.  A triangle with |n|^2 <= kDegenerate is evaluated as its three
// segments (v0 v1), (v1 v2), (v2 v0), the first of equal ones; a zero-length segment falls into its
// first endpoint's region.  Comparing squared distances to choose the region would lose half of
// float32's digits.
//
// Forward.  A first pass writes one record per primitive (its corners, and for a triangle n and
// 1 / |n|^2) into the workspace.  Then one launch covers both directions, one lane per query: a
// point walks its mesh's records, a primitive (its record in registers) walks its cloud's points.
// The other side is staged through LDS tiles that every lane reads at the same address (a
// broadcast) in ascending index, with a running (min, argmin) under a strict <: the lowest index
// wins on equal d^2, a NaN candidate is never chosen.  The batch elements' first / count tables are
// read on the device (nothing is read back: capturable).  With few queries and a long other side
// that side is cut into ranges over gridDim.y and the partial pairs are merged in range order with
// the same strict <, as in pr_chamfer.hip.  The winner is evaluated once more for its weights.
//
// Backward, three launches, no atomics, every sum in a fixed order: the same bits on every call.
// With g the incoming gradients, d d^2 / d p = 2 r and d d^2 / d v_i = -2 w_i r (the forward's
// weights; r is evaluated again by the forward's function).  (1) One wave per primitive sums the
// points that chose it (the caller's primitive -> points CSR, a stable sort of idx_p: lane l takes
// entries l, l + 64, ... in ascending order, then a fixed xor tree) and adds the primitive's own
// term into per-primitive corner gradients.  (2) One lane per point adds its own term and the
// primitives that chose it (the point -> primitives CSR, a stable sort of idx_m) in ascending
// order.  (3) One lane per vertex gathers its corners over the vertex -> corners CSR.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "pr_common.h"

namespace pr {
namespace {

constexpr int kTileFloats = 2048;     // one LDS tile (8 KiB): 128 triangles, 256 segments or 512 points
constexpr int kPointTile = 512;
constexpr int kTargetBlocks = 2048;   // workgroups wanted on a 256-CU part, as pr_chamfer.hip
constexpr int kMaxSplits = 64;
constexpr int kWaves = kThreads / 64;
constexpr float kDegenerate = 1e-30f;  // |n|^2 at or below: the triangle is its three segments

struct F3 {
  float x, y, z;
};
PR_DEV F3 load3(const float* p, int64_t i) { return F3{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]}; }
PR_DEV void store3(float* p, int64_t i, F3 v) { p[i * 3] = v.x; p[i * 3 + 1] = v.y; p[i * 3 + 2] = v.z; }
PR_DEV F3 sub(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PR_DEV F3 add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PR_DEV F3 scale3(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
PR_DEV void acc3(F3& a, F3 b) { a.x += b.x; a.y += b.y; a.z += b.z; }
PR_DEV F3 cross3(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PR_DEV float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PR_DEV bool nan3(F3 a) { return a.x != a.x || a.y != a.y || a.z != a.z; }

PR_DEV float wave_sum(float v) {  // a fixed xor tree over the 64 lanes
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
PR_DEV F3 wave_sum3(F3 v) { return F3{wave_sum(v.x), wave_sum(v.y), wave_sum(v.z)}; }

struct Hit {
  float d;  // |r|^2
  F3 w;     // weights of the closest point on the primitive's corners
  F3 r;     // p - closest point
};

// closest point of segment (a, b): the weights are (1 - v, v, 0)
PR_DEV Hit point_segment(F3 p, F3 a, F3 b) {
  const F3 ab = sub(b, a), ap = sub(p, a), bp = sub(p, b);
  const float d1 = dot3(ab, ap), d3 = dot3(ab, bp);
  float v;
  if (d1 <= 0.f) {  // a's region; a zero-length segment lands here
    v = 0.f;
  } else if (d3 >= 0.f) {
    v = 1.f;
  } else {
    v = d1 / (d1 - d3);  // d1 > 0 > d3, or NaN
  }
  Hit h;
  h.w = F3{1.f - v, v, 0.f};
  h.r = add(scale3(ap, h.w.x), scale3(bp, h.w.y));
  h.d = dot3(h.r, h.r);
  return h;
}

PR_DEV Hit point_triangle(F3 p, F3 a, F3 b, F3 c, F3 n, float inv_n2) {
  if (inv_n2 == 0.f) {  // degenerate: the first of its three segments that is nearest
    Hit h = point_segment(p, a, b);
    const Hit h1 = point_segment(p, b, c);
    if (h1.d < h.d) {
      h = h1;
      h.w = F3{0.f, h1.w.x, h1.w.y};
    }
    const Hit h2 = point_segment(p, c, a);
    if (h2.d < h.d) {
      h = h2;
      h.w = F3{h2.w.y, 0.f, h2.w.x};
    }
    return h;
  }
  const F3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp),
              d6 = dot3(ac, cp);
  Hit h;
  bool interior = false;
  if (d1 <= 0.f && d2 <= 0.f) {
    h.w = F3{1.f, 0.f, 0.f};
  } else if (d3 >= 0.f && d4 <= d3) {
    h.w = F3{0.f, 1.f, 0.f};
  } else if (d1 * d4 - d3 * d2 <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    const float den = d1 - d3, v = den > 0.f ? d1 / den : 0.f;
    h.w = F3{1.f - v, v, 0.f};
  } else if (d6 >= 0.f && d5 <= d6) {
    h.w = F3{0.f, 0.f, 1.f};
  } else if (d5 * d2 - d1 * d6 <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    const float den = d2 - d6, v = den > 0.f ? d2 / den : 0.f;
    h.w = F3{1.f - v, 0.f, v};
  } else if (d3 * d6 - d5 * d4 <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
    const float den = (d4 - d3) + (d5 - d6), v = den > 0.f ? (d4 - d3) / den : 0.f;
    h.w = F3{0.f, 1.f - v, v};
  } else {  // every test fails for a NaN as well: d is then NaN and the candidate is never chosen
    interior = true;
  }
  if (interior) {
    const float t = dot3(n, ap) * inv_n2;
    h.r = scale3(n, t);
    const F3 q = sub(ap, h.r);  // the projected point, from a
    const float w1 = dot3(n, cross3(q, ac)) * inv_n2, w2 = dot3(n, cross3(ab, q)) * inv_n2;
    h.w = F3{1.f - w1 - w2, w1, w2};
  } else {
    h.r = add(add(scale3(ap, h.w.x), scale3(bp, h.w.y)), scale3(cp, h.w.z));
  }
  h.d = dot3(h.r, h.r);
  return h;
}

// A primitive's record: PRIM 0 a, b, c, n, 1 / |n|^2 (0: degenerate) in 16 floats; PRIM 1 a, b in 8.
struct Rec {
  F3 a, b, c, n;
  float inv;
};
template <int PRIM>
constexpr int rec_floats() {
  return PRIM == 0 ? 16 : 8;
}

template <int PRIM>
PR_DEV Rec make_rec(const float* verts, const int64_t* prims, int64_t m, int64_t V) {
  constexpr int K = PRIM == 0 ? 3 : 2;
  const F3 bad{NAN, NAN, NAN};  // a vertex id outside [0, V): never chosen
  Rec r;
  const int64_t i0 = prims[m * K], i1 = prims[m * K + 1];
  r.a = i0 >= 0 && i0 < V ? load3(verts, i0) : bad;
  r.b = i1 >= 0 && i1 < V ? load3(verts, i1) : bad;
  r.c = r.n = F3{0.f, 0.f, 0.f};
  r.inv = 0.f;
  if (PRIM == 0) {
    const int64_t i2 = prims[m * K + 2];
    r.c = i2 >= 0 && i2 < V ? load3(verts, i2) : bad;
    r.n = cross3(sub(r.b, r.a), sub(r.c, r.a));
    const float n2 = dot3(r.n, r.n);
    r.inv = n2 > kDegenerate ? 1.f / n2 : 0.f;  // false for a NaN: its segments give NaN
  }
  return r;
}

template <int PRIM>
PR_DEV void write_rec(float* dst, const Rec& r) {
  dst[0] = r.a.x, dst[1] = r.a.y, dst[2] = r.a.z, dst[3] = r.b.x, dst[4] = r.b.y, dst[5] = r.b.z;
  if (PRIM == 0) {
    dst[6] = r.c.x, dst[7] = r.c.y, dst[8] = r.c.z, dst[9] = r.n.x, dst[10] = r.n.y, dst[11] = r.n.z;
    dst[12] = r.inv, dst[13] = dst[14] = dst[15] = 0.f;
  } else {
    dst[6] = dst[7] = 0.f;
  }
}

template <int PRIM>
PR_DEV Rec read_rec(const float* src) {  // 16-byte aligned: global, or LDS at one address per wave
  const float4* s = reinterpret_cast<const float4*>(src);
  const float4 x = s[0], y = s[1];
  Rec r;
  r.a = F3{x.x, x.y, x.z};
  r.b = F3{x.w, y.x, y.y};
  r.c = r.n = F3{0.f, 0.f, 0.f};
  r.inv = 0.f;
  if (PRIM == 0) {
    const float4 z = s[2], u = s[3];
    r.c = F3{y.z, y.w, z.x};
    r.n = F3{z.y, z.z, z.w};
    r.inv = u.x;
  }
  return r;
}

template <int PRIM>
PR_DEV Hit eval(F3 p, const Rec& r) {
  if (PRIM == 0) return point_triangle(p, r.a, r.b, r.c, r.n, r.inv);
  return point_segment(p, r.a, r.b);
}

template <int PRIM>
PR_DEV bool nan_rec(const Rec& r) {
  return nan3(r.a) || nan3(r.b) || (PRIM == 0 && nan3(r.c));
}

// One side of the call: batch element n owns [first[n], first[n] + count[n]) of a packed list of
// `total` entries; cap bounds every count (the host's grid).  first NULL: n cap; count NULL: cap.
struct Side {
  const int64_t* first;
  const int64_t* count;
  int64_t total, cap;
};

PR_DEV void segment_of(const Side& s, int64_t n, int64_t& first, int64_t& count) {
  const int64_t f = s.first ? s.first[n] : n * s.cap, c = s.count ? s.count[n] : s.cap;
  first = std::min<int64_t>(std::max<int64_t>(f, 0), s.total);
  count = std::min<int64_t>(std::max<int64_t>(c, 0), std::min<int64_t>(s.cap, s.total - first));
}

struct Partial {
  float d;
  int32_t idx;
};

struct FwdLaunch {
  const float* points;  // (P,3)
  const float* rec;     // (M, rec_floats)
  Side side[2];         // 0: points, 1: primitives; direction d queries side[d] against side[1 - d]
  int splits[2];
  int64_t chunk[2];     // entries of the other side per range
  float* dist[2];
  int32_t* idx[2];
  float* w[2];
  Partial* part[2];     // (splits, total) when splits > 1
  int pad_fill;         // the points are a padded batch: rows at or past a cloud's count get 0 / -1
};

// the outputs of packed query g of direction dir, whose search ended with (best, arg)
template <int PRIM>
PR_DEV void finish(const FwdLaunch& L, int dir, int64_t g, float best, int32_t arg, bool searched) {
  F3 w{0.f, 0.f, 0.f};
  float d = 0.f;
  if (arg >= 0) {
    const int64_t ip = dir == 0 ? g : arg, im = dir == 0 ? arg : g;
    w = eval<PRIM>(load3(L.points, ip), read_rec<PRIM>(L.rec + im * rec_floats<PRIM>())).w;
    d = best;
  } else if (searched) {  // nothing compared below +inf: NaN where the query is NaN itself, else +inf
    const bool qnan = dir == 0 ? nan3(load3(L.points, g)) : nan_rec<PRIM>(read_rec<PRIM>(L.rec + g * rec_floats<PRIM>()));
    d = qnan ? NAN : INFINITY;
  }
  L.dist[dir][g] = d;
  L.idx[dir][g] = arg;
  store3(L.w[dir], g, w);
}

template <int PRIM>
__global__ void __launch_bounds__(kThreads) prim_record_kernel(const float* verts, const int64_t* prims, int64_t V,
                                                               int64_t M, float* rec) {
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads)
    write_rec<PRIM>(rec + m * rec_floats<PRIM>(), make_rec<PRIM>(verts, prims, m, V));
}

// grid (query blocks, splits, 2 N): blockIdx.z = 2 n + direction
template <int PRIM>
__global__ void __launch_bounds__(kThreads) pointmesh_fwd_kernel(FwdLaunch L) {
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats];
  constexpr int RF = rec_floats<PRIM>(), kPrimTile = kTileFloats / RF;
  const int dir = blockIdx.z & 1, s = blockIdx.y;
  const int64_t n = blockIdx.z >> 1;
  const Side& Q = L.side[dir];
  const Side& D = L.side[1 - dir];
  const int64_t q0 = (int64_t)blockIdx.x * kThreads;
  if (q0 >= Q.cap || s >= L.splits[dir]) return;  // uniform over the workgroup
  int64_t qfirst, qcount, dfirst, dcount;
  segment_of(Q, n, qfirst, qcount);
  segment_of(D, n, dfirst, dcount);
  const bool fill = dir == 0 && L.pad_fill;
  if (q0 >= qcount && !fill) return;  // uniform
  const int64_t lo = std::min<int64_t>((int64_t)s * L.chunk[dir], dcount);
  const int64_t hi = q0 >= qcount ? lo : std::min<int64_t>(lo + L.chunk[dir], dcount);  // padding rows search nothing
  const int64_t i = q0 + threadIdx.x, g = qfirst + i;
  const bool live = i < qcount;
  float best = INFINITY;
  int32_t arg = -1;
  if (dir == 0) {  // a point against its mesh's records
    const F3 p = live ? load3(L.points, g) : F3{0.f, 0.f, 0.f};
    for (int64_t t0 = lo; t0 < hi; t0 += kPrimTile) {
      const int cnt = (int)std::min<int64_t>(kPrimTile, hi - t0);
      const float* src = L.rec + (dfirst + t0) * RF;
      __syncthreads();  // the previous tile has been read
      for (int k = threadIdx.x; k < cnt * RF; k += kThreads) tile[k] = src[k];
      __syncthreads();
      const int32_t j0 = (int32_t)(dfirst + t0);
      for (int k = 0; k < cnt; ++k) {
        const float d = eval<PRIM>(p, read_rec<PRIM>(tile + k * RF)).d;
        if (d < best) {
          best = d;
          arg = j0 + k;
        }
      }
    }
  } else {  // a primitive against its cloud's points
    Rec r = read_rec<PRIM>(L.rec + (live ? g : 0) * RF);  // M > 0: record 0 exists
    for (int64_t t0 = lo; t0 < hi; t0 += kPointTile) {
      const int cnt = (int)std::min<int64_t>(kPointTile, hi - t0);
      const float* src = L.points + (dfirst + t0) * 3;
      __syncthreads();
      for (int k = threadIdx.x; k < cnt * 3; k += kThreads) tile[k] = src[k];
      __syncthreads();
      const int32_t j0 = (int32_t)(dfirst + t0);
      for (int k = 0; k < cnt; ++k) {
        const float d = eval<PRIM>(F3{tile[k * 3], tile[k * 3 + 1], tile[k * 3 + 2]}, r).d;
        if (d < best) {
          best = d;
          arg = j0 + k;
        }
      }
    }
  }
  if (!live) {
    // a padded batch: the rows between the cloud's count and the padded length
    if (!fill || i >= Q.cap || g >= Q.total) return;
    arg = -1;
  }
  if (L.splits[dir] > 1) {
    L.part[dir][(int64_t)s * Q.total + g] = Partial{best, arg};
  } else {
    finish<PRIM>(L, dir, g, best, arg, live && dcount > 0);
  }
}

// grid (query blocks, 1, 2 N): the partials of a query in range order, the lowest index on a tie
template <int PRIM>
__global__ void __launch_bounds__(kThreads) pointmesh_merge_kernel(FwdLaunch L) {
  const int dir = blockIdx.z & 1;
  const int64_t n = blockIdx.z >> 1, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const Side& Q = L.side[dir];
  if (L.splits[dir] <= 1 || i >= Q.cap) return;
  int64_t qfirst, qcount, dfirst, dcount;
  segment_of(Q, n, qfirst, qcount);
  segment_of(L.side[1 - dir], n, dfirst, dcount);
  const int64_t g = qfirst + i;
  const bool live = i < qcount;
  if (!live && !(dir == 0 && L.pad_fill && g < Q.total)) return;
  float best = INFINITY;
  int32_t arg = -1;
  for (int s = 0; s < L.splits[dir]; ++s) {
    const Partial p = L.part[dir][(int64_t)s * Q.total + g];
    if (p.idx >= 0 && p.d < best) {
      best = p.d;
      arg = p.idx;
    }
  }
  finish<PRIM>(L, dir, g, best, live ? arg : -1, live && dcount > 0);
}

// one wave per primitive: corner_grad (M, K, 3) = d loss / d the primitive's corners
template <int PRIM>
__global__ void __launch_bounds__(kThreads) prim_bwd_kernel(PRPointMeshArgs a, float* corner_grad) {
  constexpr int K = PRIM == 0 ? 3 : 2;
  const int lane = threadIdx.x & 63;
  for (int64_t m = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); m < a.M; m += (int64_t)gridDim.x * kWaves) {
    const Rec rec = make_rec<PRIM>(a.verts, a.prims, m, a.V);
    const int64_t b = std::max<int64_t>(a.prim_point_start[m], 0), e = std::min<int64_t>(a.prim_point_start[m + 1], a.P);
    F3 g0{0.f, 0.f, 0.f}, g1 = g0, g2 = g0;
    if (e > b) {  // uniform over the wave
      for (int64_t j = b + lane; j < e; j += 64) {
        const int64_t i = a.prim_points[j];
        if (i < 0 || i >= a.P) continue;
        const F3 r = scale3(eval<PRIM>(load3(a.points, i), rec).r, -2.f * a.grad_dist_p[i]), w = load3(a.w_p, i);
        acc3(g0, scale3(r, w.x));
        acc3(g1, scale3(r, w.y));
        acc3(g2, scale3(r, w.z));
      }
      g0 = wave_sum3(g0), g1 = wave_sum3(g1), g2 = wave_sum3(g2);
    }
    const int64_t j = a.idx_m[m];  // the primitive's own nearest point
    if (j >= 0 && j < a.P) {
      const F3 r = scale3(eval<PRIM>(load3(a.points, j), rec).r, -2.f * a.grad_dist_m[m]), w = load3(a.w_m, m);
      acc3(g0, scale3(r, w.x));
      acc3(g1, scale3(r, w.y));
      acc3(g2, scale3(r, w.z));
    }
    if (lane == 0) {
      store3(corner_grad, m * K, g0);
      store3(corner_grad, m * K + 1, g1);
      if (PRIM == 0) store3(corner_grad, m * K + 2, g2);
    }
  }
}

template <int PRIM>
__global__ void __launch_bounds__(kThreads) point_bwd_kernel(PRPointMeshArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.P; i += (int64_t)gridDim.x * kThreads) {
    const F3 p = load3(a.points, i);
    F3 g{0.f, 0.f, 0.f};
    const int64_t j = a.idx_p[i];
    if (j >= 0 && j < a.M) g = scale3(eval<PRIM>(p, make_rec<PRIM>(a.verts, a.prims, j, a.V)).r, 2.f * a.grad_dist_p[i]);
    const int64_t b = std::max<int64_t>(a.point_prim_start[i], 0), e = std::min<int64_t>(a.point_prim_start[i + 1], a.M);
    for (int64_t k = b; k < e; ++k) {
      const int64_t m = a.point_prims[k];
      if (m < 0 || m >= a.M) continue;
      acc3(g, scale3(eval<PRIM>(p, make_rec<PRIM>(a.verts, a.prims, m, a.V)).r, 2.f * a.grad_dist_m[m]));
    }
    store3(a.grad_points, i, g);
  }
}

__global__ void __launch_bounds__(kThreads) vert_gather_kernel(PRPointMeshArgs a, const float* corner_grad, int64_t corners) {
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    F3 s{0.f, 0.f, 0.f};
    const int64_t b = std::max<int64_t>(a.vert_corner_start[v], 0), e = std::min<int64_t>(a.vert_corner_start[v + 1], corners);
    for (int64_t j = b; j < e; ++j) {
      const int64_t t = a.vert_corners[j];
      if (t >= 0 && t < corners) acc3(s, load3(corner_grad, t));
    }
    store3(a.grad_verts, v, s);
  }
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }
int grid_of(int64_t n, int64_t per, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap)); }

// ranges of the other side (at most ndb entries per batch element, `tile` per LDS tile) for nq
// queries per element; PR_POINTMESH_SPLITS overrides (read per call)
int pick_splits(int64_t N, int64_t nq, int64_t ndb, int64_t tile) {
  if (const char* e = getenv("PR_POINTMESH_SPLITS")) {
    const int s = atoi(e);
    if (s > 0) return std::min(s, kMaxSplits);
  }
  const int64_t wgs = N * blocks_of(nq), tiles = (ndb + tile - 1) / tile;
  const int64_t want = (kTargetBlocks + wgs - 1) / wgs;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, tiles), kMaxSplits));
}

int rec_floats_of(int prim) { return prim == 0 ? 16 : 8; }
int corners_of(int prim) { return prim == 0 ? 3 : 2; }

struct Layout {  // of the workspace; the forward's records and partials, the backward's corner gradients
  int s_p, s_m;
  size_t rec, part_p, part_m, corner;
  size_t bytes() const { return std::max(rec + part_p + part_m, corner); }
};

Layout layout_of(int prim, int64_t N, int64_t P, int64_t M, int64_t max_points, int64_t max_prims) {
  Layout l;
  l.s_p = pick_splits(N, max_points, max_prims, kTileFloats / rec_floats_of(prim));
  l.s_m = pick_splits(N, max_prims, max_points, kPointTile);
  l.rec = (size_t)M * rec_floats_of(prim) * sizeof(float);
  l.part_p = l.s_p > 1 ? (size_t)l.s_p * (size_t)P * sizeof(Partial) : 0;
  l.part_m = l.s_m > 1 ? (size_t)l.s_m * (size_t)M * sizeof(Partial) : 0;
  l.corner = (size_t)M * corners_of(prim) * 3 * sizeof(float);
  return l;
}

bool sizes_ok(int prim, int64_t N, int64_t P, int64_t V, int64_t M, int64_t max_points, int64_t max_prims) {
  return (prim == 0 || prim == 1) && N > 0 && N <= 32767 && P > 0 && V > 0 && M > 0 && P <= INT32_MAX &&
         M <= INT32_MAX / 16 && V <= INT32_MAX && max_points > 0 && max_points <= P && max_prims > 0 && max_prims <= M;
}

// host-side validation, before any launch
int pointmesh_check(const PRPointMeshArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (a->prim != 0 && a->prim != 1) return set_error(PR_ERR_ARG, w + ": prim must be 0 (faces) or 1 (edges), got " + std::to_string(a->prim));
  if (a->N <= 0 || a->P <= 0 || a->V <= 0 || a->M <= 0 || a->max_points <= 0 || a->max_prims <= 0)
    return set_error(PR_ERR_ARG, w + ": N, P, V, M, max_points and max_prims must be positive");
  if (a->N > 32767) return set_error(PR_ERR_ARG, w + ": N must fit the grid (32767)");
  if (a->P > INT32_MAX || a->V > INT32_MAX || a->M > INT32_MAX / 16)
    return set_error(PR_ERR_ARG, w + ": P, V and 16 M must fit int32");
  if (a->max_points > a->P || a->max_prims > a->M)
    return set_error(PR_ERR_ARG, w + ": max_points / max_prims exceed P / M");
  if (!a->cloud_first && a->N * a->max_points != a->P)
    return set_error(PR_ERR_ARG, w + ": a padded batch (cloud_first NULL) needs P = N max_points");
  if (!a->points || !a->verts || !a->prims) return set_error(PR_ERR_ARG, w + ": points / verts / prims missing");
  if (fwd && (!a->mesh_first || !a->mesh_count)) return set_error(PR_ERR_ARG, w + ": mesh_first / mesh_count missing");
  if (!a->idx_p || !a->idx_m || !a->w_p || !a->w_m) return set_error(PR_ERR_ARG, w + ": idx_p / idx_m / w_p / w_m missing");
  if (fwd && (!a->dist_p || !a->dist_m)) return set_error(PR_ERR_ARG, w + ": dist_p / dist_m missing");
  if (!fwd && (!a->prim_point_start || !a->prim_points || !a->point_prim_start || !a->point_prims))
    return set_error(PR_ERR_ARG, w + ": primitive -> points / point -> primitives CSR missing");
  if (!fwd && (!a->vert_corner_start || !a->vert_corners)) return set_error(PR_ERR_ARG, w + ": corner CSR missing");
  if (!fwd && (!a->grad_dist_p || !a->grad_dist_m || !a->grad_points || !a->grad_verts))
    return set_error(PR_ERR_ARG, w + ": grads missing");
  const size_t need = layout_of(a->prim, a->N, a->P, a->M, a->max_points, a->max_prims).bytes();
  if (!a->workspace || a->workspace_bytes < need)
    return set_error(PR_ERR_ARG, w + ": workspace missing or smaller than pr_point_mesh_workspace (" + std::to_string(need) + " bytes)");
  return PR_OK;
}

template <int PRIM>
int fwd_launch(const PRPointMeshArgs& a, hipStream_t st) {
  const Layout l = layout_of(PRIM, a.N, a.P, a.M, a.max_points, a.max_prims);
  char* ws = static_cast<char*>(a.workspace);
  float* rec = reinterpret_cast<float*>(ws);
  prim_record_kernel<PRIM><<<grid_of(a.M, kThreads, 4096), kThreads, 0, st>>>(a.verts, a.prims, a.V, a.M, rec);
  if (int e = check_launch("point_mesh_records")) return e;
  FwdLaunch L;
  L.points = a.points, L.rec = rec;
  L.side[0] = Side{a.cloud_first, a.cloud_count, a.P, a.max_points};
  L.side[1] = Side{a.mesh_first, a.mesh_count, a.M, a.max_prims};
  L.splits[0] = l.s_p, L.splits[1] = l.s_m;
  L.chunk[0] = (a.max_prims + l.s_p - 1) / l.s_p, L.chunk[1] = (a.max_points + l.s_m - 1) / l.s_m;
  L.dist[0] = a.dist_p, L.dist[1] = a.dist_m, L.idx[0] = a.idx_p, L.idx[1] = a.idx_m, L.w[0] = a.w_p, L.w[1] = a.w_m;
  L.part[0] = reinterpret_cast<Partial*>(ws + l.rec), L.part[1] = reinterpret_cast<Partial*>(ws + l.rec + l.part_p);
  L.pad_fill = a.cloud_first ? 0 : 1;
  const unsigned qb = (unsigned)blocks_of(std::max(a.max_points, a.max_prims));
  pointmesh_fwd_kernel<PRIM><<<dim3(qb, (unsigned)std::max(l.s_p, l.s_m), (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
  if (int e = check_launch("point_mesh_fwd")) return e;
  if (l.s_p > 1 || l.s_m > 1) {
    pointmesh_merge_kernel<PRIM><<<dim3(qb, 1, (unsigned)(2 * a.N)), kThreads, 0, st>>>(L);
    return check_launch("point_mesh_merge");
  }
  return PR_OK;
}

template <int PRIM>
int bwd_launch(const PRPointMeshArgs& a, hipStream_t st) {
  float* corner_grad = static_cast<float*>(a.workspace);
  prim_bwd_kernel<PRIM><<<grid_of(a.M, kWaves, 16384), kThreads, 0, st>>>(a, corner_grad);
  if (int e = check_launch("point_mesh_prim_bwd")) return e;
  point_bwd_kernel<PRIM><<<grid_of(a.P, kThreads, 4096), kThreads, 0, st>>>(a);
  if (int e = check_launch("point_mesh_point_bwd")) return e;
  vert_gather_kernel<<<grid_of(a.V, kThreads, 4096), kThreads, 0, st>>>(a, corner_grad, a.M * (PRIM == 0 ? 3 : 2));
  return check_launch("point_mesh_bwd");
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_point_mesh_workspace(int32_t prim, int64_t N, int64_t P, int64_t M, int64_t max_points,
                                          int64_t max_prims) {
  if (!sizes_ok(prim, N, P, 1, M, max_points, max_prims)) return 0;
  return layout_of(prim, N, P, M, max_points, max_prims).bytes();
}

extern "C" int pr_point_mesh_fwd(const PRPointMeshArgs* args, void* stream) {
  if (int e = pointmesh_check(args, "point_mesh_fwd", true)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return args->prim == 0 ? fwd_launch<0>(*args, st) : fwd_launch<1>(*args, st);
}

extern "C" int pr_point_mesh_bwd(const PRPointMeshArgs* args, void* stream) {
  if (int e = pointmesh_check(args, "point_mesh_bwd", false)) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return args->prim == 0 ? bwd_launch<0>(*args, st) : bwd_launch<1>(*args, st);
}
