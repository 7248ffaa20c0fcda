// Area-weighted surface sampling of a packed mesh batch (PyTorch3D 0.4.0 sample_points_from_meshes:
// the operator that feeds chamfer_distance in the deformation loop), forward and backward.
//
// Forward, three launches.  (1) One lane per face writes the float32 area.  (2) One workgroup per
// mesh scans its areas into the inclusive prefix table `cdf`: kScanChunk faces per pass (kScanPer
// consecutive faces per lane, a wave scan on shuffles, the waves in order through LDS), a float64
// carry between passes, every entry rounded to float32 once; the next pass's areas are loaded
// before the current pass is scanned.  The meshes' first / count tables are read on the device, so
// meshes of any lengths share the launch and nothing is read back.  (3) One lane per (mesh, sample):
// a Philox4x32 block (or the injected uniforms), a binary search of the mesh's segment of `cdf` for
// the first entry above r = u0 total (none: the first entry >= total, so u0 = 1 lands on the last
// face with area), the point and the optional face normal.  Two equal neighbouring entries are the
// mark of a zero-area face; both searches stop at the first of them, so such a face is never picked.
//
// Backward, two launches over the forward's (face_idx, w), whatever the noise mode was.  The caller
// passes the face -> samples CSR of this call (a stable sort of face_idx).  One wave per face walks
// the face's segment with fixed lane striding (lane l takes entries l, l + 64, ... in ascending
// order) and folds the 64 partial sums with a fixed xor tree: the (3,3) corner gradient
// sum_s w_c(s) g(s) and sum_s g_normal(s), the latter pushed through the normalisation and the cross
// product.  A face that holds most of a mesh's samples is still spread over 64 lanes.  Then one
// lane per vertex gathers its corners over the corner CSR, as the other losses' backwards do.  No
// atomics, every sum in a fixed order: the same bits on every call.
#include <math.h>

#include <algorithm>

#include "pr_common.h"

namespace pr {
namespace {

constexpr uint32_t kTagSamp = 0x53414D50u;  // "SAMP"
constexpr float kNormalEps = 2.220446049250313e-16f;
constexpr int kWaves = kThreads / 64;
constexpr int kScanPer = 4;                       // consecutive faces per lane and pass
constexpr int kScanChunk = kThreads * kScanPer;   // faces per pass of a mesh's workgroup
constexpr int64_t kMaxMeshes = 65535;             // gridDim.y of the sample pass

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
PR_DEV float norm3(F3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }

// the wave's sum in every lane: a fixed xor tree over the 64 lanes
PR_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
PR_DEV F3 wave_sum3(F3 v) { return F3{wave_sum(v.x), wave_sum(v.y), wave_sum(v.z)}; }

// mesh n's segment [first, first + count) of the packed face list, clamped to it
PR_DEV void mesh_segment(const PRSamplePointsArgs& a, int64_t n, int64_t& first, int64_t& count) {
  first = std::min<int64_t>(std::max<int64_t>(a.mesh_first_face[n], 0), a.F);
  count = std::min<int64_t>(std::max<int64_t>(a.mesh_num_faces[n], 0), a.F - first);
}

__global__ void __launch_bounds__(kThreads) face_area_kernel(PRSamplePointsArgs a, float* area) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kThreads) {
    const F3 v0 = load3(a.verts, a.faces[f * 3]), v1 = load3(a.verts, a.faces[f * 3 + 1]),
             v2 = load3(a.verts, a.faces[f * 3 + 2]);
    area[f] = 0.5f * norm3(cross3(sub(v1, v0), sub(v2, v0)));
  }
}

// grid (N): the workgroup of mesh n
__global__ void __launch_bounds__(kThreads) cdf_scan_kernel(PRSamplePointsArgs a, const float* area) {
  __shared__ double wave_sum[kWaves];
  int64_t first, nf;
  mesh_segment(a, blockIdx.x, first, nf);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* src = area + first;
  float* dst = a.cdf + first;
  float nxt[kScanPer];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int64_t i = (int64_t)threadIdx.x * kScanPer + k;
    nxt[k] = i < nf ? src[i] : 0.f;
  }
  double carry = 0.0;
  for (int64_t c0 = 0; c0 < nf; c0 += kScanChunk) {  // uniform over the workgroup
    const int64_t i0 = c0 + (int64_t)threadIdx.x * kScanPer;
    double x[kScanPer], s = 0.0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      s += (double)nxt[k];
      x[k] = s;
      const int64_t i = i0 + kScanChunk + k;  // the next pass's areas, in flight during this scan
      nxt[k] = i < nf ? src[i] : 0.f;
    }
    double inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    double base = carry, total = carry;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) base += wave_sum[w];
      total += wave_sum[w];
    }
    const double excl = base + (inc - s);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k)
      if (i0 + k < nf) dst[i0 + k] = (float)(excl + x[k]);
    carry = total;
    __syncthreads();  // wave_sum is written again in the next pass
  }
}

// grid (sample blocks, N): one lane per (n, s)
__global__ void __launch_bounds__(kThreads) sample_kernel(PRSamplePointsArgs a) {
  const int64_t n = blockIdx.y, s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= a.S) return;
  const int64_t i = n * a.S + s;
  float u0, u1, u2;
  if (a.noise_mode == PR_NOISE_INJECTED) {
    u0 = a.uniforms[i * 3], u1 = a.uniforms[i * 3 + 1], u2 = a.uniforms[i * 3 + 2];
  } else {
    uint64_t key = a.seed;  // bit 63 marks an absolute key that ignores the device base, as in the blend
    if (a.seeds && !(key >> 63)) key = mix64(a.seeds[0] ^ key);
    const U4 b = philox_block(key, (uint32_t)s, (uint32_t)n, 0u, kTagSamp);
    u0 = u01(b.x), u1 = u01(b.y), u2 = u01(b.z);
  }
  int64_t first, nf;
  mesh_segment(a, n, first, nf);
  int32_t face = -1;
  F3 w{0.f, 0.f, 0.f}, p{0.f, 0.f, 0.f}, nrm{0.f, 0.f, 0.f};
  const float total = nf > 0 ? a.cdf[first + nf - 1] : 0.f;
  if (total > 0.f) {  // false for a NaN total as well: a dead row
    const float* cdf = a.cdf + first;
    const float r = u0 * total;
    int64_t lo = 0, hi = nf;
    while (lo < hi) {  // the first entry above r
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] > r) hi = mid; else lo = mid + 1;
    }
    if (lo == nf) {  // none: the first entry that reaches the total (the last one does)
      lo = 0, hi = nf - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
      }
    }
    const int64_t f = first + lo;
    face = (int32_t)f;
    const float su = sqrtf(u1);
    w = F3{1.f - su, su * (1.f - u2), su * u2};
    const F3 v0 = load3(a.verts, a.faces[f * 3]), v1 = load3(a.verts, a.faces[f * 3 + 1]),
             v2 = load3(a.verts, a.faces[f * 3 + 2]);
    p = add(add(scale3(v0, w.x), scale3(v1, w.y)), scale3(v2, w.z));
    if (a.normals) {
      const F3 c = cross3(sub(v1, v0), sub(v2, v1));
      const float den = fmaxf(norm3(c), kNormalEps);
      nrm = F3{c.x / den, c.y / den, c.z / den};
    }
  }
  store3(a.samples, i, p);
  if (a.normals) store3(a.normals, i, nrm);
  store3(a.w, i, w);
  a.face_idx[i] = face;
}

// one wave per face: face_grad (F,3,3) = d loss / d the face's corners
__global__ void __launch_bounds__(kThreads) face_bwd_kernel(PRSamplePointsArgs a, float* face_grad) {
  const int lane = threadIdx.x & 63;
  const int64_t total = a.N * a.S;
  for (int64_t f = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); f < a.F; f += (int64_t)gridDim.x * kWaves) {
    const int64_t b = std::max<int64_t>(a.face_sample_start[f], 0), e = std::min<int64_t>(a.face_sample_start[f + 1], total);
    F3 g0{0.f, 0.f, 0.f}, g1 = g0, g2 = g0, gn = g0;
    if (e > b) {  // uniform over the wave
      for (int64_t j = b + lane; j < e; j += 64) {
        const int64_t i = a.face_samples[j];
        if (i < 0 || i >= total) continue;
        const F3 g = load3(a.grad_samples, i), w = load3(a.w, i);
        acc3(g0, scale3(g, w.x));
        acc3(g1, scale3(g, w.y));
        acc3(g2, scale3(g, w.z));
        if (a.grad_normals) acc3(gn, load3(a.grad_normals, i));
      }
      g0 = wave_sum3(g0), g1 = wave_sum3(g1), g2 = wave_sum3(g2);
      if (a.grad_normals) {
        gn = wave_sum3(gn);
        const F3 v0 = load3(a.verts, a.faces[f * 3]), v1 = load3(a.verts, a.faces[f * 3 + 1]),
                 v2 = load3(a.verts, a.faces[f * 3 + 2]);
        const F3 e1 = sub(v1, v0), e2 = sub(v2, v1), c = cross3(e1, e2);
        const float len = norm3(c);
        F3 gc;
        if (len >= kNormalEps) {  // (g_n - n (n . g_n)) / |c|
          const F3 nrm{c.x / len, c.y / len, c.z / len};
          gc = scale3(sub(gn, scale3(nrm, dot3(nrm, gn))), 1.f / len);
        } else {  // clamped: torch's clamp passes nothing to |c|
          gc = scale3(gn, 1.f / kNormalEps);
        }
        // c = e1 x e2: d / d e1 = e2 x g_c, d / d e2 = g_c x e1; e1 = v1 - v0, e2 = v2 - v1
        const F3 d1 = cross3(e2, gc), d2 = cross3(gc, e1);
        g0 = sub(g0, d1);
        g1 = add(g1, sub(d1, d2));
        acc3(g2, d2);
      }
    }
    if (lane == 0) {
      store3(face_grad, f * 3, g0);
      store3(face_grad, f * 3 + 1, g1);
      store3(face_grad, f * 3 + 2, g2);
    }
  }
}

__global__ void __launch_bounds__(kThreads) vert_bwd_kernel(PRSamplePointsArgs a, const float* face_grad) {
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    F3 s{0.f, 0.f, 0.f};
    for (int64_t j = a.vert_corner_start[v]; j < a.vert_corner_start[v + 1]; ++j) {
      const int64_t t = a.vert_corners[j];
      if (t >= 0 && t < 3 * a.F) acc3(s, load3(face_grad, t));
    }
    store3(a.grad_verts, v, s);
  }
}

size_t workspace_bytes(int64_t F) { return (size_t)F * 9 * sizeof(float); }  // bwd: (F,3,3); fwd: (F) areas

int blocks_of(int64_t n, int64_t per, int64_t cap) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap));
}

// host-side validation, before any launch
int sample_check(const PRSamplePointsArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (a->N <= 0 || a->S <= 0 || a->V <= 0 || a->F <= 0)
    return set_error(PR_ERR_ARG, w + ": N, S, V and F must be positive");
  if (a->N > kMaxMeshes) return set_error(PR_ERR_ARG, w + ": N must fit the grid (65535)");
  if (a->S > INT32_MAX / a->N || a->F > INT32_MAX / 3)
    return set_error(PR_ERR_ARG, w + ": N S and 3 F must fit int32");
  if (!a->verts || !a->faces) return set_error(PR_ERR_ARG, w + ": verts / faces missing");
  if (fwd && (!a->mesh_first_face || !a->mesh_num_faces))
    return set_error(PR_ERR_ARG, w + ": mesh_first_face / mesh_num_faces missing");
  if (fwd && a->noise_mode != PR_NOISE_PHILOX && a->noise_mode != PR_NOISE_INJECTED)
    return set_error(PR_ERR_ARG, w + ": unknown noise_mode " + std::to_string(a->noise_mode));
  if (fwd && a->noise_mode == PR_NOISE_INJECTED && !a->uniforms)
    return set_error(PR_ERR_ARG, w + ": uniforms missing (PR_NOISE_INJECTED)");
  if (fwd && (!a->cdf || !a->samples)) return set_error(PR_ERR_ARG, w + ": cdf / samples missing");
  if ((fwd && !a->face_idx) || !a->w) return set_error(PR_ERR_ARG, w + ": face_idx / w missing");
  if (!fwd && (!a->face_sample_start || !a->face_samples))
    return set_error(PR_ERR_ARG, w + ": face -> samples CSR missing");
  if (!fwd && (!a->vert_corner_start || !a->vert_corners)) return set_error(PR_ERR_ARG, w + ": corner CSR missing");
  if (!fwd && (!a->grad_samples || !a->grad_verts)) return set_error(PR_ERR_ARG, w + ": grads missing");
  if (!a->workspace || a->workspace_bytes < workspace_bytes(a->F))
    return set_error(PR_ERR_ARG, w + ": workspace missing or smaller than pr_sample_points_workspace (" +
                                     std::to_string(workspace_bytes(a->F)) + " bytes)");
  return PR_OK;
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_sample_points_workspace(int64_t F) { return F > 0 ? workspace_bytes(F) : 0; }

extern "C" int pr_sample_points_fwd(const PRSamplePointsArgs* args, void* stream) {
  if (int e = sample_check(args, "sample_points_fwd", true)) return e;
  const PRSamplePointsArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* area = static_cast<float*>(a.workspace);
  face_area_kernel<<<blocks_of(a.F, kThreads, 4096), kThreads, 0, st>>>(a, area);
  if (int e = check_launch("sample_face_area")) return e;
  cdf_scan_kernel<<<(unsigned)a.N, kThreads, 0, st>>>(a, area);
  if (int e = check_launch("sample_cdf_scan")) return e;
  sample_kernel<<<dim3((unsigned)((a.S + kThreads - 1) / kThreads), (unsigned)a.N), kThreads, 0, st>>>(a);
  return check_launch("sample_points_fwd");
}

extern "C" int pr_sample_points_bwd(const PRSamplePointsArgs* args, void* stream) {
  if (int e = sample_check(args, "sample_points_bwd", false)) return e;
  const PRSamplePointsArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* face_grad = static_cast<float*>(a.workspace);
  face_bwd_kernel<<<blocks_of(a.F, kWaves, 16384), kThreads, 0, st>>>(a, face_grad);
  if (int e = check_launch("sample_face_bwd")) return e;
  vert_bwd_kernel<<<blocks_of(a.V, kThreads, 4096), kThreads, 0, st>>>(a, face_grad);
  return check_launch("sample_points_bwd");
}
