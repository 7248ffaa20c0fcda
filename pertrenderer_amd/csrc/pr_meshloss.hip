// Mesh regularisers of the vertex-deformation task (eval.py:454-457: PyTorch3D 0.4.0
// mesh_laplacian_smoothing with its "uniform", "cot" and "cotcurv" weights, and mesh_edge_loss),
// forward and backward.  One lane per packed vertex; a vertex's row of the neighbour CSR (uniform,
// edge loss) or of the face-corner CSR (cot, cotcurv) is walked in a plain loop, so every sum is a
// gather in the row's order: no atomics, the same bits on every call.  The scalar loss is formed
// like pr_rgb_mse's: per-workgroup partial sums in a fixed order, then one workgroup sums the
// partials in block order.  A Laplacian costs 2-3 launches forward and 1 backward instead of the
// ~25 torch kernels (cat, sort, unique, index_adds, norm, ...) of the composition in loss.py.
//
// The cotangent matrix L is symmetric and a constant of the backward (PyTorch3D builds it under
// no_grad), so d loss / d v_k = g (sum_i L_ki s_i p_i - d_k p_k) with p_i = w_i l_i / |l_i| (0 where
// |l_i| = 0, torch.norm's subgradient): the forward stores s_i p_i (`gather`) and d_k p_k (`diag`)
// and the backward is the forward's gather over them.  Both gather over the corners of vertex i:
// in face (i, j, k) the corner adds cot_k x_j + cot_j x_k (the cot at a corner weighs the edge
// opposite to it), which needs no edge -> face map.
//
// mesh_normal_consistency (loss.py's definition) follows the same scheme one level up: one lane per
// face over the face-pair CSR forward (3 launches), one lane per face and then one per vertex over
// the corner CSR backward (2 launches), instead of the ~100 torch kernels of the composition.
#include "pr_common.h"

namespace pr {
namespace {

struct F3 {
  float x, y, z;
};
PR_DEV F3 load3(const float* p, int64_t i) { return F3{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]}; }
PR_DEV void store3(float* p, int64_t i, F3 v) { p[i * 3] = v.x; p[i * 3 + 1] = v.y; p[i * 3 + 2] = v.z; }
PR_DEV F3 sub(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PR_DEV F3 scale3(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
PR_DEV void acc3(F3& a, F3 b) { a.x += b.x; a.y += b.y; a.z += b.z; }
PR_DEV float norm3(F3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }

constexpr int kLossBlocks = 512;

// the workgroup's sum of `acc` (wave butterflies, then the waves in order) -> partials[block]
PR_DEV void block_partial(float acc, float* partials) {
  __shared__ float red[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    partials[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(kThreads) mesh_finalize_kernel(const float* partials, int nblk, float* loss) {
  __shared__ float red[kThreads / 64];
  float acc = 0.f;
  for (int b = threadIdx.x; b < nblk; b += kThreads) acc += partials[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    *loss = s;
  }
}

// per face: the three corner cotangents and the (clamped) Heron area
__global__ void __launch_bounds__(kThreads) face_cot_kernel(PRMeshLossArgs a) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kThreads) {
    const F3 v0 = load3(a.verts, a.faces[f * 3]), v1 = load3(a.verts, a.faces[f * 3 + 1]),
             v2 = load3(a.verts, a.faces[f * 3 + 2]);
    const float A = norm3(sub(v1, v2)), B = norm3(sub(v0, v2)), C = norm3(sub(v0, v1));
    const float s = 0.5f * (A + B + C);
    const float area = sqrtf(fmaxf(s * (s - A) * (s - B) * (s - C), 1e-12f));
    const float A2 = A * A, B2 = B * B, C2 = C * C, d = 4.f * area;
    a.face_cot[f * 4] = (B2 + C2 - A2) / d;
    a.face_cot[f * 4 + 1] = (A2 + C2 - B2) / d;
    a.face_cot[f * 4 + 2] = (A2 + B2 - C2) / d;
    a.face_cot[f * 4 + 3] = area;
  }
}

// sum over the corners of vertex v of cot_k x_j + cot_j x_k (x = a (V,3) field); r: the sum of the
// weights, area: the area sum of v's faces
PR_DEV F3 corner_gather(const PRMeshLossArgs& a, const float* x, int64_t v, float* r, float* area) {
  F3 s{0.f, 0.f, 0.f};
  float rs = 0.f, as = 0.f;
  for (int64_t j = a.vert_corner_start[v]; j < a.vert_corner_start[v + 1]; ++j) {
    const int64_t t = a.vert_corners[j], f = t / 3;
    const int c = (int)(t - f * 3), c1 = c == 2 ? 0 : c + 1, c2 = c == 0 ? 2 : c - 1;
    const float cot1 = a.face_cot[f * 4 + c1], cot2 = a.face_cot[f * 4 + c2];
    acc3(s, scale3(load3(x, a.faces[f * 3 + c1]), cot2));
    acc3(s, scale3(load3(x, a.faces[f * 3 + c2]), cot1));
    rs += cot1;
    rs += cot2;
    as += a.face_cot[f * 4 + 3];
  }
  if (r) *r = rs;
  if (area) *area = as;
  return s;
}

PR_DEV F3 nbr_gather(const PRMeshLossArgs& a, const float* x, int64_t v) {
  F3 s{0.f, 0.f, 0.f};
  for (int64_t j = a.nbr_start[v]; j < a.nbr_start[v + 1]; ++j) acc3(s, load3(x, a.nbr[j]));
  return s;
}

template <int M>
__global__ void __launch_bounds__(kThreads) lap_fwd_kernel(PRMeshLossArgs a) {
  float acc = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    const F3 vi = load3(a.verts, v);
    // sc: the weight of the neighbour sum in l_i; dsc: minus the derivative of l_i by v_i
    float sc, dsc = 1.f;
    F3 l;
    if (M == PR_MESH_LAP_UNIFORM) {
      const int64_t deg = a.nbr_start[v + 1] - a.nbr_start[v];
      sc = 1.f / (float)(deg > 1 ? deg : 1);
      l = sub(scale3(nbr_gather(a, a.verts, v), sc), vi);
    } else {
      float r, area;
      const F3 s = corner_gather(a, a.verts, v, &r, &area);
      if (M == PR_MESH_LAP_COT) {
        sc = r > 0.f ? 1.f / r : r;
        l = sub(scale3(s, sc), vi);
      } else {
        sc = 0.25f * (area > 0.f ? 1.f / area : area);
        dsc = r * sc;
        l = scale3(sub(s, scale3(vi, r)), sc);
      }
    }
    const float n = norm3(l), w = a.weight[v];
    acc += w * n;
    const F3 p = n > 0.f ? scale3(l, w / n) : F3{0.f, 0.f, 0.f};
    store3(a.gather, v, scale3(p, sc));
    store3(a.diag, v, scale3(p, dsc));
  }
  block_partial(acc, a.partials);
}

template <int M>
__global__ void __launch_bounds__(kThreads) lap_bwd_kernel(PRMeshLossArgs a) {
  const float g = *a.grad_loss;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    const F3 s = M == PR_MESH_LAP_UNIFORM ? nbr_gather(a, a.gather, v) : corner_gather(a, a.gather, v, nullptr, nullptr);
    store3(a.grad_verts, v, scale3(sub(s, load3(a.diag, v)), g));
  }
}

__global__ void __launch_bounds__(kThreads) edge_fwd_kernel(PRMeshLossArgs a) {
  float acc = 0.f;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    const F3 vi = load3(a.verts, v);
    float s = 0.f;
    for (int64_t j = a.nbr_start[v]; j < a.nbr_start[v + 1]; ++j) {
      const int64_t n = a.nbr[j];
      if (n <= v) continue;  // every unique edge once, at its lower vertex
      const float d = norm3(sub(vi, load3(a.verts, n))) - a.target_length;
      s += d * d;
    }
    acc += a.weight[v] * s;
  }
  block_partial(acc, a.partials);
}

__global__ void __launch_bounds__(kThreads) edge_bwd_kernel(PRMeshLossArgs a) {
  const float g = *a.grad_loss;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    const F3 vi = load3(a.verts, v);
    F3 s{0.f, 0.f, 0.f};
    for (int64_t j = a.nbr_start[v]; j < a.nbr_start[v + 1]; ++j) {
      const F3 d = sub(vi, load3(a.verts, a.nbr[j]));
      const float len = norm3(d);
      if (len > 0.f) acc3(s, scale3(d, 2.f * (len - a.target_length) / len));
    }
    store3(a.grad_verts, v, scale3(s, g * a.weight[v]));
  }
}

// ---- normal consistency: loss = (1/P) sum over the face pairs (a, b) of 1 - n_a . n_b with
// n_f = c_f / max(|c_f|, eps), c_f = (v1 - v0) x (v2 - v0) (loss.py's composition, not PyTorch3D's
// per-edge formula).  Every pair stands in the CSR rows of both of its faces, so a face's row sum
// s_f = sum of its partners' normals is d (sum of cosines) / d n_f, and half the row sums of
// 1 - n_f . n_p add up to the pair sum.
constexpr float kNormalEps = 1e-6f;

PR_DEV F3 cross3(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PR_DEV float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PR_DEV F3 load3of4(const float* p, int64_t i) { return F3{p[i * 4], p[i * 4 + 1], p[i * 4 + 2]}; }

// per face: n_f and 1 / max(|c_f|, eps), the latter negated where the clamp is active
__global__ void __launch_bounds__(kThreads) face_normal_kernel(PRNormalConsistencyArgs a) {
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kThreads) {
    const F3 v0 = load3(a.verts, a.faces[f * 3]), v1 = load3(a.verts, a.faces[f * 3 + 1]),
             v2 = load3(a.verts, a.faces[f * 3 + 2]);
    const F3 c = cross3(sub(v1, v0), sub(v2, v0));
    const float len = norm3(c), den = fmaxf(len, kNormalEps);
    a.face_normal[f * 4] = c.x / den;
    a.face_normal[f * 4 + 1] = c.y / den;
    a.face_normal[f * 4 + 2] = c.z / den;
    a.face_normal[f * 4 + 3] = len >= kNormalEps ? 1.f / den : -1.f / den;
  }
}

__global__ void __launch_bounds__(kThreads) normal_pairs_kernel(PRNormalConsistencyArgs a) {
  float acc = 0.f;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kThreads) {
    const F3 n = load3of4(a.face_normal, f);
    F3 s{0.f, 0.f, 0.f};
    float t = 0.f;
    for (int64_t j = a.pair_start[f]; j < a.pair_start[f + 1]; ++j) {
      const F3 p = load3of4(a.face_normal, a.pair_partner[j]);
      acc3(s, p);
      t += 1.f - dot3(n, p);  // the 1 - cos terms, not the cosines: they do not cancel on a smooth mesh
    }
    store3(a.face_sum, f, s);
    acc += t;
  }
  block_partial(acc * (0.5f / (float)a.P), a.partials);
}

// per face: d loss / d c_f from d loss / d n_f = -(g / P) s_f, through the normalisation
__global__ void __launch_bounds__(kThreads) normal_face_bwd_kernel(PRNormalConsistencyArgs a) {
  const float g = -*a.grad_loss / (float)a.P;
  for (int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * kThreads) {
    const F3 n = load3of4(a.face_normal, f), gn = scale3(load3(a.face_sum, f), g);
    const float inv = a.face_normal[f * 4 + 3];
    // |c| >= eps: (g_n - n (n . g_n)) / |c|; clamped: g_n / eps (torch's clamp_min passes nothing to |c|)
    const F3 gc = inv > 0.f ? scale3(sub(gn, scale3(n, dot3(n, gn))), inv) : scale3(gn, -inv);
    store3(a.face_grad, f, gc);
  }
}

// per vertex over its face corners: c = e1 x e2, e1 = v1 - v0, e2 = v2 - v0, so d/d v1 = e2 x g_c,
// d/d v2 = g_c x e1 and d/d v0 = minus both
__global__ void __launch_bounds__(kThreads) normal_vert_bwd_kernel(PRNormalConsistencyArgs a) {
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * kThreads) {
    F3 s{0.f, 0.f, 0.f};
    for (int64_t j = a.vert_corner_start[v]; j < a.vert_corner_start[v + 1]; ++j) {
      const int64_t t = a.vert_corners[j], f = t / 3;
      const int c = (int)(t - f * 3);
      const F3 v0 = load3(a.verts, a.faces[f * 3]), gc = load3(a.face_grad, f);
      const F3 d1 = cross3(sub(load3(a.verts, a.faces[f * 3 + 2]), v0), gc);
      const F3 d2 = cross3(gc, sub(load3(a.verts, a.faces[f * 3 + 1]), v0));
      acc3(s, c == 1 ? d1 : (c == 2 ? d2 : F3{-d1.x - d2.x, -d1.y - d2.y, -d1.z - d2.z}));
    }
    store3(a.grad_verts, v, s);
  }
}

int loss_blocks(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, kLossBlocks));
}

// host-side validation, before any launch
int mesh_check(const PRMeshLossArgs* a, const char* what, bool laplacian, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (a->V <= 0 || a->F < 0) return set_error(PR_ERR_ARG, w + ": V must be positive and F non-negative");
  if (laplacian && a->method != PR_MESH_LAP_UNIFORM && a->method != PR_MESH_LAP_COT &&
      a->method != PR_MESH_LAP_COTCURV)
    return set_error(PR_ERR_ARG, w + ": unknown method " + std::to_string(a->method));
  const bool csr_nbr = !laplacian || a->method == PR_MESH_LAP_UNIFORM;
  // the Laplacian's backward reads the forward's gather / diag only
  if ((fwd || !laplacian) && (!a->verts || !a->weight)) return set_error(PR_ERR_ARG, w + ": verts / weight missing");
  if (csr_nbr && (!a->nbr_start || !a->nbr)) return set_error(PR_ERR_ARG, w + ": neighbour CSR missing");
  if (!csr_nbr && (!a->faces || !a->vert_corner_start || !a->vert_corners || !a->face_cot))
    return set_error(PR_ERR_ARG, w + ": faces / corner CSR / face_cot missing");
  if (laplacian && (!a->gather || !a->diag)) return set_error(PR_ERR_ARG, w + ": gather / diag missing");
  if (fwd && (!a->partials || !a->loss)) return set_error(PR_ERR_ARG, w + ": loss / workspace missing");
  if (!fwd && (!a->grad_loss || !a->grad_verts)) return set_error(PR_ERR_ARG, w + ": grads missing");
  return PR_OK;
}

int normal_check(const PRNormalConsistencyArgs* a, const char* what, bool fwd) {
  const std::string w(what);
  if (!a) return set_error(PR_ERR_ARG, w + ": null args");
  if (a->V <= 0 || a->F <= 0 || a->P <= 0) return set_error(PR_ERR_ARG, w + ": V, F and P must be positive");
  if (!a->verts || !a->faces) return set_error(PR_ERR_ARG, w + ": verts / faces missing");
  if (!a->face_normal || !a->face_sum) return set_error(PR_ERR_ARG, w + ": face_normal / face_sum missing");
  if (fwd && (!a->pair_start || !a->pair_partner)) return set_error(PR_ERR_ARG, w + ": face-pair CSR missing");
  if (fwd && (!a->partials || !a->loss)) return set_error(PR_ERR_ARG, w + ": loss / workspace missing");
  if (!fwd && (!a->vert_corner_start || !a->vert_corners)) return set_error(PR_ERR_ARG, w + ": corner CSR missing");
  if (!fwd && (!a->grad_loss || !a->face_grad || !a->grad_verts)) return set_error(PR_ERR_ARG, w + ": grads missing");
  return PR_OK;
}

}  // namespace
}  // namespace pr

using namespace pr;

extern "C" size_t pr_mesh_loss_workspace(int64_t V) { return V > 0 ? (size_t)loss_blocks(V) : 1; }

extern "C" int pr_mesh_laplacian_fwd(const PRMeshLossArgs* args, void* stream) {
  if (int e = mesh_check(args, "mesh_laplacian_fwd", true, true)) return e;
  const PRMeshLossArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nb = loss_blocks(a.V);
  if (a.method != PR_MESH_LAP_UNIFORM && a.F > 0) {
    face_cot_kernel<<<loss_blocks(a.F), kThreads, 0, st>>>(a);
    if (int e = check_launch("mesh_face_cot")) return e;
  }
  if (a.method == PR_MESH_LAP_UNIFORM)
    lap_fwd_kernel<PR_MESH_LAP_UNIFORM><<<nb, kThreads, 0, st>>>(a);
  else if (a.method == PR_MESH_LAP_COT)
    lap_fwd_kernel<PR_MESH_LAP_COT><<<nb, kThreads, 0, st>>>(a);
  else
    lap_fwd_kernel<PR_MESH_LAP_COTCURV><<<nb, kThreads, 0, st>>>(a);
  if (int e = check_launch("mesh_laplacian_fwd")) return e;
  mesh_finalize_kernel<<<1, kThreads, 0, st>>>(a.partials, nb, a.loss);
  return check_launch("mesh_finalize");
}

extern "C" int pr_mesh_laplacian_bwd(const PRMeshLossArgs* args, void* stream) {
  if (int e = mesh_check(args, "mesh_laplacian_bwd", true, false)) return e;
  const PRMeshLossArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nb = (int)std::min<int64_t>((a.V + kThreads - 1) / kThreads, 4096);
  if (a.method == PR_MESH_LAP_UNIFORM)
    lap_bwd_kernel<PR_MESH_LAP_UNIFORM><<<nb, kThreads, 0, st>>>(a);
  else
    lap_bwd_kernel<PR_MESH_LAP_COT><<<nb, kThreads, 0, st>>>(a);
  return check_launch("mesh_laplacian_bwd");
}

extern "C" int pr_mesh_edge_fwd(const PRMeshLossArgs* args, void* stream) {
  if (int e = mesh_check(args, "mesh_edge_fwd", false, true)) return e;
  const PRMeshLossArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nb = loss_blocks(a.V);
  edge_fwd_kernel<<<nb, kThreads, 0, st>>>(a);
  if (int e = check_launch("mesh_edge_fwd")) return e;
  mesh_finalize_kernel<<<1, kThreads, 0, st>>>(a.partials, nb, a.loss);
  return check_launch("mesh_finalize");
}

extern "C" int pr_mesh_edge_bwd(const PRMeshLossArgs* args, void* stream) {
  if (int e = mesh_check(args, "mesh_edge_bwd", false, false)) return e;
  const PRMeshLossArgs& a = *args;
  edge_bwd_kernel<<<(int)std::min<int64_t>((a.V + kThreads - 1) / kThreads, 4096), kThreads, 0,
                    reinterpret_cast<hipStream_t>(stream)>>>(a);
  return check_launch("mesh_edge_bwd");
}

extern "C" int pr_mesh_normal_consistency_fwd(const PRNormalConsistencyArgs* args, void* stream) {
  if (int e = normal_check(args, "mesh_normal_consistency_fwd", true)) return e;
  const PRNormalConsistencyArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nb = loss_blocks(a.F);
  face_normal_kernel<<<nb, kThreads, 0, st>>>(a);
  if (int e = check_launch("mesh_face_normal")) return e;
  normal_pairs_kernel<<<nb, kThreads, 0, st>>>(a);
  if (int e = check_launch("mesh_normal_pairs")) return e;
  mesh_finalize_kernel<<<1, kThreads, 0, st>>>(a.partials, nb, a.loss);
  return check_launch("mesh_finalize");
}

extern "C" int pr_mesh_normal_consistency_bwd(const PRNormalConsistencyArgs* args, void* stream) {
  if (int e = normal_check(args, "mesh_normal_consistency_bwd", false)) return e;
  const PRNormalConsistencyArgs& a = *args;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  normal_face_bwd_kernel<<<(int)std::min<int64_t>((a.F + kThreads - 1) / kThreads, 4096), kThreads, 0, st>>>(a);
  if (int e = check_launch("mesh_normal_face_bwd")) return e;
  normal_vert_bwd_kernel<<<(int)std::min<int64_t>((a.V + kThreads - 1) / kThreads, 4096), kThreads, 0, st>>>(a);
  return check_launch("mesh_normal_vert_bwd");
}
