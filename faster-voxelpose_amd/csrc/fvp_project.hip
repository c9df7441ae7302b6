// Back-projection kernels (gfx950): heatmap staging, sampling grids, whole-space cubes with
// fused z-max, per-person cubes, orthographic tri-plane maxima, and the fused
// project+tri-plane fast path.  Reference sites: lib/models/project_whole.py:49-88,
// lib/models/project_individual.py:60-136, lib/models/joint_localization_net.py:80-81,
// lib/models/cnns_2d.py:174.
//
// Data layout in HBM
//   heat     [B][V][J][H][W]        NCHW, as the reference hands it over
//   heat_cl  [B][V][H*W][JP]        channels-last, JP = 4*ceil(J/4): one bilinear tap of one
//                                   (voxel, view) is JP contiguous floats = JP/4 dwordx4 loads
//                                   shared by all joints (the reference gathers J planes)
//   cubes    [B][J][X][Y][Z]        z fastest (reference layout)
//   planes   [nP][3][J][C][C]       xy | xz | yz maxima of one person's cube
// All kernels are HBM/L2-bound gathers; lanes run along z so loads of neighbouring voxels hit
// neighbouring heatmap pixels and every store is a contiguous 256-byte row.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdlib>

#include "fvp_common.h"
#include "fvp_geom.h"

namespace fvp {

// ---------------------------------------------------------------------------------------------
// NCHW -> channels-last staging: one thread per pixel, coalesced reads per channel plane,
// JP/4 dwordx4 stores per thread.
template <int NV>
__global__ void __launch_bounds__(256) k_heat_to_cl(const float* __restrict__ heat, float* __restrict__ cl,
                                                    int J, int HW) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const size_t bv = blockIdx.y;
  if (pix >= HW) return;
  const float* src = heat + bv * size_t(J) * HW + pix;
  float v[4 * NV];
#pragma unroll
  for (int j = 0; j < 4 * NV; ++j) v[j] = (j < J) ? src[size_t(j) * HW] : 0.0f;
  float4* dst = reinterpret_cast<float4*>(cl + (bv * HW + pix) * size_t(4 * NV));
#pragma unroll
  for (int q = 0; q < NV; ++q) dst[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// ---------------------------------------------------------------------------------------------
// Sampling grid for the drop-in cache / parity tests: one thread per (view, voxel).
__global__ void __launch_bounds__(256) k_sample_grid(const float* __restrict__ ax, const float* __restrict__ ay,
                                                     const float* __restrict__ az, int nx, int ny, int nz,
                                                     const Cam* __restrict__ cams, FvpGeom g,
                                                     float* __restrict__ grid) {
  const int n = nx * ny * nz;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int v = blockIdx.y;
  if (i >= n) return;
  const int iz = i % nz, iy = (i / nz) % ny, ix = i / (nz * ny);
  float gx, gy;
  project_norm(cams[v], g, ax[ix], ay[iy], az[iz], gx, gy);
  grid[(size_t(v) * n + i) * 2 + 0] = gx;
  grid[(size_t(v) * n + i) * 2 + 1] = gy;
}

// mean over views of the bilinear samples of one world point, clamped to [0,1]
// (project_whole.py:83,86 / project_individual.py:130,134): sum views in order, divide by V.
template <int NV>
__device__ __forceinline__ void backproject_point(const float* __restrict__ heat_cl_frame,
                                                  const Cam* __restrict__ cams, const FvpGeom& g, float wx,
                                                  float wy, float wz, float (&acc)[4 * NV]) {
  const size_t view_stride = size_t(g.H) * g.W * (4 * NV);
  for (int v = 0; v < g.V; ++v) {
    float gx, gy;
    project_norm(cams[v], g, wx, wy, wz, gx, gy);
    const Taps t = bilinear_taps(gx, gy, g.W, g.H);
    float s[4 * NV];
    if (t.inside) {
      sample_view<NV>(heat_cl_frame + v * view_stride, t, s);
    } else {
#pragma unroll
      for (int c = 0; c < 4 * NV; ++c) s[c] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) acc[c] = (v == 0) ? s[c] : __fadd_rn(acc[c], s[c]);
  }
  const float nv = float(g.V);
#pragma unroll
  for (int c = 0; c < 4 * NV; ++c) acc[c] = clampf(__fdiv_rn(acc[c], nv), 0.0f, 1.0f);
}

// ---------------------------------------------------------------------------------------------
// Joint evidence: what backproject_point would put into a voxel centred on each fused joint, kept per view.
// One lane per (frame, person slot, joint) walks the views in order; channel j is one scalar load per tap
// (the value sample_view computes for that channel: same taps, weights and fma chain).  A few thousand items:
// the launch is latency-bound, nothing here is tuned.
//   views[b][v][n][j] = (px, py, depth, s_v)   pixel in the original image before the clamp, camera-space z
//   conf[b][n][j]     = clamp01((s_0 + ... + s_{V-1}) / V)
// Slots with fused[b][n][0][3] < 0 are written as zeros.
__global__ void __launch_bounds__(256)
k_joint_evidence(const float* __restrict__ heat_cl, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                 const float* __restrict__ fused, int B, int N, FvpGeom g, float* __restrict__ views,
                 float* __restrict__ conf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int J = g.J, JP = g.JP;
  if (i >= B * N * J) return;
  const int bn = i / J, j = i - bn * J;
  const int b = bn / N, n = bn - b * N;
  const bool valid = fused[size_t(bn) * J * 5 + 3] >= 0.0f;
  const float* p = fused + size_t(i) * 5;
  const float wx = p[0], wy = p[1], wz = p[2];
  const size_t view_stride = size_t(g.H) * g.W * JP;
  const float* frame = heat_cl + size_t(b) * g.V * view_stride;
  const Cam* cm = cams + size_t(frame_set[b]) * g.V;
  float acc = 0.0f;
  for (int v = 0; v < g.V; ++v) {
    float px = 0.0f, py = 0.0f, depth = 0.0f, s = 0.0f;
    if (valid) {
      float gx, gy;
      project_pixel(cm[v], wx, wy, wz, px, py, depth);
      pixel_to_norm(g, px, py, gx, gy);
      const Taps t = bilinear_taps(gx, gy, g.W, g.H);
      if (t.inside) {
        const float* cl = frame + v * view_stride + j;
        float h[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = ((t.inside >> k) & 1) ? cl[size_t(t.off[k]) * JP] : 0.0f;
        s = __fmul_rn(h[0], t.w[0]);
#pragma unroll
        for (int k = 1; k < 4; ++k) s = __fmaf_rn(h[k], t.w[k], s);
      }
    }
    acc = (v == 0) ? s : __fadd_rn(acc, s);
    if (views)
      reinterpret_cast<float4*>(views)[((size_t(b) * g.V + v) * N + n) * J + j] = make_float4(px, py, depth, s);
  }
  if (conf) conf[i] = clampf(__fdiv_rn(acc, float(g.V)), 0.0f, 1.0f);
}

// ---------------------------------------------------------------------------------------------
// Joint visibility per view (fvp_joint_visibility, include/fvp.h): the ray from the camera centre to a joint against the
// capsule model of every present person of the frame.  One workgroup per (frame, person slot): the frame's N*J joints
// (w = 1 iff finite) and the presence flags are staged in LDS, thread t < V*J owns (v, j) = (t / J, t % J) and walks the
// persons and primitives in order - every LDS read and every table read (the table is a kernel argument) is uniform over
// the workgroup.  Per-view results go through LDS; thread j < J sums the seeing views in ascending v.  No atomics.
struct VisPrims {
  int n;
  int ik[FVP_VIS_MAX_PRIMS];        // i | k << 8
  float r[FVP_VIS_MAX_PRIMS];
};

__device__ __forceinline__ float dot3(float p0, float p1, float p2, float q0, float q1, float q2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(p0, q0), __fmul_rn(p1, q1)), __fmul_rn(p2, q2));
}

__global__ void __launch_bounds__(256)
k_joint_visibility(const float* __restrict__ fused, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                   const int* __restrict__ ids, const float* __restrict__ views, int V, int N, int J, VisPrims prm,
                   float guard, float xmax, float ymax, int* __restrict__ occluder, float* __restrict__ vis_conf,
                   int* __restrict__ vis_count) {
  __shared__ float4 pose[FVP_VIS_MAX_PEOPLE * FVP_MAX_JOINTS];
  __shared__ int present[FVP_VIS_MAX_PEOPLE];
  __shared__ float seen_s[FVP_MAX_VIEWS * FVP_MAX_JOINTS];
  __shared__ int seen[FVP_MAX_VIEWS * FVP_MAX_JOINTS];
  const int b = blockIdx.x / N, n = blockIdx.x - b * N;
  const int tid = threadIdx.x;
  const float* frame = fused + size_t(b) * N * J * 5;
  for (int q = tid; q < N * J; q += 256) {
    const float x = frame[q * 5 + 0], y = frame[q * 5 + 1], z = frame[q * 5 + 2];
    const bool fin = fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;
    pose[q] = make_float4(x, y, z, fin ? 1.0f : 0.0f);
  }
  if (tid < N) present[tid] = frame[tid * J * 5 + 3] >= 0.0f && (!ids || ids[b * N + tid] >= 0);
  __syncthreads();
  const int v = tid / J, j = tid - v * J;
  if (v < V) {
    const Cam& cm = cams[size_t(frame_set[b]) * V + v];
    const float c0 = cm.T[0], c1 = cm.T[1], c2 = cm.T[2];
    const float4 P = pose[n * J + j];
    const float d10 = __fsub_rn(P.x, c0), d11 = __fsub_rn(P.y, c1), d12 = __fsub_rn(P.z, c2);
    const float a = dot3(d10, d11, d12, d10, d11, d12);
    const float len = sqrtf(a);
    int occ = -2;
    if (present[n] && P.w != 0.0f && len > guard) {
      const float smax = __fsub_rn(1.0f, __fdiv_rn(guard, len));
      float best = 0.0f;
      occ = -1;
      for (int m = 0; m < N; ++m) {
        if (!present[m]) continue;
        for (int l = 0; l < prm.n; ++l) {
          const int pi = prm.ik[l] & 255, pk = prm.ik[l] >> 8;
          const float4 A = pose[m * J + pi], Bq = pose[m * J + pk];
          if (A.w == 0.0f || Bq.w == 0.0f || (m == n && (pi == j || pk == j))) continue;
          const float d20 = __fsub_rn(Bq.x, A.x), d21 = __fsub_rn(Bq.y, A.y), d22 = __fsub_rn(Bq.z, A.z);
          const float r00 = __fsub_rn(c0, A.x), r01 = __fsub_rn(c1, A.y), r02 = __fsub_rn(c2, A.z);
          const float e = dot3(d20, d21, d22, d20, d21, d22);
          const float f = dot3(d20, d21, d22, r00, r01, r02);
          const float c = dot3(d10, d11, d12, r00, r01, r02);
          float sv, tv;
          if (e == 0.0f) {
            tv = 0.0f;
            sv = clampf(__fdiv_rn(-c, a), 0.0f, smax);
          } else {
            const float bb = dot3(d10, d11, d12, d20, d21, d22);
            const float den = __fsub_rn(__fmul_rn(a, e), __fmul_rn(bb, bb));
            sv = den > 0.0f ? clampf(__fdiv_rn(__fsub_rn(__fmul_rn(bb, f), __fmul_rn(c, e)), den), 0.0f, smax) : 0.0f;
            tv = __fdiv_rn(__fadd_rn(__fmul_rn(bb, sv), f), e);
            if (tv < 0.0f) {
              tv = 0.0f;
              sv = clampf(__fdiv_rn(-c, a), 0.0f, smax);
            } else if (tv > 1.0f) {
              tv = 1.0f;
              sv = clampf(__fdiv_rn(__fsub_rn(bb, c), a), 0.0f, smax);
            }
          }
          const float w0 = __fsub_rn(__fadd_rn(c0, __fmul_rn(d10, sv)), __fadd_rn(A.x, __fmul_rn(d20, tv)));
          const float w1 = __fsub_rn(__fadd_rn(c1, __fmul_rn(d11, sv)), __fadd_rn(A.y, __fmul_rn(d21, tv)));
          const float w2 = __fsub_rn(__fadd_rn(c2, __fmul_rn(d12, sv)), __fadd_rn(A.z, __fmul_rn(d22, tv)));
          const float rr = __fmul_rn(prm.r[l], prm.r[l]);
          // persons in ascending m and a strict compare: among equal s the lowest slot stays
          if (dot3(w0, w1, w2, w0, w1, w2) <= rr && (occ < 0 || sv < best)) {
            best = sv;
            occ = m;
          }
        }
      }
    }
    const size_t o = ((size_t(b) * V + v) * N + n) * J + j;
    if (occluder) occluder[o] = occ;
    if (views) {
      const float4 e4 = reinterpret_cast<const float4*>(views)[o];
      seen[tid] = occ == -1 && e4.z > 0.0f && e4.x >= 0.0f && e4.x <= xmax && e4.y >= 0.0f && e4.y <= ymax;
      seen_s[tid] = e4.w;
    }
  }
  if (!views) return;                 // uniform: a kernel argument
  __syncthreads();
  if (tid < J) {
    float sum = 0.0f;
    int cnt = 0;
    for (int u = 0; u < V; ++u)
      if (seen[u * J + tid]) {
        sum = __fadd_rn(sum, seen_s[u * J + tid]);
        ++cnt;
      }
    const size_t o = (size_t(b) * N + n) * J + tid;
    if (vis_conf) vis_conf[o] = cnt ? clampf(__fdiv_rn(sum, float(cnt)), 0.0f, 1.0f) : 0.0f;
    if (vis_count) vis_count[o] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------
// Triangulated joints from the views (fvp_triangulate_joints, include/fvp.h): the point the rays through the 2-D heatmap
// peaks of the usable views agree on, its reprojection residual per view and the residual per camera.  One workgroup per
// (frame, person slot); the set's camera records are staged in LDS once.  Thread t < V*J owns (v, j) = (t / J, t % J) for
// steps 1-6 of the definition - the window around the reprojected fused joint, the peak, its sub-cell refinement, the
// pixel in the original image, the undistorted ray - and leaves ray, weight, observation and state in LDS.  Thread j < J
// then solves its joint's 3x3 normal equations in fp64 over the views in ascending order (named scalars: no indexed local
// arrays, nothing in scratch), computes the residuals, runs the one rejection round and writes the per-joint outputs;
// the (v, j) threads write obs and view_state.  No atomics.  Every window load lies inside the map: the loops run over the
// window clipped to the map, and the centre is tested as a float before it becomes an int.
struct TriParams {
  float inv[6];                     // heat-map cell -> original pixel (the host's inverse, fp32)
  int radius, iters, min_views, nsets;
  float min_peak, reject_px;
  double min_det;
};

__device__ __forceinline__ float tri_refine(float m, float c, float p) {
  const float den = __fsub_rn(__fsub_rn(__fmul_rn(2.0f, c), m), p);
  return den > 0.0f ? clampf(__fdiv_rn(__fmul_rn(0.5f, __fsub_rn(p, m)), den), -0.5f, 0.5f) : 0.0f;
}

// step 5: the observed pixel of the original image back through the lens model, `iters` fixed-point rounds from y = u
// (shared with the camera re-fit below: one function, one set of bits)
__device__ __forceinline__ void tri_undistort(const Cam& cm, float ox, float oy, int iters, float& y0n, float& y1n) {
  const float u0 = __fdiv_rn(__fsub_rn(ox, cm.c[0]), cm.f[0]), u1 = __fdiv_rn(__fsub_rn(oy, cm.c[1]), cm.f[1]);
  y0n = u0, y1n = u1;
  for (int it = 0; it < iters; ++it) {
    const float rr = __fadd_rn(__fmul_rn(y0n, y0n), __fmul_rn(y1n, y1n));
    float d = __fadd_rn(1.0f, __fmul_rn(cm.k[0], rr));
    d = __fadd_rn(d, __fmul_rn(__fmul_rn(cm.k[1], rr), rr));
    d = __fadd_rn(d, __fmul_rn(__fmul_rn(__fmul_rn(cm.k[2], rr), rr), rr));
    const float t0 = __fadd_rn(__fmul_rn(__fmul_rn(__fmul_rn(2.0f, cm.p[0]), y0n), y1n),
                               __fmul_rn(cm.p[1], __fadd_rn(rr, __fmul_rn(__fmul_rn(2.0f, y0n), y0n))));
    const float t1 = __fadd_rn(__fmul_rn(__fmul_rn(__fmul_rn(2.0f, cm.p[1]), y0n), y1n),
                               __fmul_rn(cm.p[0], __fadd_rn(rr, __fmul_rn(__fmul_rn(2.0f, y1n), y1n))));
    y0n = __fdiv_rn(__fsub_rn(u0, t0), d);
    y1n = __fdiv_rn(__fsub_rn(u1, t1), d);
  }
}

// steps 1-6 for one (view, joint): the state, the ray (d, w) and the observation (ox, oy, peak, -1)
__device__ __forceinline__ int tri_observe(const float* __restrict__ cl, const Cam& cm, const FvpGeom& g,
                                           const TriParams& tp, float wx, float wy, float wz, float4& ray, float4& ob) {
  if (!(fabsf(wx) <= FLT_MAX && fabsf(wy) <= FLT_MAX && fabsf(wz) <= FLT_MAX)) return FVP_TRI_OUTSIDE;
  float px, py, depth;
  project_pixel(cm, wx, wy, wz, px, py, depth);
  if (!(depth > 0.0f)) return FVP_TRI_OUTSIDE;
  const float ax = __fmaf_rn(g.rt[2], 1.0f, __fmaf_rn(g.rt[1], py, __fmul_rn(g.rt[0], px)));
  const float ay = __fmaf_rn(g.rt[5], 1.0f, __fmaf_rn(g.rt[4], py, __fmul_rn(g.rt[3], px)));
  const float hx = __fdiv_rn(__fmul_rn(ax, g.hm_w), g.img_w);
  const float hy = __fdiv_rn(__fmul_rn(ay, g.hm_h), g.img_h);
  if (!(fabsf(hx) <= FLT_MAX && fabsf(hy) <= FLT_MAX)) return FVP_TRI_OUTSIDE;
  const float cxf = floorf(__fadd_rn(hx, 0.5f)), cyf = floorf(__fadd_rn(hy, 0.5f));
  const int r = tp.radius, W = g.W, H = g.H, JP = g.JP;
  // as floats, before any conversion: a centre whose window holds no cell of the map costs no load
  if (!(cxf >= float(-r) && cxf <= float(W - 1 + r) && cyf >= float(-r) && cyf <= float(H - 1 + r))) return FVP_TRI_OUTSIDE;
  const int cx = int(cxf), cy = int(cyf);
  const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < W - 1 ? cx + r : W - 1;
  const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < H - 1 ? cy + r : H - 1;
  bool have = false;
  float best = 0.0f;
  int bx = 0, by = 0;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      const float val = cl[size_t(y * W + x) * JP];
      // ascending (y, x) and a strict compare: a tie stays with the smallest (y, x); a NaN never wins
      if (val == val && (!have || val > best)) {
        have = true;
        best = val;
        bx = x;
        by = y;
      }
    }
  if (!have) return FVP_TRI_PEAK_LOW;
  ob.z = best;
  if (!(best >= tp.min_peak)) return FVP_TRI_PEAK_LOW;
  if (bx == cx - r || bx == cx + r || by == cy - r || by == cy + r) return FVP_TRI_NOT_ENCLOSED;
  // the winner is inside the map; a neighbour outside it counts as 0
  const float xm = bx > 0 ? cl[size_t(by * W + bx - 1) * JP] : 0.0f;
  const float xp = bx < W - 1 ? cl[size_t(by * W + bx + 1) * JP] : 0.0f;
  const float ym = by > 0 ? cl[size_t((by - 1) * W + bx) * JP] : 0.0f;
  const float yp = by < H - 1 ? cl[size_t((by + 1) * W + bx) * JP] : 0.0f;
  const float qx = __fadd_rn(float(bx), tri_refine(xm, best, xp));
  const float qy = __fadd_rn(float(by), tri_refine(ym, best, yp));
  const float ox = __fmaf_rn(tp.inv[2], 1.0f, __fmaf_rn(tp.inv[1], qy, __fmul_rn(tp.inv[0], qx)));
  const float oy = __fmaf_rn(tp.inv[5], 1.0f, __fmaf_rn(tp.inv[4], qy, __fmul_rn(tp.inv[3], qx)));
  ob.x = ox;
  ob.y = oy;
  float y0n, y1n;
  tri_undistort(cm, ox, oy, tp.iters, y0n, y1n);
  const float g0 = __fadd_rn(__fadd_rn(__fmul_rn(cm.R[0], y0n), __fmul_rn(cm.R[3], y1n)), cm.R[6]);
  const float g1 = __fadd_rn(__fadd_rn(__fmul_rn(cm.R[1], y0n), __fmul_rn(cm.R[4], y1n)), cm.R[7]);
  const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(cm.R[2], y0n), __fmul_rn(cm.R[5], y1n)), cm.R[8]);
  const float len = sqrtf(dot3(g0, g1, g2, g0, g1, g2));
  ray = make_float4(__fdiv_rn(g0, len), __fdiv_rn(g1, len), __fdiv_rn(g2, len), clampf(best, 0.0f, 1.0f));
  return FVP_TRI_USED;
}

// step 8 over the views of `mask`, ascending: false iff degenerate
__device__ __forceinline__ bool tri_solve(const float4* ray_s, const Cam* cam_s, int V, int J, int j, unsigned mask,
                                          double min_det, float& X0, float& X1, float& X2) {
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int u = 0; u < V; ++u) {
    if (!((mask >> u) & 1u)) continue;
    const float4 q = ray_s[u * J + j];
    const double dx = q.x, dy = q.y, dz = q.z, w = q.w;
    const double c0 = cam_s[u].T[0], c1 = cam_s[u].T[1], c2 = cam_s[u].T[2];
    const double m00 = 1.0 - dx * dx, m11 = 1.0 - dy * dy, m22 = 1.0 - dz * dz;
    const double m01 = -(dx * dy), m02 = -(dx * dz), m12 = -(dy * dz);
    a00 = a00 + w * m00;
    a01 = a01 + w * m01;
    a02 = a02 + w * m02;
    a11 = a11 + w * m11;
    a12 = a12 + w * m12;
    a22 = a22 + w * m22;
    b0 = b0 + w * ((m00 * c0 + m01 * c1) + m02 * c2);
    b1 = b1 + w * ((m01 * c0 + m11 * c1) + m12 * c2);
    b2 = b2 + w * ((m02 * c0 + m12 * c1) + m22 * c2);
  }
  const double k00 = a11 * a22 - a12 * a12, k01 = a02 * a12 - a01 * a22, k02 = a01 * a12 - a02 * a11;
  const double k11 = a00 * a22 - a02 * a02, k12 = a01 * a02 - a00 * a12, k22 = a00 * a11 - a01 * a01;
  const double det = (a00 * k00 + a01 * k01) + a02 * k02;
  const double t3 = ((a00 + a11) + a22) / 3.0;
  if (!(det > min_det * ((t3 * t3) * t3))) return false;          // a NaN fails
  X0 = float(((k00 * b0 + k01 * b1) + k02 * b2) / det);
  X1 = float(((k01 * b0 + k11 * b1) + k12 * b2) / det);
  X2 = float(((k02 * b0 + k12 * b1) + k22 * b2) / det);
  return true;
}

// step 9 over the views of `mask`: e_v into the observation's fourth element
__device__ __forceinline__ void tri_residuals(float4* ob_s, const Cam* cam_s, int V, int J, int j, unsigned mask, float X0,
                                              float X1, float X2) {
  for (int u = 0; u < V; ++u) {
    if (!((mask >> u) & 1u)) continue;
    float px, py, depth;
    project_pixel(cam_s[u], X0, X1, X2, px, py, depth);
    const float ex = __fsub_rn(px, ob_s[u * J + j].x), ey = __fsub_rn(py, ob_s[u * J + j].y);
    ob_s[u * J + j].w = sqrtf(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)));
  }
}

__global__ void __launch_bounds__(256)
k_triangulate_joints(const float* __restrict__ heat_cl, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                     const float* __restrict__ fused, const int* __restrict__ ids, const int* __restrict__ occluder, int N,
                     FvpGeom g, TriParams tp, float* __restrict__ tri_poses, int* __restrict__ tri_count,
                     float* __restrict__ tri_stats, float* __restrict__ obs, int* __restrict__ view_state) {
  __shared__ Cam cam_s[FVP_MAX_VIEWS];
  __shared__ float4 ray_s[256];
  __shared__ float4 ob_s[256];
  __shared__ int st_s[256];
  const int V = g.V, J = g.J;
  const int b = blockIdx.x / N, n = blockIdx.x - b * N;
  const int tid = threadIdx.x;
  const int set = frame_set[b];
  const float* person = fused + (size_t(b) * N + n) * J * 5;
  // uniform over the workgroup; a camera set outside the table is never read
  const bool evaluated = set >= 0 && set < tp.nsets && person[3] >= 0.0f && (!ids || ids[b * N + n] >= 0);
  if (evaluated && tid < V * FVP_CAM_FLOATS)
    reinterpret_cast<float*>(cam_s)[tid] = reinterpret_cast<const float*>(cams + size_t(set) * V)[tid];
  __syncthreads();
  const int v = tid / J, j = tid - v * J;
  const size_t o = ((size_t(b) * V + v) * N + n) * J + j;
  if (v < V) {
    int state = FVP_TRI_NOT_EVALUATED;
    float4 ray = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ob = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (evaluated) {
      const float* cl = heat_cl + (size_t(b) * V + v) * g.H * g.W * g.JP + j;
      state = tri_observe(cl, cam_s[v], g, tp, person[j * 5 + 0], person[j * 5 + 1], person[j * 5 + 2], ray, ob);
      if (state == FVP_TRI_USED && occluder && occluder[o] != -1) state = FVP_TRI_OCCLUDED;
    }
    ray_s[tid] = ray;
    ob_s[tid] = ob;
    st_s[tid] = state;
  }
  __syncthreads();
  if (tid < J) {
    const float P0 = person[tid * 5 + 0], P1 = person[tid * 5 + 1], P2 = person[tid * 5 + 2];
    float X0 = P0, X1 = P1, X2 = P2, shift = 0.0f, rms = 0.0f;
    int count = -2;
    if (evaluated) {
      unsigned mask = 0;
      int usable = 0;
      for (int u = 0; u < V; ++u)
        if (st_s[u * J + tid] == FVP_TRI_USED) {
          mask |= 1u << u;
          ++usable;
        }
      count = usable;
      float Y0 = 0.0f, Y1 = 0.0f, Y2 = 0.0f;
      if (usable >= tp.min_views) {
        if (!tri_solve(ray_s, cam_s, V, J, tid, mask, tp.min_det, Y0, Y1, Y2)) {
          count = -1;
        } else {
          tri_residuals(ob_s, cam_s, V, J, tid, mask, Y0, Y1, Y2);
          if (tp.reject_px > 0.0f) {
            unsigned keep = 0;
            int kept = 0;
            for (int u = 0; u < V; ++u)
              if (((mask >> u) & 1u) && !(ob_s[u * J + tid].w > tp.reject_px)) {
                keep |= 1u << u;
                ++kept;
              }
            float Z0, Z1, Z2;
            if (keep != mask && kept >= tp.min_views && tri_solve(ray_s, cam_s, V, J, tid, keep, tp.min_det, Z0, Z1, Z2)) {
              for (int u = 0; u < V; ++u)
                if (((mask & ~keep) >> u) & 1u) {
                  st_s[u * J + tid] = FVP_TRI_REJECTED;
                  ob_s[u * J + tid].w = -1.0f;
                }
              mask = keep;
              count = kept;
              Y0 = Z0, Y1 = Z1, Y2 = Z2;
              tri_residuals(ob_s, cam_s, V, J, tid, mask, Y0, Y1, Y2);
            }
          }
          X0 = Y0, X1 = Y1, X2 = Y2;
          const float s0 = __fsub_rn(X0, P0), s1 = __fsub_rn(X1, P1), s2 = __fsub_rn(X2, P2);
          shift = sqrtf(dot3(s0, s1, s2, s0, s1, s2));
          float num = 0.0f, den = 0.0f;
          for (int u = 0; u < V; ++u) {
            if (!((mask >> u) & 1u)) continue;
            const float e = ob_s[u * J + tid].w, w = ray_s[u * J + tid].w;
            num = __fadd_rn(num, __fmul_rn(w, __fmul_rn(e, e)));
            den = __fadd_rn(den, w);
          }
          rms = sqrtf(__fdiv_rn(num, den));
        }
      }
      if (count < tp.min_views)                       // too few views or degenerate: the usable views solved nothing
        for (int u = 0; u < V; ++u)
          if ((mask >> u) & 1u) st_s[u * J + tid] = FVP_TRI_UNSOLVED;
    }
    const size_t q = (size_t(b) * N + n) * J + tid;
    if (tri_poses) {
      tri_poses[q * 5 + 0] = X0;
      tri_poses[q * 5 + 1] = X1;
      tri_poses[q * 5 + 2] = X2;
      tri_poses[q * 5 + 3] = person[tid * 5 + 3];
      tri_poses[q * 5 + 4] = person[tid * 5 + 4];
    }
    if (tri_count) tri_count[q] = count;
    if (tri_stats) {
      tri_stats[q * 2 + 0] = shift;
      tri_stats[q * 2 + 1] = rms;
    }
  }
  __syncthreads();
  if (v < V) {
    if (obs) reinterpret_cast<float4*>(obs)[o] = ob_s[tid];
    if (view_state) view_state[o] = st_s[tid];
  }
}

// The residual per camera: one workgroup per (frame, view) over the N*J joint-views of obs / view_state.  Thread t sums the
// used entries t, t + 256, ... in ascending order, then a tree of fixed shape (stride 128, 64, ..., 1) folds the 256
// partial sums: the value does not depend on scheduling.
__global__ void __launch_bounds__(256)
k_view_residual(const float* __restrict__ obs, const int* __restrict__ view_state, int NJ, float* __restrict__ cam_resid,
                int* __restrict__ cam_count) {
  __shared__ float sum_s[256];
  __shared__ int cnt_s[256];
  const int tid = threadIdx.x;
  const float4* ob = reinterpret_cast<const float4*>(obs) + size_t(blockIdx.x) * NJ;
  const int* st = view_state + size_t(blockIdx.x) * NJ;
  float sum = 0.0f;
  int cnt = 0;
  for (int q = tid; q < NJ; q += 256)
    if (st[q] == FVP_TRI_USED) {
      sum = __fadd_rn(sum, ob[q].w);
      ++cnt;
    }
  sum_s[tid] = sum;
  cnt_s[tid] = cnt;
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      sum_s[tid] = __fadd_rn(sum_s[tid], sum_s[tid + stride]);
      cnt_s[tid] += cnt_s[tid + stride];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (cam_resid) cam_resid[blockIdx.x] = cnt_s[0] ? __fdiv_rn(sum_s[0], float(cnt_s[0])) : 0.0f;
    if (cam_count) cam_count[blockIdx.x] = cnt_s[0];
  }
}

// ---------------------------------------------------------------------------------------------
// Camera re-fit (fvp_camera_refit_accumulate / fvp_camera_refit_solve, include/fvp.h): a robust resection of every camera
// against the 3-D joints, one Gauss-Newton step on its six extrinsic parameters.  All of it in fp64, every operation
// rounded on its own (this file is built without contraction); only the undistortion is the triangulation's fp32 function.
//
// Accumulate: one workgroup of 256 threads per camera (set, view).  Thread t walks the joint-views q = t, t + 256, ... of
// the whole batch in ascending order and keeps the 31 sums of its counting entries in registers (every index below is a
// compile-time constant after unrolling: nothing in scratch); the 256 partial vectors then fold through LDS in four slices
// of eight elements, [element][thread] so that neighbouring lanes touch neighbouring doubles, as a tree of fixed shape
// (stride 128, 64, ..., 1).  No atomics: the sums do not depend on scheduling.
__host__ __device__ constexpr int refit_ut(int i, int k) { return i * 6 - i * (i - 1) / 2 + (k - i); }   // H_ik, i <= k
__host__ __device__ constexpr int refit_lt(int i, int k) { return i * (i + 1) / 2 + k; }                 // L_ik, k <= i

__global__ void __launch_bounds__(256)
k_camera_refit_accumulate(const float* __restrict__ points, const float* __restrict__ obs,
                          const int* __restrict__ view_state, const Cam* __restrict__ cams,
                          const int* __restrict__ frame_set, int B, int V, int NJ, int iters, float huber_px, float decay,
                          double* __restrict__ acc) {
  __shared__ double red_s[8 * 256];
  const int tid = threadIdx.x;
  const int set = blockIdx.x / V, v = blockIdx.x - set * V;
  const Cam cm = cams[blockIdx.x];
  const double f0 = cm.f[0], f1 = cm.f[1], hub = huber_px;
  double p[FVP_CAL_ACC];
#pragma unroll
  for (int i = 0; i < FVP_CAL_ACC; ++i) p[i] = 0.0;
  const int total = B * NJ;
  for (int q = tid; q < total; q += 256) {
    const int b = q / NJ;
    if (frame_set[b] != set) continue;
    const size_t o = (size_t(b) * V + v) * NJ + (q - b * NJ);
    if (view_state[o] != FVP_TRI_USED) continue;
    const float X0 = points[size_t(q) * 5 + 0], X1 = points[size_t(q) * 5 + 1], X2 = points[size_t(q) * 5 + 2];
    const float4 ob = reinterpret_cast<const float4*>(obs)[o];
    if (!(fabsf(X0) <= FLT_MAX && fabsf(X1) <= FLT_MAX && fabsf(X2) <= FLT_MAX)) continue;
    if (!(fabsf(ob.x) <= FLT_MAX && fabsf(ob.y) <= FLT_MAX)) continue;
    const float wf = clampf(ob.z, 0.0f, 1.0f);
    if (!(wf > 0.0f)) continue;
    const double d0 = double(X0) - double(cm.T[0]), d1 = double(X1) - double(cm.T[1]), d2 = double(X2) - double(cm.T[2]);
    const double xc0 = (double(cm.R[0]) * d0 + double(cm.R[1]) * d1) + double(cm.R[2]) * d2;
    const double xc1 = (double(cm.R[3]) * d0 + double(cm.R[4]) * d1) + double(cm.R[5]) * d2;
    const double z = (double(cm.R[6]) * d0 + double(cm.R[7]) * d1) + double(cm.R[8]) * d2;
    if (!(z > 1.0)) continue;
    float y0f, y1f;
    tri_undistort(cm, ob.x, ob.y, iters, y0f, y1f);
    const double iz = 1.0 / z, u = xc0 / z, w = xc1 / z;
    const double r0 = (double(y0f) - u) * f0, r1 = (double(y1f) - w) * f1;
    const double Ju[6] = {f0 * (-(u * w)), f0 * (1.0 + u * u), f0 * (-w), f0 * iz, 0.0, f0 * (-(u * iz))};
    const double Jv[6] = {f1 * (-(1.0 + w * w)), f1 * (u * w), f1 * u, 0.0, f1 * iz, f1 * (-(w * iz))};
    const double e2 = r0 * r0 + r1 * r1, e = sqrt(e2);
    const double h = (hub > 0.0 && e > hub) ? hub / e : 1.0;
    const double ww = double(wf) * h;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = i; k < 6; ++k) p[refit_ut(i, k)] = p[refit_ut(i, k)] + ww * ((Ju[i] * Ju[k]) + (Jv[i] * Jv[k]));
      p[21 + i] = p[21 + i] + ww * ((Ju[i] * r0) + (Jv[i] * r1));
    }
    p[27] = p[27] + ww;
    p[28] = p[28] + ww * e2;
    p[29] = p[29] + 1.0;
    p[30] = p[30] + (h < 1.0 ? 1.0 : 0.0);
  }
  double* out = acc + size_t(blockIdx.x) * FVP_CAL_ACC;
#pragma unroll
  for (int sl = 0; sl < FVP_CAL_ACC / 8; ++sl) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red_s[i * 256 + tid] = p[sl * 8 + i];
    __syncthreads();
    for (int stride = 128; stride >= 1; stride >>= 1) {
      if (tid < stride) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red_s[i * 256 + tid] = red_s[i * 256 + tid] + red_s[i * 256 + tid + stride];
      }
      __syncthreads();
    }
    if (tid < 8) {
      const int i = sl * 8 + tid;
      out[i] = i == FVP_CAL_ACC - 1 ? 0.0 : out[i] * double(decay) + red_s[tid * 256];
    }
    __syncthreads();
  }
}

// Solve: one thread per camera.  The 6x6 system lives in named registers: every loop below has compile-time bounds and is
// unrolled, so that no array is indexed by a run-time value.  The Cholesky factor overwrites the scaled matrix in place.
__global__ void __launch_bounds__(64)
k_camera_refit_solve(const double* __restrict__ acc, const Cam* __restrict__ cams_in, int ncam, int min_obs, double lambda,
                     double min_pivot, double max_angle, double max_shift, Cam* __restrict__ cams_out,
                     float* __restrict__ cal_stats, int* __restrict__ cal_state) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= ncam) return;
  const double* a = acc + size_t(c) * FVP_CAL_ACC;
  Cam cm = cams_in[c];
  double g[6], D[6], A[21], dl[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = a[21 + i];
  const double sw = a[27], se = a[28], count = a[29];
  const double rms_before = sw > 0.0 ? sqrt(se / sw) : 0.0;
  double theta = 0.0, sigma = 0.0, rms_pred = 0.0, minpiv = 0.0;
  int state = FVP_CAL_OK;
  if (!(count >= double(min_obs))) state = FVP_CAL_FEW;
  if (state == FVP_CAL_OK) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double hii = a[refit_ut(i, i)];
      bad = bad || !(hii > 0.0);
      D[i] = sqrt(hii);
    }
    if (bad) state = FVP_CAL_DEGENERATE;
  }
  if (state == FVP_CAL_OK) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < i; ++k) A[refit_lt(i, k)] = a[refit_ut(k, i)] / (D[i] * D[k]);
      A[refit_lt(i, i)] = a[refit_ut(i, i)] / (D[i] * D[i]) + lambda;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double piv = A[refit_lt(j, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) piv = piv - A[refit_lt(j, k)] * A[refit_lt(j, k)];
      bad = bad || !(piv > min_pivot);                       // a NaN fails
      minpiv = (j == 0 || piv < minpiv) ? piv : minpiv;
      const double ljj = sqrt(piv);
      A[refit_lt(j, j)] = ljj;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double t = A[refit_lt(i, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) t = t - A[refit_lt(i, k)] * A[refit_lt(j, k)];
        A[refit_lt(i, j)] = t / ljj;
      }
    }
    if (bad) state = FVP_CAL_DEGENERATE;
  }
  if (state == FVP_CAL_OK) {
    double y[6], zt[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double t = g[i] / D[i];
#pragma unroll
      for (int k = 0; k < i; ++k) t = t - A[refit_lt(i, k)] * y[k];
      y[i] = t / A[refit_lt(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double t = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) t = t - A[refit_lt(k, i)] * zt[k];
      zt[i] = t / A[refit_lt(i, i)];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) dl[i] = zt[i] / D[i];
    theta = sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
    sigma = sqrt((dl[3] * dl[3] + dl[4] * dl[4]) + dl[5] * dl[5]);
    if (!(theta <= DBL_MAX && sigma <= DBL_MAX)) state = FVP_CAL_DEGENERATE;      // a step that is not finite is no step
  }
  if (state == FVP_CAL_OK) {
    const double gd = ((((g[0] * dl[0] + g[1] * dl[1]) + g[2] * dl[2]) + g[3] * dl[3]) + g[4] * dl[4]) + g[5] * dl[5];
    const double left = se - gd;
    rms_pred = sw > 0.0 ? sqrt((left > 0.0 ? left : 0.0) / sw) : 0.0;
    double kappa = 1.0;
    if (theta > max_angle) kappa = max_angle / theta;
    if (sigma > max_shift) {
      const double k2 = max_shift / sigma;
      if (k2 < kappa) kappa = k2;
    }
    if (kappa < 1.0) {
      state = FVP_CAL_CLAMPED;
#pragma unroll
      for (int i = 0; i < 6; ++i) dl[i] = dl[i] * kappa;
      theta = sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
      sigma = sqrt((dl[3] * dl[3] + dl[4] * dl[4]) + dl[5] * dl[5]);
    }
    // Cayley retraction: the unit quaternion (1, w/2) / |(1, w/2)| - no transcendental function anywhere
    const double h0 = 0.5 * dl[0], h1 = 0.5 * dl[1], h2 = 0.5 * dl[2];
    const double n = sqrt(1.0 + ((h0 * h0 + h1 * h1) + h2 * h2));
    const double qw = 1.0 / n, qx = h0 / n, qy = h1 / n, qz = h2 / n;
    const double C[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw),
                         2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw),
                         2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)};
    double Rn[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        Rn[3 * i + k] = (C[3 * i] * double(cm.R[k]) + C[3 * i + 1] * double(cm.R[3 + k])) + C[3 * i + 2] * double(cm.R[6 + k]);
    double Tn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Tn[k] = double(cm.T[k]) - ((Rn[k] * dl[3] + Rn[3 + k] * dl[4]) + Rn[6 + k] * dl[5]);
#pragma unroll
    for (int i = 0; i < 9; ++i) cm.R[i] = float(Rn[i]);
#pragma unroll
    for (int k = 0; k < 3; ++k) cm.T[k] = float(Tn[k]);
  } else {
    theta = sigma = rms_pred = minpiv = 0.0;
  }
  cams_out[c] = cm;
  if (cal_stats) {
    float* st = cal_stats + size_t(c) * 6;
    st[0] = float(theta);
    st[1] = float(sigma);
    st[2] = float(rms_before);
    st[3] = float(rms_pred);
    st[4] = float(count);
    st[5] = float(minpiv);
  }
  if (cal_state) cal_state[c] = state;
}

// ---------------------------------------------------------------------------------------------
// Whole-space cubes (+ fused z-max).  A workgroup owns CPB = 256/Z complete z-columns so the
// z-max never leaves the workgroup: values go through LDS [JP][256] and CPB*J threads each
// reduce one column of one joint.
template <int NV>
__global__ void __launch_bounds__(256)
k_project_whole(const float* __restrict__ heat_cl, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az, int X,
                int Y, int Z, FvpGeom g, float* __restrict__ cubes, float* __restrict__ zmax) {
  __shared__ float sm[4 * NV][256];
  const int cpb = 256 / Z;
  const int b = blockIdx.y;
  const int t = threadIdx.x;
  const int cl_ = t / Z, z = t - cl_ * Z;
  const int col = blockIdx.x * cpb + cl_;
  const int ncol = X * Y;
  const bool active = cl_ < cpb && col < ncol;
  const int J = g.J;
  float acc[4 * NV];
#pragma unroll
  for (int c = 0; c < 4 * NV; ++c) acc[c] = 0.0f;
  if (active) {
    const int x = col / Y, y = col - x * Y;
    const float* frame = heat_cl + size_t(b) * g.V * g.H * g.W * (4 * NV);
    backproject_point<NV>(frame, cams + size_t(frame_set[b]) * g.V, g, ax[x], ay[y], az[z], acc);
    if (cubes) {
      const size_t vox = size_t(col) * Z + z;
      const size_t nvox = size_t(ncol) * Z;
#pragma unroll
      for (int c = 0; c < 4 * NV; ++c)
        if (c < J) cubes[(size_t(b) * J + c) * nvox + vox] = acc[c];
    }
  }
  if (zmax) {
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) sm[c][t] = acc[c];
    __syncthreads();
    for (int item = t; item < cpb * J; item += 256) {
      const int c = item / cpb, k = item - c * cpb;
      const int cc = blockIdx.x * cpb + k;
      if (cc < ncol) {
        float m = sm[c][k * Z];
        for (int zz = 1; zz < Z; ++zz) m = fmaxf(m, sm[c][k * Z + zz]);
        zmax[(size_t(b) * J + c) * ncol + cc] = m;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Per-person cube, materialised (drop-in for project_individual.ProjectLayer.forward).
// boxes[p] = tl[3], start[3], end[3] in fine-grid indices (fvp_person_boxes).
template <int NV>
__global__ void __launch_bounds__(256)
k_project_individual(const float* __restrict__ heat_cl, const Cam* __restrict__ cams,
                     const int* __restrict__ frame_set, const int* __restrict__ person_frame,
                     const uint8_t* __restrict__ person_valid, const int* __restrict__ boxes,
                     const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ fz, int C,
                     FvpGeom g, float* __restrict__ cubes) {
  const int p = blockIdx.y;
  const int lv = blockIdx.x * 256 + threadIdx.x;
  const int nvox = C * C * C;
  if (lv >= nvox) return;
  const int J = g.J;
  const int lz = lv % C, ly = (lv / C) % C, lx = lv / (C * C);
  const int* bx = boxes + p * 9;
  const int gx_ = bx[0] + lx, gy_ = bx[1] + ly, gz_ = bx[2] + lz;
  bool in = (!person_valid || person_valid[p]);
  in = in && bx[3] < bx[6] && bx[4] < bx[7] && bx[5] < bx[8];   // empty window -> all zero (:125)
  in = in && gx_ >= bx[3] && gx_ < bx[6] && gy_ >= bx[4] && gy_ < bx[7] && gz_ >= bx[5] && gz_ < bx[8];
  float acc[4 * NV];
#pragma unroll
  for (int c = 0; c < 4 * NV; ++c) acc[c] = 0.0f;
  if (in) {
    const int b = person_frame[p];
    const float* frame = heat_cl + size_t(b) * g.V * g.H * g.W * (4 * NV);
    backproject_point<NV>(frame, cams + size_t(frame_set[b]) * g.V, g, fx[gx_], fy[gy_], fz[gz_], acc);
  }
#pragma unroll
  for (int c = 0; c < 4 * NV; ++c)
    if (c < J) cubes[(size_t(p) * J + c) * nvox + lv] = acc[c];
}

// ---------------------------------------------------------------------------------------------
// Orthographic maxima of a materialised cube: one workgroup per (person, joint), x-slabs
// streamed through LDS; yz keeps a running max in registers.  PER = (y,z) cells per thread, a power of two >= C*C/256
// (as a run-time bound on a 64-deep unrolled loop the 64 `i < per` predicates were kept as SGPR pairs: 78 spills, round 4).
template <int PER>
__global__ void __launch_bounds__(256)
k_triplane_max(const float* __restrict__ cubes, float* __restrict__ planes, int J, int C) {
  HIP_DYNAMIC_SHARED(float, slab)                     // [C][C+1]
  const int j = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  const int CC = C * C, ld = C + 1;
  const float* cube = cubes + (size_t(p) * J + j) * CC * C;
  float* pxy = planes + ((size_t(p) * 3 + 0) * J + j) * CC;
  float* pxz = planes + ((size_t(p) * 3 + 1) * J + j) * CC;
  float* pyz = planes + ((size_t(p) * 3 + 2) * J + j) * CC;
  float run[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) run[i] = -INFINITY;
  for (int x = 0; x < C; ++x) {
    __syncthreads();
    int ncell = CC;
    FVP_OPAQUE(ncell);                                // (the PER bounds tests stay in the loop: hoisted, each is an SGPR pair)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int cell = t + i * 256;
      if (cell < ncell) {
        const float v = cube[size_t(x) * CC + cell];
        slab[(cell / C) * ld + (cell % C)] = v;
        run[i] = fmaxf(run[i], v);
      }
    }
    __syncthreads();
    for (int r = t; r < 2 * C; r += 256) {
      if (r < C) {                                     // xy[x][y=r] = max_z
        float m = slab[r * ld];
        for (int z = 1; z < C; ++z) m = fmaxf(m, slab[r * ld + z]);
        pxy[x * C + r] = m;
      } else {                                         // xz[x][z] = max_y
        const int z = r - C;
        float m = slab[z];
        for (int y = 1; y < C; ++y) m = fmaxf(m, slab[y * ld + z]);
        pxz[x * C + z] = m;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int cell = t + i * 256;
    if (cell < CC) pyz[cell] = run[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Fused fast path: sample every voxel of the person's window and emit the three maxima
// without writing the cube.
//
// The gather is bound by the texture-addresser / L1 line rate (GRBM_TA_BUSY 95 % in the first
// version, which gave every lane a whole 64-byte pixel = 4 dwordx4 loads touching 64 different
// cache lines per instruction).  Here four consecutive lanes share one voxel: lane q of the quad
// loads channels 4q..4q+3 of each tap, so one dwordx4 instruction covers 16 voxels x 64
// contiguous bytes (4x fewer lines per instruction).  The projection arithmetic is shared inside
// the quad: lane q projects view q and the tap descriptors are broadcast with DPP quad_perm.
//
// Workgroup = (person, 256 (y,z) cells) x 4 lanes = 1024 threads; lanes of a wave: 16 consecutive
// z x 4 channel quads; loop over x inside the thread.
//   yz[y][z] = max_x : running max in registers, owned by this workgroup -> plain store
//   xy[x][y] = max_z : shuffle over the 16 z-lanes of a wave, then LDS across the row's waves
//   xz[x][z] = max_y : LDS over the workgroup's rows, then integer atomicMax across workgroups
//                      (values are clamped to [0,1] => non-negative => int order == float order;
//                      planes are pre-zeroed, so the result is order-independent and bit-equal
//                      to the materialised path)
// Workgroups are numbered so that all persons of one frame run on one XCD (block id mod 8 is the
// XCD): an XCD's L2 then serves one frame's heatmaps instead of all of them.
struct TapD {   // tap descriptor of one (voxel, view): 4 offsets, 4 weights, inside mask
  int off[4];
  float w[4];
  int inside;
};

template <int SRC>
__device__ __forceinline__ int quad_bcast_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, SRC * 0x55, 0xf, 0xf, false);   // quad_perm [SRC,SRC,SRC,SRC]
}
template <int SRC>
__device__ __forceinline__ TapD quad_bcast(const TapD& t) {
  TapD r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.off[k] = quad_bcast_i<SRC>(t.off[k]);
    r.w[k] = __int_as_float(quad_bcast_i<SRC>(__float_as_int(t.w[k])));
  }
  r.inside = quad_bcast_i<SRC>(t.inside);
  return r;
}

__device__ __forceinline__ TapD make_taps(const Cam& cm, const FvpGeom& g, float wx, float wy, float wz) {
  float gx, gy;
  project_norm(cm, g, wx, wy, wz, gx, gy);
  const Taps t = bilinear_taps(gx, gy, g.W, g.H);
  TapD d;
#pragma unroll
  for (int k = 0; k < 4; ++k) { d.off[k] = t.off[k]; d.w[k] = t.w[k]; }
  d.inside = t.inside;
  return d;
}

// acc[i] (+)= bilinear sample of channels ch0..ch0+3 (reference accumulation order: nw*w then fma)
__device__ __forceinline__ void sample4(const float* __restrict__ cl, int JP, int ch0, const TapD& t, bool first,
                                        float (&acc)[4]) {
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = (t.inside >> k) & 1;
    v[k] = *reinterpret_cast<const float4*>(cl + size_t(in ? t.off[k] : 0) * JP + ch0);
    if (!in) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float s[4] = {__fmul_rn(v[0].x, t.w[0]), __fmul_rn(v[0].y, t.w[0]), __fmul_rn(v[0].z, t.w[0]),
                __fmul_rn(v[0].w, t.w[0])};
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    s[0] = __fmaf_rn(v[k].x, t.w[k], s[0]);
    s[1] = __fmaf_rn(v[k].y, t.w[k], s[1]);
    s[2] = __fmaf_rn(v[k].z, t.w[k], s[2]);
    s[3] = __fmaf_rn(v[k].w, t.w[k], s[3]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = first ? s[i] : __fadd_rn(acc[i], s[i]);
}

// Whole-space cubes + fused z-max, quad-lane form (the default): 4 lanes per voxel, lane q
// gathers channels [16n + 4q, +4) of every tap, so the four lanes of a voxel read one contiguous
// 64-byte run per tap (16 cache lines per wave instruction instead of 64 -- the gather is bound by
// the texture-addresser line rate) and lane q computes the projection of view q for the quad
// (DPP broadcast).  Same per-channel arithmetic as k_project_whole (bit-equal cubes).
// the per-voxel body of the quad-lane form: mean over views of the bilinear samples of channels [16n + 4q, +4),
// clamped to [0,1] (shared by the whole-space kernel and the proposal-column kernel, so both give the same bits)
template <int NVL>
__device__ __forceinline__ void whole_point_quad(const float* __restrict__ frame, const Cam* __restrict__ cm,
                                                 const FvpGeom& g, int q, bool active, float wx, float wy, float wz,
                                                 float (&out)[NVL][4]) {
  const int JP = g.JP;
  const size_t view_stride = size_t(g.H) * g.W * JP;
  float acc[NVL][4];
#pragma unroll
  for (int n = 0; n < NVL; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[n][i] = 0.0f;
  TapD mine;
  mine.inside = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { mine.off[k] = 0; mine.w[k] = 0.0f; }
  if (active && q < g.V) mine = make_taps(cm[q], g, wx, wy, wz);
  auto add_view = [&](const TapD& tv, int v) {
#pragma unroll
    for (int n = 0; n < NVL; ++n) {
      const int ch0 = 16 * n + 4 * q;
      if (ch0 < JP) {
        if (tv.inside) sample4(frame + v * view_stride, JP, ch0, tv, v == 0, acc[n]);
        else if (v == 0) { acc[n][0] = acc[n][1] = acc[n][2] = acc[n][3] = 0.0f; }
      }
    }
  };
  { const TapD tv = quad_bcast<0>(mine); if (active) add_view(tv, 0); }
  if (g.V > 1) { const TapD tv = quad_bcast<1>(mine); if (active) add_view(tv, 1); }
  if (g.V > 2) { const TapD tv = quad_bcast<2>(mine); if (active) add_view(tv, 2); }
  if (g.V > 3) { const TapD tv = quad_bcast<3>(mine); if (active) add_view(tv, 3); }
  for (int v = 4; v < g.V; ++v)
    if (active) add_view(make_taps(cm[v], g, wx, wy, wz), v);
  const float nv = float(g.V);
#pragma unroll
  for (int n = 0; n < NVL; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[n][i] = clampf(__fdiv_rn(acc[n][i], nv), 0.0f, 1.0f);
}

template <int NVL>
__global__ void __launch_bounds__(1024)
k_project_whole_q(const float* __restrict__ heat_cl, const Cam* __restrict__ cams,
                  const int* __restrict__ frame_set, const float* __restrict__ ax, const float* __restrict__ ay,
                  const float* __restrict__ az, int X, int Y, int Z, int B, int nblk, FvpGeom g,
                  float* __restrict__ cubes, float* __restrict__ zmax) {
  __shared__ float sm[16 * NVL][256];
  const int cpb = 256 / Z;
  // 1-D grid of B * nblk workgroups.  Consecutive workgroup ids go round-robin over the 8 XCDs (each with
  // its own L2), so with B % 8 == 0 frame f is pinned to XCD f % 8: an XCD's L2 then holds the heatmaps of
  // one frame at a time instead of all B (HBM-side fetch was 3.5x the algorithmic bytes without it).
  int b, bxi;
  if (B % 8 == 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    b = xcd + 8 * (j / nblk);
    bxi = j % nblk;
  } else {
    b = blockIdx.x / nblk;
    bxi = blockIdx.x % nblk;
  }
  const int t = threadIdx.x, q = t & 3, vl = t >> 2;           // vl = voxel inside the workgroup
  const int cl_ = vl / Z, z = vl - cl_ * Z;
  const int col = bxi * cpb + cl_;
  const int ncol = X * Y;
  const bool active = cl_ < cpb && col < ncol;
  const int J = g.J, JP = g.JP;
  const size_t view_stride = size_t(g.H) * g.W * JP;
  const float* frame = heat_cl + size_t(b) * g.V * view_stride;
  const Cam* cm = cams + size_t(frame_set[b]) * g.V;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  if (active) {
    const int x = col / Y, y = col - x * Y;
    wx = ax[x];
    wy = ay[y];
    wz = az[z];
  }
  float val[NVL][4];
  whole_point_quad<NVL>(frame, cm, g, q, active, wx, wy, wz, val);
  const size_t vox = size_t(col) * Z + z;
  const size_t nvox = size_t(ncol) * Z;
#pragma unroll
  for (int n = 0; n < NVL; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * n + 4 * q + i;
      const float v = val[n][i];
      if (zmax) sm[c][vl] = active ? v : 0.0f;
      if (cubes && active && c < J) cubes[(size_t(b) * J + c) * nvox + vox] = v;
    }
  if (zmax) {
    __syncthreads();
    for (int item = t; item < cpb * J; item += 1024) {
      const int c = item / cpb, k = item - c * cpb;
      const int cc = bxi * cpb + k;
      if (cc < ncol) {
        float m = sm[c][k * Z];
        for (int zz = 1; zz < Z; ++zz) m = fmaxf(m, sm[c][k * Z + zz]);
        zmax[(size_t(b) * J + c) * ncol + cc] = m;
      }
    }
  }
}

// Proposal z-columns only (human_detection_net.py:92-93 gathers N columns of the cubes per frame and nothing else
// of them is used by the fused forward): feat1d[b*N + k][c][z] = cubes[b][c][flat[b][k]][z], computed by the very
// device function of k_project_whole_q (same bits as the materialised cubes), 61 MB of cube writes per 8 frames never
// happen.  Workgroup = one proposal column: Z voxels x 4 lanes.
template <int NVL>
__global__ void __launch_bounds__(1024)
k_project_columns_q(const float* __restrict__ heat_cl, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                    const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az, int Y,
                    int Z, int ncol, int N, FvpGeom g, const long long* __restrict__ flat, float* __restrict__ feat1d) {
  const int pi = blockIdx.x, b = pi / N;
  const int t = threadIdx.x, q = t & 3, z = t >> 2;
  const long long col = flat[pi];
  const bool active = z < Z && col >= 0 && col < ncol;
  const int J = g.J;
  const size_t view_stride = size_t(g.H) * g.W * g.JP;
  const float* frame = heat_cl + size_t(b) * g.V * view_stride;
  const Cam* cm = cams + size_t(frame_set[b]) * g.V;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  if (active) {
    const int x = int(col) / Y, y = int(col) - x * Y;
    wx = ax[x];
    wy = ay[y];
    wz = az[z];
  }
  float val[NVL][4];
  whole_point_quad<NVL>(frame, cm, g, q, active, wx, wy, wz, val);
#pragma unroll
  for (int n = 0; n < NVL; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * n + 4 * q + i;
      if (z < Z && c < J) feat1d[(size_t(pi) * J + c) * Z + z] = active ? val[n][i] : 0.0f;
    }
}

#if FVP_DIAG   // the round-1 gather form of the fused projection: diagnostics build only (FVP_TRIPLANE_GATHER=1)
template <int NVL>   // channel quads per lane: ceil(JP/16)
__global__ void __launch_bounds__(1024)
k_project_triplane(const float* __restrict__ heat_cl, const Cam* __restrict__ cams, const int* __restrict__ frame_set,
                   const int* __restrict__ person_frame, const uint8_t* __restrict__ person_valid,
                   const int* __restrict__ boxes, const float* __restrict__ fx, const float* __restrict__ fy,
                   const float* __restrict__ fz, int C, int nP, int chunks, int ppf, FvpGeom g,
                   float* __restrict__ planes) {
  __shared__ float sm_xz[4 * NVL * 4][256];       // [channel][cell]
  __shared__ float sm_xy[16][4 * NVL * 4];        // [wave][channel]
  // ---- block -> (person, chunk), frame-major per XCD when the frame count allows it
  int p, chunk;
  {
    const int id = blockIdx.x;
    const int bpf = ppf * chunks;                 // blocks per frame
    const int nframes = nP / ppf;
    if (nframes % 8 == 0) {
      const int xcd = id & 7, j = id >> 3;
      const int frame = xcd + 8 * (j / bpf), r = j % bpf;
      p = frame * ppf + r / chunks;
      chunk = r % chunks;
    } else {
      p = id / chunks;
      chunk = id % chunks;
    }
  }
  if (person_valid && !person_valid[p]) return;
  const int* bx = boxes + p * 9;
  const int tl0 = bx[0], tl1 = bx[1], tl2 = bx[2];
  const int s0 = bx[3], s1 = bx[4], s2 = bx[5], e0 = bx[6], e1 = bx[7], e2 = bx[8];
  if (s0 >= e0 || s1 >= e1 || s2 >= e2) return;
  const int t = threadIdx.x, q = t & 3, lane = t & 63, wave = t >> 6;
  const int J = g.J, JP = g.JP, CC = C * C;
  const int rows = 256 / C > 0 ? 256 / C : 1;
  const int cell_l = t >> 2;                       // 0..255 within the workgroup
  const int cell = chunk * 256 + cell_l;
  const int y = cell / C, z = cell - y * C;
  const int y_first = (chunk * 256) / C;
  if (tl1 + y_first >= e1 || tl1 + y_first + rows - 1 < s1) return;   // chunk outside the y window
  const int gy_ = tl1 + y, gz_ = tl2 + z;
  const bool yz_in = y < C && gy_ >= s1 && gy_ < e1 && gz_ >= s2 && gz_ < e2;
  const int b = person_frame[p];
  const size_t view_stride = size_t(g.H) * g.W * JP;
  const float* frame = heat_cl + size_t(b) * g.V * view_stride;
  const Cam* cm = cams + size_t(frame_set[b]) * g.V;
  const float wy = yz_in ? fy[gy_] : 0.0f, wz = yz_in ? fz[gz_] : 0.0f;
  float* pxy = planes + (size_t(p) * 3 + 0) * J * CC;
  float* pxz = planes + (size_t(p) * 3 + 1) * J * CC;
  float* pyz = planes + (size_t(p) * 3 + 2) * J * CC;
  const int wpr = C >= 16 ? C / 16 : 1;           // waves per y row
  float run[NVL][4];
#pragma unroll
  for (int n = 0; n < NVL; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) run[n][i] = 0.0f;
  const float nv = float(g.V);
  const int lx0 = s0 - tl0, lx1 = e0 - tl0;
  for (int lx = lx0; lx < lx1; ++lx) {
    const float wx = fx[tl0 + lx];
    float acc[NVL][4];
#pragma unroll
    for (int n = 0; n < NVL; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[n][i] = 0.0f;
    // lane q projects view q; descriptors are shared inside the quad by DPP
    TapD mine;
    mine.inside = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { mine.off[k] = 0; mine.w[k] = 0.0f; }
    if (yz_in && q < g.V) mine = make_taps(cm[q], g, wx, wy, wz);
    auto add_view = [&](const TapD& tv, int v) {
#pragma unroll
      for (int n = 0; n < NVL; ++n) {
        const int ch0 = 16 * n + 4 * q;
        if (ch0 < JP) {
          if (tv.inside) sample4(frame + v * view_stride, JP, ch0, tv, v == 0, acc[n]);
          else if (v == 0) { acc[n][0] = acc[n][1] = acc[n][2] = acc[n][3] = 0.0f; }
        }
      }
    };
    { const TapD tv = quad_bcast<0>(mine); if (yz_in) add_view(tv, 0); }
    if (g.V > 1) { const TapD tv = quad_bcast<1>(mine); if (yz_in) add_view(tv, 1); }
    if (g.V > 2) { const TapD tv = quad_bcast<2>(mine); if (yz_in) add_view(tv, 2); }
    if (g.V > 3) { const TapD tv = quad_bcast<3>(mine); if (yz_in) add_view(tv, 3); }
    for (int v = 4; v < g.V; ++v)
      if (yz_in) add_view(make_taps(cm[v], g, wx, wy, wz), v);
#pragma unroll
    for (int n = 0; n < NVL; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[n][i] = clampf(__fdiv_rn(acc[n][i], nv), 0.0f, 1.0f);
        run[n][i] = fmaxf(run[n][i], acc[n][i]);
      }
    // ---- reductions
    __syncthreads();                               // previous iteration's LDS readers are done
#pragma unroll
    for (int n = 0; n < NVL; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 16 * n + 4 * q + i;
        sm_xz[c][cell_l] = acc[n][i];
        float m = acc[n][i];
        const int zw = C < 16 ? C : 16;            // z lanes of this row inside the wave
        for (int o = (zw >> 1) * 4; o >= 4; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (C >= 16) { if ((lane >> 2) == 0) sm_xy[wave][c] = m; }
        else if (((lane >> 2) & (zw - 1)) == 0 && c < J && y < C && m > 0.0f) pxy[size_t(c) * CC + lx * C + y] = m;
      }
    __syncthreads();
    if (C >= 16) {                                 // xy: combine the waves of each row
      const int nitem = rows * J;
      if (t < nitem) {
        const int r = t / J, c = t - r * J;
        float m = sm_xy[r * wpr][c];
        for (int k = 1; k < wpr; ++k) m = fmaxf(m, sm_xy[r * wpr + k][c]);
        const int yy = y_first + r;
        if (yy < C && m > 0.0f) pxy[size_t(c) * CC + lx * C + yy] = m;
      }
    }
    for (int item = t; item < J * C; item += 1024) {   // xz: max over this workgroup's rows
      const int c = item / C, zz = item - c * C;
      float m = sm_xz[c][zz];
      for (int r = 1; r < rows; ++r) m = fmaxf(m, sm_xz[c][r * C + zz]);
      if (m > 0.0f) {
        if (chunks > 1) atomicMax(reinterpret_cast<int*>(&pxz[size_t(c) * CC + lx * C + zz]), __float_as_int(m));
        else pxz[size_t(c) * CC + lx * C + zz] = m;
      }
    }
  }
  if (y < C) {
#pragma unroll
    for (int n = 0; n < NVL; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 16 * n + 4 * q + i;
        if (c < J && run[n][i] > 0.0f) pyz[size_t(c) * CC + y * C + z] = run[n][i];
      }
  }
}

#endif  // FVP_DIAG

}  // namespace fvp
#include "fvp_project_lds.h"
namespace fvp {

// z-max of materialised cubes: one thread per (b,j,x,y) column.
__global__ void __launch_bounds__(256) k_zmax(const float* __restrict__ cubes, float* __restrict__ zmax, long n, int Z) {
  const long i = long(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const float* c = cubes + i * Z;
  float m = c[0];
  for (int z = 1; z < Z; ++z) m = fmaxf(m, c[z]);
  zmax[i] = m;
}

// ---------------------------------------------------------------------------------------------
// fvp_person_boxes: integer window arithmetic of project_individual.py:110-121.
__global__ void __launch_bounds__(64)
k_person_boxes(const float* __restrict__ centers, int n, const float* __restrict__ consts, int f0, int f1, int f2,
               int c0, int c1, int c2, int* __restrict__ boxes, float* __restrict__ offset) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* pc = centers + size_t(i) * 7;
  const int fine[3] = {f0, f1, f2}, cube[3] = {c0, c1, c2};
  int tl[3], m[3];
  for (int a = 0; a < 3; ++a) {
    // round(c*scale + bias): two roundings then half-to-even, .int() truncation (exact here)
    const float v = __fadd_rn(__fmul_rn(pc[a], consts[a]), consts[3 + a]);
    tl[a] = int(rintf(v));
    // offset = tl / (fine-1) * whole - whole/2 + ind/2   (left to right, :111)
    const float whole = consts[6 + a], ind = consts[9 + a];
    float o = __fmul_rn(__fdiv_rn(float(tl[a]), float(fine[a] - 1)), whole);
    o = __fadd_rn(__fsub_rn(o, __fdiv_rn(whole, 2.0f)), __fdiv_rn(ind, 2.0f));
    offset[size_t(i) * 3 + a] = o;
  }
  for (int a = 0; a < 2; ++a) {
    // ((1 - bbox) / 2 * (C - 1)).int(), negatives -> 0 (:114-115); z margin is 0 (:117)
    const float r = __fmul_rn(__fdiv_rn(__fsub_rn(1.0f, pc[5 + a]), 2.0f), float(cube[a] - 1));
    m[a] = int(r);
    if (m[a] < 0) m[a] = 0;
  }
  m[2] = 0;
  for (int a = 0; a < 3; ++a) {
    const int s = tl[a] + m[a], e = tl[a] + cube[a] - m[a];
    boxes[i * 9 + a] = tl[a];
    boxes[i * 9 + 3 + a] = s >= 0 ? s : 0;
    boxes[i * 9 + 6 + a] = e <= fine[a] ? e : fine[a];
  }
}

// fvp_plane_live_rows: the rows of a person's three planes that the projection can write (rows of the x-y and x-z planes
// are x, rows of the y-z plane are y), cube-relative: {start - tl, end - tl} clamped to [0, C]; an empty window in any axis
// leaves all three planes at the caller's zero fill: {0, 0}.
__global__ void __launch_bounds__(64)
k_plane_live_rows(const int* __restrict__ boxes, int n, int C, int* __restrict__ live_rows) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int* b = boxes + size_t(i) * 9;
  const bool empty = b[3] >= b[6] || b[4] >= b[7] || b[5] >= b[8];
  int lo[2], hi[2];
  for (int a = 0; a < 2; ++a) {
    const int r0 = b[3 + a] - b[a], r1 = b[6 + a] - b[a];
    lo[a] = empty || r0 < 0 ? 0 : r0 > C ? C : r0;
    hi[a] = empty || r1 < 0 ? 0 : r1 > C ? C : r1;
  }
  int* o = live_rows + size_t(i) * 6;
  o[0] = lo[0]; o[1] = hi[0];
  o[2] = lo[0]; o[3] = hi[0];
  o[4] = lo[1]; o[5] = hi[1];
}

}  // namespace fvp

// =============================================================================================
// C ABI
// =============================================================================================
using namespace fvp;

#define FVP_NV_SWITCH(nv, CALL)     \
  switch (nv) {                     \
    case 1: { CALL(1); } break;     \
    case 2: { CALL(2); } break;     \
    case 3: { CALL(3); } break;     \
    case 4: { CALL(4); } break;     \
    case 5: { CALL(5); } break;     \
    case 6: { CALL(6); } break;     \
    case 7: { CALL(7); } break;     \
    case 8: { CALL(8); } break;     \
    default: return FVP_ELIMIT;     \
  }

static int check_geom(const FvpGeom* g) {
  if (!g) return FVP_EINVAL;
  if (g->V < 1 || g->V > FVP_MAX_VIEWS || g->J < 1 || g->J > FVP_MAX_JOINTS) return FVP_ELIMIT;
  if (g->JP != 4 * ((g->J + 3) / 4) || g->W < 2 || g->H < 2) return FVP_EINVAL;
  return 0;
}

extern "C" int fvp_heatmaps_to_cl(const float* heat, float* heat_cl, int B, const FvpGeom* g, fvp_stream_t s) {
  FVP_REQUIRE(heat && heat_cl && B >= 0);
  if (int e = check_geom(g)) return e;
  if (B == 0) return 0;
  const int HW = g->H * g->W;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
#define CALL(NV)                                                                                             \
  auto k = &k_heat_to_cl<NV>;                                                                                \
  hipLaunchKernelGGL(k, dim3(ceil_div(HW, 256), B * g->V), dim3(256), 0, as_stream(s), heat, heat_cl, g->J, HW);
  FVP_NV_SWITCH(g->JP / 4, CALL)
#undef CALL
  return launch_status();
}

extern "C" int fvp_sample_grid(const float* ax, const float* ay, const float* az, int nx, int ny, int nz,
                               const float* cams, const FvpGeom* g, float* grid, fvp_stream_t s) {
  FVP_REQUIRE(ax && ay && az && cams && grid && nx > 0 && ny > 0 && nz > 0);
  if (int e = check_geom(g)) return e;
  const int n = nx * ny * nz;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_sample_grid, dim3(ceil_div(n, 256), g->V), dim3(256), 0, as_stream(s), ax, ay, az, nx, ny,
                     nz, reinterpret_cast<const Cam*>(cams), *g, grid);
  return launch_status();
}

extern "C" int fvp_project_whole(const float* heat_cl, const float* cams, const int32_t* frame_set,
                                 const float* ax, const float* ay, const float* az, int X, int Y, int Z, int B,
                                 const FvpGeom* g, float* cubes, float* zmax, fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && ax && ay && az && (cubes || zmax) && X > 0 && Y > 0 && Z > 0);
  if (int e = check_geom(g)) return e;
  FVP_LIMIT(Z <= 256);
  if (B == 0) return 0;
  const int cpb = 256 / Z;
  ProfScope ps(FVP_K_PROJECT_WHOLE, as_stream(s));
  static const bool no_quad = fvp::diag_env("FVP_WHOLE_NO_QUAD") != nullptr;
  const int nvl = ceil_div(g->JP, 16);
  if (!no_quad && nvl <= 2) {
    const int nblk = ceil_div(X * Y, cpb);
    if (nvl == 1)
      hipLaunchKernelGGL(k_project_whole_q<1>, dim3(nblk * B), dim3(1024), 0, as_stream(s), heat_cl,
                         reinterpret_cast<const Cam*>(cams), frame_set, ax, ay, az, X, Y, Z, B, nblk, *g, cubes, zmax);
    else
      hipLaunchKernelGGL(k_project_whole_q<2>, dim3(nblk * B), dim3(1024), 0, as_stream(s), heat_cl,
                         reinterpret_cast<const Cam*>(cams), frame_set, ax, ay, az, X, Y, Z, B, nblk, *g, cubes, zmax);
    return launch_status();
  }
#define CALL(NV)                                                                                              \
  auto k = &k_project_whole<NV>;                                                                              \
  hipLaunchKernelGGL(k, dim3(ceil_div(X * Y, cpb), B), dim3(256), 0, as_stream(s), heat_cl,                   \
                     reinterpret_cast<const Cam*>(cams), frame_set, ax, ay, az, X, Y, Z, *g, cubes, zmax);
  FVP_NV_SWITCH(g->JP / 4, CALL)
#undef CALL
  return launch_status();
}

extern "C" int fvp_joint_evidence(const float* heat_cl, const float* cams, const int32_t* frame_set,
                                  const float* fused_poses, int B, int N, const FvpGeom* g, float* views,
                                  float* joint_conf, fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && fused_poses && (views || joint_conf) && B >= 0 && N >= 0);
  if (int e = check_geom(g)) return e;
  FVP_LIMIT(size_t(B) * N * g->J * g->V < (size_t(1) << 29));   // item and element indices stay inside int32
  if (B == 0 || N == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_joint_evidence, dim3(ceil_div(B * N * g->J, 256)), dim3(256), 0, as_stream(s), heat_cl,
                     reinterpret_cast<const Cam*>(cams), frame_set, fused_poses, B, N, *g, views, joint_conf);
  return launch_status();
}

extern "C" int fvp_joint_visibility(const float* fused_poses, const float* cams, const int32_t* frame_set,
                                    const int32_t* ids, const float* views, int B, int V, int N, int J,
                                    const int32_t* prims, const float* radius_mm, int L, float guard_mm, int Hs, int Ws,
                                    int32_t* occluder, float* vis_conf, int32_t* vis_count, fvp_stream_t s) {
  FVP_REQUIRE(fused_poses && cams && frame_set && ((prims && radius_mm) || L <= 0));
  FVP_REQUIRE((occluder || vis_conf || vis_count) && (views || (!vis_conf && !vis_count)));
  FVP_REQUIRE(B >= 0 && V >= 1 && N >= 1 && J >= 1 && Hs >= 1 && Ws >= 1 && L >= 0);
  FVP_REQUIRE(guard_mm >= 0.0f && guard_mm <= FLT_MAX);          // a NaN fails
  FVP_LIMIT(N <= FVP_VIS_MAX_PEOPLE && J <= FVP_MAX_JOINTS && V <= FVP_MAX_VIEWS && L <= FVP_VIS_MAX_PRIMS);
  VisPrims prm;
  prm.n = L;
  for (int l = 0; l < FVP_VIS_MAX_PRIMS; ++l) {
    prm.ik[l] = 0;
    prm.r[l] = 0.0f;
    if (l >= L) continue;
    const int i = prims[2 * l], k = prims[2 * l + 1];
    FVP_REQUIRE(i >= 0 && i < J && k >= 0 && k < J && radius_mm[l] > 0.0f && radius_mm[l] <= FLT_MAX);
    prm.ik[l] = i | (k << 8);
    prm.r[l] = radius_mm[l];
  }
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_joint_visibility, dim3(B * N), dim3(256), 0, as_stream(s), fused_poses,
                     reinterpret_cast<const Cam*>(cams), frame_set, ids, views, V, N, J, prm, guard_mm, float(Ws - 1),
                     float(Hs - 1), occluder, vis_conf, vis_count);
  return launch_status();
}

extern "C" int fvp_triangulate_joints(const float* heat_cl, const float* cams, int nsets, const int32_t* frame_set,
                                      const float* fused_poses, const int32_t* ids, const int32_t* occluder, int B, int N,
                                      const FvpGeom* g, int radius, float min_peak, int undistort_iters, int min_views,
                                      float min_det, float reject_px, float* tri_poses, int32_t* tri_count,
                                      float* tri_stats, float* obs, int32_t* view_state, float* cam_resid,
                                      int32_t* cam_count, fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && fused_poses);
  FVP_REQUIRE(tri_poses || tri_count || tri_stats || obs || view_state || cam_resid || cam_count);
  FVP_REQUIRE((obs && view_state) || (!cam_resid && !cam_count));
  FVP_REQUIRE(B >= 0 && N >= 1 && nsets >= 1 && radius >= 1 && min_views >= 2 && undistort_iters >= 0);
  FVP_REQUIRE(fabsf(min_peak) <= FLT_MAX && fabsf(min_det) <= FLT_MAX && fabsf(reject_px) <= FLT_MAX);   // a NaN fails
  if (int e = check_geom(g)) return e;
  FVP_LIMIT(radius <= FVP_TRI_MAX_RADIUS && undistort_iters <= 16);
  // heat-map cell -> pixel of the original image: the inverse of rt and of the heat scale, in double, rounded once
  const double r0 = g->rt[0], r1 = g->rt[1], r2 = g->rt[2], r3 = g->rt[3], r4 = g->rt[4], r5 = g->rt[5];
  const double sx = double(g->img_w) / double(g->hm_w), sy = double(g->img_h) / double(g->hm_h);
  const double det = r0 * r4 - r1 * r3;
  TriParams tp;
  tp.inv[0] = float(r4 / det * sx);
  tp.inv[1] = float(-r1 / det * sy);
  tp.inv[2] = float((r1 * r5 - r4 * r2) / det);
  tp.inv[3] = float(-r3 / det * sx);
  tp.inv[4] = float(r0 / det * sy);
  tp.inv[5] = float((r3 * r2 - r0 * r5) / det);
  for (int i = 0; i < 6; ++i) FVP_REQUIRE(fabsf(tp.inv[i]) <= FLT_MAX);      // a singular rt, a zero heat-map size
  tp.radius = radius;
  tp.iters = undistort_iters;
  tp.min_views = min_views;
  tp.nsets = nsets;
  tp.min_peak = min_peak;
  tp.reject_px = reject_px;
  tp.min_det = double(min_det);
  if (B == 0) return 0;
  const bool per_camera = cam_resid || cam_count;
  ProfScope ps(FVP_K_OTHER, as_stream(s), 0.0, per_camera ? 2 : 1);
  hipLaunchKernelGGL(k_triangulate_joints, dim3(B * N), dim3(256), 0, as_stream(s), heat_cl,
                     reinterpret_cast<const Cam*>(cams), frame_set, fused_poses, ids, occluder, N, *g, tp, tri_poses,
                     tri_count, tri_stats, obs, view_state);
  if (per_camera)
    hipLaunchKernelGGL(k_view_residual, dim3(B * g->V), dim3(256), 0, as_stream(s), obs, view_state, N * g->J, cam_resid,
                       cam_count);
  return launch_status();
}

extern "C" int fvp_camera_refit_accumulate(const float* points, const float* obs, const int32_t* view_state,
                                           const float* cams, int nsets, const int32_t* frame_set, int B, int V, int N, int J,
                                           int undistort_iters, float huber_px, float decay, double* acc, fvp_stream_t s) {
  FVP_REQUIRE(points && obs && view_state && cams && frame_set && acc);
  FVP_REQUIRE(B >= 0 && V >= 1 && N >= 1 && J >= 1 && nsets >= 1 && undistort_iters >= 0);
  FVP_REQUIRE(fabsf(huber_px) <= FLT_MAX && decay >= 0.0f && decay <= 1.0f);                             // a NaN fails
  FVP_LIMIT(V <= FVP_MAX_VIEWS && J <= FVP_MAX_JOINTS && undistort_iters <= 16);
  FVP_LIMIT(static_cast<long long>(B) * N * J <= INT_MAX && static_cast<long long>(nsets) * V <= INT_MAX);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s), 0.0, 1);
  hipLaunchKernelGGL(k_camera_refit_accumulate, dim3(nsets * V), dim3(256), 0, as_stream(s), points, obs, view_state,
                     reinterpret_cast<const Cam*>(cams), frame_set, B, V, N * J, undistort_iters, huber_px, decay, acc);
  return launch_status();
}

extern "C" int fvp_camera_refit_solve(const double* acc, const float* cams_in, int nsets, int V, int min_obs, float lambda,
                                      float min_pivot, float max_angle_rad, float max_shift_mm, float* cams_out,
                                      float* cal_stats, int32_t* cal_state, fvp_stream_t s) {
  FVP_REQUIRE(acc && cams_in && cams_out && cams_out != cams_in);
  FVP_REQUIRE(nsets >= 1 && V >= 1 && min_obs >= 6);
  FVP_REQUIRE(lambda >= 0.0f && lambda <= FLT_MAX);                                                      // a NaN fails
  FVP_REQUIRE(min_pivot > 0.0f && min_pivot <= FLT_MAX && max_angle_rad > 0.0f && max_angle_rad <= FLT_MAX);
  FVP_REQUIRE(max_shift_mm > 0.0f && max_shift_mm <= FLT_MAX);
  FVP_LIMIT(V <= FVP_MAX_VIEWS && static_cast<long long>(nsets) * V <= INT_MAX);
  ProfScope ps(FVP_K_OTHER, as_stream(s), 0.0, 1);
  hipLaunchKernelGGL(k_camera_refit_solve, dim3(ceil_div(nsets * V, 64)), dim3(64), 0, as_stream(s), acc,
                     reinterpret_cast<const Cam*>(cams_in), nsets * V, min_obs, double(lambda), double(min_pivot),
                     double(max_angle_rad), double(max_shift_mm), reinterpret_cast<Cam*>(cams_out), cal_stats, cal_state);
  return launch_status();
}

extern "C" int fvp_project_columns(const float* heat_cl, const float* cams, const int32_t* frame_set, const float* ax,
                                   const float* ay, const float* az, int X, int Y, int Z, int B, const FvpGeom* g,
                                   const int64_t* flat, int N, float* feat1d, fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && ax && ay && az && flat && feat1d && X > 0 && Y > 0 && Z > 0 && N > 0);
  if (int e = check_geom(g)) return e;
  FVP_LIMIT(Z <= 256 && g->JP <= 32);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_PROJECT_WHOLE, as_stream(s));
  const int threads = ceil_div(4 * Z, 64) * 64;
  if (g->JP <= 16)
    hipLaunchKernelGGL(k_project_columns_q<1>, dim3(B * N), dim3(threads), 0, as_stream(s), heat_cl,
                       reinterpret_cast<const Cam*>(cams), frame_set, ax, ay, az, Y, Z, X * Y, N, *g,
                       reinterpret_cast<const long long*>(flat), feat1d);
  else
    hipLaunchKernelGGL(k_project_columns_q<2>, dim3(B * N), dim3(threads), 0, as_stream(s), heat_cl,
                       reinterpret_cast<const Cam*>(cams), frame_set, ax, ay, az, Y, Z, X * Y, N, *g,
                       reinterpret_cast<const long long*>(flat), feat1d);
  return launch_status();
}

extern "C" int fvp_zmax(const float* cubes, float* zmax, long n, int Z, fvp_stream_t s) {
  FVP_REQUIRE(cubes && zmax && n >= 0 && Z > 0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_zmax, dim3(unsigned((n + 255) / 256)), dim3(256), 0, as_stream(s), cubes, zmax, n, Z);
  return launch_status();
}

extern "C" int fvp_person_boxes(const float* centers, int n, const float* consts, const int32_t* fine_cube,
                                int32_t* boxes, float* offset, fvp_stream_t s) {
  FVP_REQUIRE(centers && consts && fine_cube && boxes && offset && n >= 0);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_person_boxes, dim3(ceil_div(n, 64)), dim3(64), 0, as_stream(s), centers, n, consts,
                     fine_cube[0], fine_cube[1], fine_cube[2], fine_cube[3], fine_cube[4], fine_cube[5], boxes,
                     offset);
  return launch_status();
}

extern "C" int fvp_plane_live_rows(const int32_t* boxes, int nP, int C, int32_t* live_rows, fvp_stream_t s) {
  FVP_REQUIRE(boxes && live_rows && nP >= 0 && C > 0);
  if (nP == 0) return 0;
  hipLaunchKernelGGL(k_plane_live_rows, dim3(ceil_div(nP, 64)), dim3(64), 0, as_stream(s), boxes, nP, C, live_rows);
  return launch_status();
}

static int check_cube(int C) {
  if (C < 4 || C > 256 || (C & (C - 1)) != 0) return FVP_ELIMIT;   // power of two (row segments)
  return 0;
}

extern "C" int fvp_project_individual(const float* heat_cl, const float* cams, const int32_t* frame_set,
                                      const int32_t* person_frame, const uint8_t* person_valid,
                                      const int32_t* boxes, const float* fx, const float* fy, const float* fz,
                                      const int32_t* fine, int C, int nP, const FvpGeom* g, float* cubes,
                                      fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && person_frame && boxes && fx && fy && fz && cubes && nP >= 0);
  (void)fine;
  if (int e = check_geom(g)) return e;
  if (int e = check_cube(C)) return e;
  if (nP == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
#define CALL(NV)                                                                                                 \
  auto k = &k_project_individual<NV>;                                                                            \
  hipLaunchKernelGGL(k, dim3(ceil_div(C * C * C, 256), nP), dim3(256), 0, as_stream(s), heat_cl,                 \
                     reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, fx, fy, fz, \
                     C, *g, cubes);
  FVP_NV_SWITCH(g->JP / 4, CALL)
#undef CALL
  return launch_status();
}

extern "C" int fvp_triplane_max(const float* cubes, float* planes, int nP, int J, int C, fvp_stream_t s) {
  FVP_REQUIRE(cubes && planes && nP >= 0 && J > 0);
  if (int e = check_cube(C)) return e;
  FVP_LIMIT(C <= 128);
  if (nP == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  const int per = (C * C + 255) / 256;                 // <= 64 for C <= 128
  const dim3 grid(J, nP);
  const size_t lds = size_t(C) * (C + 1) * sizeof(float);
#define FVP_TRIMAX(PER_) hipLaunchKernelGGL(k_triplane_max<PER_>, grid, dim3(256), lds, as_stream(s), cubes, planes, J, C)
  if (per <= 1) FVP_TRIMAX(1);
  else if (per <= 4) FVP_TRIMAX(4);
  else if (per <= 16) FVP_TRIMAX(16);
  else FVP_TRIMAX(64);
#undef FVP_TRIMAX
  return launch_status();
}

// y segments per x strip of the owned fused projection (k_project_triplane_own): a shape rule, nothing read from the
// device.  The grid is ceil(C / 4) strips x ny x nP workgroups, of which a window of w x h fine voxels uses
// ceil(w / 4) x min(ny, ceil(h / 4)).  Measured (profiles/triplane_owned.txt; us per launch, block form 339-341 / Shelf 480 /
// Campus 152): the kernel lives on many small workgroups per CU - whole strips (ny = 1) take 629 us (Shelf 788), ny = 2
// 339-348 (534, 225), ny = 4 350 (499, 148), ny = 8 345-350 (475, 147), and one y block per workgroup (ny = C / 4 = 16)
// 327-329 (460, 144-146): the only setting below the block form on all three, so the rule is a function of C alone.  (Coarser
// segments would let a workgroup store its x-z cells without atomics; the imbalance of long strips costs more than that.
// Coarser counts are reachable through FVP_TRI_NY in the diagnostics build only.)
static int tri_owned_ny(int C) { return ceil_div(C, kBY); }

extern "C" int fvp_project_individual_triplane(const float* heat_cl, const float* cams, const int32_t* frame_set,
                                               const int32_t* person_frame, const uint8_t* person_valid,
                                               const int32_t* boxes, const float* fx, const float* fy,
                                               const float* fz, const int32_t* fine, int C, int nP, const FvpGeom* g,
                                               float* planes, int persons_per_frame, const float* fine_grid,
                                               fvp_stream_t s) {
  FVP_REQUIRE(heat_cl && cams && frame_set && person_frame && boxes && fx && fy && fz && planes && nP >= 0);
  FVP_REQUIRE(!fine_grid || fine);
  if (int e = check_geom(g)) return e;
  if (int e = check_cube(C)) return e;
  if (nP == 0) return 0;
  // persons_per_frame > 0 promises person p belongs to frame p / persons_per_frame (used only to
  // place the workgroups of one frame on one XCD); 0 = unknown
  const int ppf = (persons_per_frame > 0 && nP % persons_per_frame == 0) ? persons_per_frame : nP;
  [[maybe_unused]] const int chunks = ceil_div(C * C, 256);      // (the diagnostics build's gather form)
  const int nvl = ceil_div(g->JP, 16);
  ProfScope ps(FVP_K_PROJECT_TRIPLANE, as_stream(s));
  // The shipped forms for every joint count (JP <= 32) are UNSTAGED: the owned form k_project_triplane_own wherever its LDS
  // cells fit (below: Panoptic 339-341 -> 327-329 us, Shelf 480 -> 460-461 us, Campus 152 -> 144-146 us against the block
  // form, same bits), else the compact-block kernel k_project_triplane_blk (round 4: Panoptic 494 -> 348 us, Shelf 709 ->
  // 592 us, Campus 161 -> 158 us against the LDS-staged forms, same bits; lanes whose channel quad lies beyond JP idle, so
  // miniature joint counts run them too).  The LDS-staged quad / lane-per-voxel forms
  // and the round-1 gather form exist in the diagnostics build only (round 6), behind FVP_TRIPLANE_STAGED / _LANE /
  // _QUAD / _GATHER; they give the same bits (tests/test_emu_kernels.py, tools/gpu_switch_matrix.sh).
  const int F0 = fine_grid ? fine[0] : 0, F1 = fine_grid ? fine[1] : 0, F2 = fine_grid ? fine[2] : 0;
  const int nby = ceil_div(C, kBY);
#if FVP_DIAG
  const int nbx = ceil_div(C, kBX);
  static const bool gather = fvp::diag_env("FVP_TRIPLANE_GATHER") != nullptr;
  // FVP_TRIPLANE_QUAD=1: the round-2 form of the LDS-staged kernel (four lanes per voxel) instead of one lane per voxel
  const bool quad_form = fvp::diag_env("FVP_TRIPLANE_QUAD") != nullptr;            // read per call: tests switch it
  // diagnostics (wrong results): 1 no sampling, 2 no tile DMA, 4 no plane maxima, 8 no global-gather fallback
  static const int tri_ablate_env = fvp::diag_env("FVP_TRI_ABLATE") ? atoi(fvp::diag_env("FVP_TRI_ABLATE")) : 0;
  // bit 16 (NOT a diagnostic: results are identical either way): rectangles that fit the two tiles together are
  // staged across both when their turn comes instead of being gathered from global memory.  On for the
  // lane-per-voxel form (its gather reads 64 lines per instruction), off for the quad form (measured 495 -> 515 us:
  // the quad form's gather runs on the otherwise idle texture path beside the LDS reads of the staged rectangles).
  // FVP_TRI_TWO_TILE=0/1 overrides.
  const char* tt_env = fvp::diag_env("FVP_TRI_TWO_TILE");
  const bool staged = fvp::diag_env("FVP_TRIPLANE_STAGED") != nullptr;
  const bool force_lane = fvp::diag_env("FVP_TRIPLANE_LANE") != nullptr;           // read per call: tests switch it
  // lane-per-voxel staged form: JP = 4 .. 12 and 20 (JP = 16 stages through the quad form; JP 24 .. 32 would spill)
  const bool lane_form = !gather && !quad_form && g->JP <= 20 && ((staged && g->JP != 16) || force_lane);
  const int tri_ablate = (tri_ablate_env & ~16) | ((tt_env ? atoi(tt_env) != 0 : lane_form) ? 16 : 0);
  // tests: FVP_TRI_CAP_PX lowers the rectangle size the kernel treats as fitting a tile (the allocation is unchanged),
  // so that one-tile, two-tile and global-gather rectangles all occur on small fixtures; read per call
  auto cap_lim = [](int cap) { const char* e = fvp::diag_env("FVP_TRI_CAP_PX"); const int v = e ? atoi(e) : cap; return v > 0 && v < cap ? v : cap; };
  // two tiles per workgroup, two workgroups (512 threads, <= 128 VGPRs) per CU: 4 x 36 KB + state
  const int cap_px = int((36 * 1024) / (size_t(g->JP) * 4));
  const size_t lds = 2 * size_t(cap_px) * g->JP * 4 + 64;
  if (lane_form) {
    const int lq = (g->JP / 4) | 1;                                           // tile pixel pitch in quads (odd)
    const int cap_px = int((36 * 1024) / (size_t(lq) * 16));
    const size_t lds = 2 * size_t(cap_px) * lq * 16 + 64;
    FVP_LIMIT(size_t(cap_px) * lq * 4 >= size_t(kBX * kBY + (kBX + kBY) * 32) * g->JP);   // the block's plane cells alias tile 0
#define CALL2(NQ_, CACHED_)                                                                                       \
  {                                                                                                                \
    static LdsOptIn optin;                                                                                         \
    auto k = &k_project_triplane_lds2<NQ_, CACHED_>;                                                              \
    if (int e = lds_opt_in(optin, reinterpret_cast<const void*>(k), lds)) return e;                                \
    hipLaunchKernelGGL(k, dim3(nbx * nby * nP), dim3(kTriThreads), lds, as_stream(s), heat_cl,                     \
                       reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, \
                       nP, nbx, nby, ppf, cap_px, *g, fine_grid, F0, F1, F2, planes, tri_ablate, cap_lim(cap_px));                  \
  }
#define CASE2(NQ_) case NQ_: if (fine_grid) CALL2(NQ_, true) else CALL2(NQ_, false) break;
    switch (g->JP / 4) {
      CASE2(1) CASE2(2) CASE2(3) CASE2(4) CASE2(5)
      default: return FVP_ELIMIT;
    }
#undef CASE2
#undef CALL2
    return launch_status();
  }
  const bool blk_form = !gather && !quad_form && !staged;
#else
  constexpr bool blk_form = true;
#endif
  // JP = 16 (Panoptic): the compact-block form WITHOUT LDS staging (k_project_triplane_blk, round 4).  FVP_TRIPLANE_STAGED=1
  // (diagnostics build) keeps the staged quad form for comparison; both give the same bits.
  if (blk_form && nvl <= 2) {
    const int nbx2 = ceil_div(C, kBlkBX);
    const int bz = nvl == 2 ? 16 : kBlkBZ;
    // z-resident cells (ZRES, diagnostics build only: FVP_TRI_ZRES=1).  Measured in round 5, same box, same bits: Panoptic
    // 345 -> 389 us, Shelf 587 -> 654 us, Campus 155 -> 187 us.  The 35-43 KB of cells per workgroup cap a CU at 3-4
    // workgroups where the per-z-block cells (10 KB) let the register count decide (5), and the barriers it removes were
    // never the bound: the phases of the other workgroups on the CU already fill them.
    int zsh = 0;
    while ((1 << zsh) < C) ++zsh;
    const size_t lds_z = (size_t(kBlkBX + kBY) << zsh) * (g->JP + 1) * 4;
#if FVP_DIAG
    const char* zr_env = fvp::diag_env("FVP_TRI_ZRES");
    const bool zres = zr_env && atoi(zr_env) != 0 && (1 << zsh) >= bz && lds_z <= kTriZresMaxLds;
#else
    constexpr bool zres = false;
#endif
    // The OWNED form (k_project_triplane_own, fvp_project_lds.h): x strips that keep their x-y maxima in registers and their
    // x-z cells in LDS; only y-z is merged through global atomics.  Taken wherever its cells fit kTriOwnMaxLds (36 KB: C <= 32,
    // and C = 64 up to JP = 20); beyond that (C = 64 with JP >= 24: 37.5 KB; C >= 128: 42.5 KB and more leave three workgroups per
    // CU, panoptic128 measured 559 -> 523 frames/s) the block form below stays.  The kernel addresses one frame's heatmaps
    // and one camera set's coordinate cache with 32-bit offsets, so shapes whose H * W * JP * V or F0 * F1 * F2 * V do not fit
    // 31 bits keep the block form too (its offsets are 64-bit).  The
    // diagnostics build keeps the block form selectable: FVP_TRI_OWNED=0 (FVP_TRI_ZRES=1 implies it), and FVP_TRI_NY=n
    // overrides the segment count.  Same bits either way.
    const bool fits32 = (long long)g->H * g->W * g->JP * g->V <= INT_MAX && (long long)F0 * F1 * F2 * g->V <= INT_MAX;
    bool owned = tri_owned_lds(C, g->JP) <= kTriOwnMaxLds && fits32 && !zres;
    int ny = tri_owned_ny(C);
#if FVP_DIAG
    if (const char* e = fvp::diag_env("FVP_TRI_OWNED")) owned = owned && atoi(e) != 0;      // read per call: tests switch it
    if (const char* e = fvp::diag_env("FVP_TRI_NY")) {
      const int v = atoi(e), top = ceil_div(C, kBY);
      ny = v < 1 ? 1 : (v > top ? top : v);
    }
#endif
    if (owned) {
      const int nsx = ceil_div(C, kOwnSX);
      int zsh_o = 0;
      while ((1 << zsh_o) < C || (1 << zsh_o) < kOwnBZ) ++zsh_o;
      const size_t lds_o = tri_owned_lds(C, g->JP);
      const bool q5o = nvl == 2 && g->JP == 20 && fvp::diag_env("FVP_TRI_NO_Q5") == nullptr;
#define CALLO(NVL_, CACHED_, Q5_)                                                                                            \
  hipLaunchKernelGGL((k_project_triplane_own<NVL_, CACHED_, Q5_>), dim3(nsx * ny * nP), dim3(kOwnThreads), lds_o,           \
                     as_stream(s), heat_cl, reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, \
                     fx, fy, fz, C, nP, nsx, ny, ppf, *g, fine_grid, F0, F1, F2, planes, zsh_o)
      if (q5o) { if (fine_grid) CALLO(2, true, true); else CALLO(2, false, true); }
      else if (nvl == 2) { if (fine_grid) CALLO(2, true, false); else CALLO(2, false, false); }
      else { if (fine_grid) CALLO(1, true, false); else CALLO(1, false, false); }
#undef CALLO
      return launch_status();
    }
    const size_t lds_b = zres ? lds_z : size_t(kBlkBX * kBY + (kBlkBX + kBY) * bz) * (g->JP + 1) * 4;   // cell pitch JP + 1
#define CALLB(NVL_, CACHED_, ZRES_)                                                                                          \
  hipLaunchKernelGGL((k_project_triplane_blk<NVL_, CACHED_, ZRES_>), dim3(nbx2 * nby * nP), dim3(kBlkThreads), lds_b,       \
                     as_stream(s), heat_cl, reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, \
                     fx, fy, fz, C, nP, nbx2, nby, ppf, *g, fine_grid, F0, F1, F2, planes, zsh)
#if FVP_DIAG
#define CALLB2(NVL_)                                                                     \
  {                                                                                      \
    if (fine_grid) { if (zres) CALLB(NVL_, true, true); else CALLB(NVL_, true, false); } \
    else { if (zres) CALLB(NVL_, false, true); else CALLB(NVL_, false, false); }         \
  }
#else
#define CALLB2(NVL_)                                                                     \
  {                                                                                      \
    if (fine_grid) CALLB(NVL_, true, false); else CALLB(NVL_, false, false);             \
  }
#endif
    // JP = 20 (J = 17: Shelf / Campus): five channel quads - the fifth sampled for four voxels in one pass (Q5, round 6).
    // FVP_TRI_NO_Q5=1 (diagnostics build) keeps the two-group form for comparison; same bits.
    const bool q5 = nvl == 2 && g->JP == 20 && !zres && fvp::diag_env("FVP_TRI_NO_Q5") == nullptr;
    if (q5) {
      if (fine_grid)
        hipLaunchKernelGGL((k_project_triplane_blk<2, true, false, true>), dim3(nbx2 * nby * nP), dim3(kBlkThreads), lds_b, as_stream(s),
                           heat_cl, reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, nP,
                           nbx2, nby, ppf, *g, fine_grid, F0, F1, F2, planes, zsh);
      else
        hipLaunchKernelGGL((k_project_triplane_blk<2, false, false, true>), dim3(nbx2 * nby * nP), dim3(kBlkThreads), lds_b, as_stream(s),
                           heat_cl, reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, nP,
                           nbx2, nby, ppf, *g, fine_grid, F0, F1, F2, planes, zsh);
    } else if (nvl == 2) CALLB2(2) else CALLB2(1)
#undef CALLB2
#undef CALLB
    return launch_status();
  }
#if FVP_DIAG
  if (!gather && nvl <= 2) {
    FVP_LIMIT(cap_px >= kBX * kBY + (kBX + kBY) * (nvl == 1 ? 32 : 16));      // the block's plane cells alias tile 0
#define CALL(NVL_, CACHED_)                                                                                        \
  {                                                                                                                \
    static LdsOptIn optin;                                                                                         \
    auto k = &k_project_triplane_lds<NVL_, CACHED_>;                                                               \
    if (int e = lds_opt_in(optin, reinterpret_cast<const void*>(k), lds)) return e;                                \
    hipLaunchKernelGGL(k, dim3(nbx * nby * nP), dim3(kTriThreads), lds, as_stream(s), heat_cl,                     \
                       reinterpret_cast<const Cam*>(cams), frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, \
                       nP, nbx, nby, ppf, cap_px, *g, fine_grid, F0, F1, F2, planes, tri_ablate, cap_lim(cap_px));                  \
  }
    if (nvl == 1) {
      if (fine_grid) CALL(1, true) else CALL(1, false)
    } else {
      if (fine_grid) CALL(2, true) else CALL(2, false)
    }
#undef CALL
    return launch_status();
  }
  if (nvl == 1) {
    auto k = &k_project_triplane<1>;
    hipLaunchKernelGGL(k, dim3(chunks * nP), dim3(1024), 0, as_stream(s), heat_cl, reinterpret_cast<const Cam*>(cams),
                       frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, nP, chunks, ppf, *g, planes);
  } else if (nvl == 2) {
    auto k = &k_project_triplane<2>;
    hipLaunchKernelGGL(k, dim3(chunks * nP), dim3(1024), 0, as_stream(s), heat_cl, reinterpret_cast<const Cam*>(cams),
                       frame_set, person_frame, person_valid, boxes, fx, fy, fz, C, nP, chunks, ppf, *g, planes);
  } else {
    return FVP_ELIMIT;
  }
  return launch_status();
#else
  return FVP_ELIMIT;                                     // more than 32 joint channels
#endif
}
