// Input heatmaps rasterised from 2-D detections (the reference's "precomputed-heatmap path"):
// lib/dataset/JointsDataset.py:271-338 (generate_input_heatmap, eval branch) on the GPU.
//
// One workgroup per (image, band of RB rows): the band of ALL joints lives in LDS
// (tile[J][RB][W]); the people of the image are stamped one after the other (windows of different
// people overlap; the element-wise max makes the order irrelevant, and exp(.) <= 1 makes the
// reference's clip(0, 1) a no-op), each wave taking every fourth joint.  The band is then written
// once, coalesced, in both layouts: NCHW rows and the channels-last staging copy.  All scalar
// arithmetic of the reference is float64 (numpy promotes the float32 arange against float64
// scalars) and is kept in float64 here: integer truncations, floor division and the IEEE sqrt /
// division are exact, so window positions are bit-identical; exp(double) is rounded to float32 once.
//
// Second input producer of this file: camera frames -> backbone input (k_ingest_*, fvp_ingest_frames below).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "fvp_common.h"

namespace fvp {

// A joint is stamped, and counts for its person's extent, when both quotients are finite (a NaN or an Inf fails the compare)
__device__ __forceinline__ bool ras_finite(double x, double y) {
  const double big = 1.7976931348623157e308;          // DBL_MAX
  return fabs(x) <= big && fabs(y) <= big;
}
constexpr double kRasBig = 1073741824.0;              // 2^30: window corners and lengths are clamped to it before int()

__global__ void __launch_bounds__(256)
k_rasterise(const double* __restrict__ joints, const int* __restrict__ num_people, int P, int J, int W, int H, int RB,
            double fsx, double fsy, double sigma, float* __restrict__ nchw, float* __restrict__ cl, int JP) {
  HIP_DYNAMIC_SHARED(float, tile)                     // [J][RB][W]
  constexpr int kMaxPJ = 1024;                        // people x joints handled per pass (host-checked)
  __shared__ double q[kMaxPJ][2];                     // joints / feat_stride
  __shared__ double prm[64][4];                       // per person: tmp_size, x0, den, ng
  const int img = blockIdx.y, y0 = blockIdx.x * RB, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rows = H - y0 < RB ? H - y0 : RB;
  const int plane = RB * W;
  for (int i = t; i < J * plane; i += 256) tile[i] = 0.0f;
  const int np_ = num_people[img] < P ? num_people[img] : P;
  // ---- per-joint quotients and per-person Gaussian parameters, once per workgroup
  const double* pj = joints + size_t(img) * P * J * 2;
  for (int i = t; i < np_ * J; i += 256) {
    q[i][0] = pj[2 * i] / fsx;
    q[i][1] = pj[2 * i + 1] / fsy;
  }
  __syncthreads();
  if (t < np_) {
    // compute_human_scale (:197-203) with every FINITE joint visible (include/fvp.h: a joint with a NaN or an Inf is left out)
    const double(*qp)[2] = q + t * J;
    double minx = 0, maxx = 0, miny = 0, maxy = 0;
    bool any = false;
    for (int k = 0; k < J; ++k) {
      if (!ras_finite(qp[k][0], qp[k][1])) continue;
      minx = any ? fmin(minx, qp[k][0]) : qp[k][0];
      maxx = any ? fmax(maxx, qp[k][0]) : qp[k][0];
      miny = any ? fmin(miny, qp[k][1]) : qp[k][1];
      maxy = any ? fmax(maxy, qp[k][1]) : qp[k][1];
      any = true;
    }
    const double ext = fmax(maxy - miny, maxx - minx);
    double hs = ext * ext;
    hs = fmin(fmax(hs, 1.0 / 4 * 96 * 96), 4.0 * 96 * 96);
    hs = 2 * hs;
    const double cur_sigma = sigma * sqrt(hs / (96.0 * 96.0));
    const double tmp_size = cur_sigma * 3;
    const double size = 2 * tmp_size + 1;
    prm[t][0] = any ? tmp_size : -1.0;                // no finite joint: the person stamps nothing
    prm[t][1] = floor(size / 2);                      // x0 = y0 = size // 2
    prm[t][2] = 2 * (cur_sigma * cur_sigma);
    prm[t][3] = fmin(ceil(size), kRasBig);            // len(np.arange(0, size, 1))
  }
  for (int n = 0; n < np_; ++n) {
    __syncthreads();                                  // parameters ready; previous person's LDS stores done
    const double tmp_size = prm[n][0], x0 = prm[n][1], den = prm[n][2];
    if (!(tmp_size >= 0)) continue;                   // uniform over the workgroup
    const int ng = int(prm[n][3]);
    for (int j = wave; j < J; j += 4) {
      const double qx = q[n * J + j][0], qy = q[n * J + j][1];
      if (!ras_finite(qx, qy)) continue;
      // Python's int() truncates toward zero and never overflows: the window is placed in float64 (trunc() of a double is
      // exact, and so is float(int(q))), and only a window that meets the image - corners within 2 tmp_size + 2 of it - is
      // converted to int.  No NaN or Inf reaches a conversion (sigma and the strides are finite: host-checked).
      const double mu_x = trunc(qx), mu_y = trunc(qy);
      const double dul0 = trunc(mu_x - tmp_size), dul1 = trunc(mu_y - tmp_size);
      const double dbr0 = trunc(mu_x + tmp_size + 1), dbr1 = trunc(mu_y + tmp_size + 1);
      if (dul0 >= W || dul1 >= H || dbr0 < 0 || dbr1 < 0) continue;
      const int ul0 = int(fmax(dul0, -kRasBig)), ul1 = int(fmax(dul1, -kRasBig));
      const int br0 = int(fmin(dbr0, kRasBig)), br1 = int(fmin(dbr1, kRasBig));
      const int gx0 = ul0 < 0 ? -ul0 : 0, gx1 = (br0 < W ? br0 : W) - ul0;
      const int gy0 = ul1 < 0 ? -ul1 : 0, gy1 = (br1 < H ? br1 : H) - ul1;
      const int ix0 = ul0 > 0 ? ul0 : 0, iy0 = ul1 > 0 ? ul1 : 0;
      // numpy slicing clamps the stop index to the array length
      const int wx = (gx1 < ng ? gx1 : ng) - gx0, wy = (gy1 < ng ? gy1 : ng) - gy0;
      if (wx <= 0 || wy <= 0) continue;
      // rows of the window inside this band
      const int ya = iy0 > y0 ? iy0 : y0, yb = (iy0 + wy < y0 + rows ? iy0 + wy : y0 + rows);
      if (ya >= yb) continue;
      float* tj = tile + j * plane;
      for (int i = lane; i < (yb - ya) * wx; i += 64) {
        const int ry = i / wx, xx = i - ry * wx;
        const int yy = ya + ry - iy0;                 // row inside the window slice
        const double dx = double(gx0 + xx) - x0, dy = double(gy0 + yy) - x0;
        const float g = float(exp(-(dx * dx + dy * dy) / den));
        float* d = tj + (ya + ry - y0) * W + ix0 + xx;
        *d = fmaxf(*d, g);
      }
    }
  }
  __syncthreads();
  const int HW = H * W;
  if (nchw)
    for (int i = t; i < J * rows * W; i += 256) {
      const int j = i / (rows * W), r = i - j * (rows * W);
      nchw[(size_t(img) * J + j) * HW + y0 * W + r] = tile[j * plane + r];
    }
  if (cl)
    for (int i = t; i < rows * W * JP; i += 256) {
      const int px = i / JP, c = i - px * JP;
      cl[(size_t(img) * HW + y0 * W + px) * JP + c] = c < J ? tile[c * plane + px] : 0.0f;
    }
}


// ---- camera frames -> backbone input ----------------------------------------------------------------------------------
// uint8 HWC frames at the camera's resolution -> bilinear warp through a 2x3 matrix (destination pixel -> source pixel,
// taps outside the frame are 0), channel swap, / 255, mean / std: the reference's preprocess.py warpAffine call and its
// loader (JointsDataset.py:129-133, run/validate.py:44-52) in one pass, written as the stem's pixel-pair bf16 input
// (k_bb_input's layout) and / or as the fp32 NCHW tensor a torch backbone reads.  Memory traffic only: one lane per
// destination pixel PAIR, one 16-byte store.
//
// The arithmetic is fixed (include/fvp.h) and lives in ingest_pair(), which takes the source of a tap's pixel as a
// functor.  One form ships: k_ingest_gather reads the bytes from global memory (any matrix).  A second form that first
// copied the source rectangle of a 128 x 4 destination tile into LDS with 16-byte loads (rows realigned by their byte
// offset) computed the same bits but was not faster on the card - 257 us against 192 us for 40 frames 1080p -> 512x960,
// 159 against 167 us at 512x960 -> 512x960 (profiles/ingest_kernel.txt) - and was dropped; FVP_INGEST_GENERAL is
// accepted and changes nothing.  This TU is compiled with -ffp-contract=off: every * + - / below is rounded on its own.
struct IngestPrm {
  float inv[6], mean[3], stdv[3];
};
struct alignas(16) IngestB16 { uint32_t w[4]; };            // one 16-byte store

__device__ __forceinline__ uint16_t ingest_f2bf(float f) {   // round to nearest even: f2bf of fvp_backbone.hip
  uint32_t u = uint32_t(__float_as_int(f));
  u += 0x7fffu + ((u >> 16) & 1u);
  return uint16_t(u >> 16);
}

__device__ __forceinline__ float ingest_coord(float a, float b, float c, int x, int y) {
  return a * float(x) + b * float(y) + c;
}

// floor() of a source coordinate as an int; anything that cannot have a tap inside [0, n) becomes -2 (both taps outside)
__device__ __forceinline__ int ingest_cell(float fl, int n) { return (fl >= -1.0f && fl < float(n)) ? int(fl) : -2; }

struct IngestPx { float c[3]; };                            // one source pixel, OUTPUT channel order

// Destination pixels (2 * xp, y) and (2 * xp + 1, y) of image n.  tap(yy, xx) = the source pixel as three floats in
// output channel order, both coordinates already inside the frame; it is called once per in-frame tap and feeds the
// three bilinear evaluations (an NV12 tap converts to R, G, B there, once).
template <class Tap>
__device__ __forceinline__ void ingest_pair(const IngestPrm& p, int Hs, int Ws, int H, int W, int n, int y, int xp,
                                            uint16_t* __restrict__ nhwc8, float* __restrict__ nchw, Tap tap) {
  uint16_t v16[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const long hw = long(H) * W;
  const IngestPx zero = {{0.0f, 0.0f, 0.0f}};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int x = 2 * xp + e;
    const float sx = ingest_coord(p.inv[0], p.inv[1], p.inv[2], x, y);
    const float sy = ingest_coord(p.inv[3], p.inv[4], p.inv[5], x, y);
    const float flx = floorf(sx), fly = floorf(sy);
    const float fx = sx - flx, fy = sy - fly;
    const int x0 = ingest_cell(flx, Ws), y0 = ingest_cell(fly, Hs);
    const bool xa = x0 >= 0, xb = x0 + 1 >= 0 && x0 + 1 < Ws, ya = y0 >= 0, yb = y0 + 1 >= 0 && y0 + 1 < Hs;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const IngestPx p00 = ya && xa ? tap(y0, x0) : zero, p01 = ya && xb ? tap(y0, x0 + 1) : zero;
    const IngestPx p10 = yb && xa ? tap(y0 + 1, x0) : zero, p11 = yb && xb ? tap(y0 + 1, x0 + 1) : zero;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = gy * (gx * p00.c[c] + fx * p01.c[c]) + fy * (gx * p10.c[c] + fx * p11.c[c]);
      const float o = __fdiv_rn(__fdiv_rn(v, 255.0f) - p.mean[c], p.stdv[c]);
      v16[4 * e + c] = ingest_f2bf(o);
      if (nchw) nchw[(long(n) * 3 + c) * hw + long(y) * W + x] = o;
    }
  }
  if (nhwc8) {
    IngestB16 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o.w[e] = uint32_t(v16[2 * e]) | (uint32_t(v16[2 * e + 1]) << 16);
    *reinterpret_cast<IngestB16*>(nhwc8 + ((long(n) * H + y) * (W / 2) + xp) * 8) = o;
  }
}

// Any matrix, 12 byte loads per pixel through L1.
__global__ void __launch_bounds__(256)
k_ingest_gather(const uint8_t* __restrict__ frames, int N, int Hs, int Ws, IngestPrm p, int H, int W, int swap,
                uint16_t* __restrict__ nhwc8, float* __restrict__ nchw) {
  const long i = long(blockIdx.x) * 256 + threadIdx.x;       // one thread per pixel PAIR
  const int w2 = W / 2;
  if (i >= long(N) * H * w2) return;
  const int n = int(i / (long(H) * w2));
  const int r = int(i - long(n) * H * w2);
  const int y = r / w2, xp = r - y * w2;
  const uint8_t* f = frames + long(n) * Hs * Ws * 3;
  const int c0 = swap ? 2 : 0, c2 = 2 - c0;
  ingest_pair(p, Hs, Ws, H, W, n, y, xp, nhwc8, nchw, [&](int yy, int xx) {
    const uint8_t* q = f + (long(yy) * Ws + xx) * 3;
    return IngestPx{{float(q[c0]), float(q[1]), float(q[c2])}};
  });
}

// NV12 surface (include/fvp.h): a tap is one luma byte and the (U, V) pair of its 2 x 2 quad as ONE 2-byte load,
// converted to R, G, B in int32 once.  8 + 8 loads per lane against the 24 of k_ingest_gather, 1.5 source bytes per pixel
// against 3.  Neighbouring taps that share a chroma sample load it again (same cache line).
struct Nv12Prm {
  long y_pitch, uv_pitch, y_frame, uv_frame;
  int yoff, cy, crv, cgu, cgv, cbu;
};

__device__ __forceinline__ float ingest_clip8(int v) {      // (v >> 20) clipped to a byte; >> is arithmetic
  const int b = v >> 20;
  return float(b < 0 ? 0 : b > 255 ? 255 : b);
}

__global__ void __launch_bounds__(256)
k_ingest_nv12(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp, int N, int Hs, int Ws, Nv12Prm q,
              IngestPrm p, int H, int W, uint16_t* __restrict__ nhwc8, float* __restrict__ nchw) {
  const long i = long(blockIdx.x) * 256 + threadIdx.x;       // one thread per pixel PAIR
  const int w2 = W / 2;
  if (i >= long(N) * H * w2) return;
  const int n = int(i / (long(H) * w2));
  const int r = int(i - long(n) * H * w2);
  const int y = r / w2, xp = r - y * w2;
  const uint8_t* fy = yp + long(n) * q.y_frame;
  const uint8_t* fuv = uvp + long(n) * q.uv_frame;
  ingest_pair(p, Hs, Ws, H, W, n, y, xp, nhwc8, nchw, [&](int yy, int xx) {
    const int luma = fy[long(yy) * q.y_pitch + xx];
    const uint32_t w = *reinterpret_cast<const uint16_t*>(fuv + long(yy >> 1) * q.uv_pitch + 2 * (xx >> 1));
    const int c = luma > q.yoff ? luma - q.yoff : 0, d = int(w & 0xffu) - 128, e = int(w >> 8) - 128;
    const int l = q.cy * c + (1 << 19);
    return IngestPx{{ingest_clip8(l + q.crv * e), ingest_clip8(l + q.cgu * d + q.cgv * e), ingest_clip8(l + q.cbu * d)}};
  });
}

// ---- Bayer raw frames (fvp_demosaic_bayer, fvp_ingest_bayer; include/fvp.h, ABI 24) -------------------------------------
// One byte per source pixel.  The source RGB pixel is the integer Malvar-He-Cutler filter of include/fvp.h: bayer_px() on
// the six neighbour sums of a site, the only place the formulas are written.  Three kernels use it:
//   k_demosaic_bayer       a lane owns 4 x 2 pixels (two whole cells): a 6 x 8 window read as three dwords per row where
//                          the row is 4-byte aligned (bytes otherwise, row by row), 12-byte stores;
//   k_ingest_bayer_lds     a workgroup owns 64 x 8 destination pixels: the source rectangle of its taps (from inv at the
//                          tile's corners: every rounded operation of ingest_coord is monotone, so the extremes are there)
//                          plus the halo goes into LDS with dword loads, is demosaiced and toned ONCE there by the same
//                          4 x 2 block code into one packed dword per pixel, and ingest_pair's tap is one LDS read;
//   k_ingest_bayer_gather  any matrix: 13 byte loads per tap.  Taken when the rectangle of bayer_lds_plan() does not fit.
// The site type of a pixel depends on its parity alone, the pattern is uniform: no lane diverges on it.
struct BayerPrm {
  long pitch, frame;
  int rx, ry;
};
struct BayerRgb { int r, g, b; };

// about the edge sample, without repeating it.  The final clamp never acts on a neighbour of a real pixel (offsets <= 2,
// n >= 4): it keeps the columns past a frame whose width is no multiple of 4, which nothing uses, inside the row.
__device__ __forceinline__ int bayer_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return i < 0 ? 0 : i;
}

__device__ __forceinline__ int bayer_round(int x16) {        // clip(0, 255, (X16 + 8) >> 4); >> is arithmetic
  const int v = (x16 + 8) >> 4;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// xr: the site's column parity is the red one; yr: its row parity is the red one
__device__ __forceinline__ BayerRgb bayer_px(int c, int H1, int V1, int D, int H2, int V2, bool xr, bool yr) {
  const int own = 16 * c;
  int r, g, b;
  if (xr == yr) {                                            // a red or a blue site
    g = 8 * c + 4 * (H1 + V1) - 2 * (H2 + V2);
    const int third = 12 * c + 4 * D - 3 * (H2 + V2);
    r = xr ? own : third;
    b = xr ? third : own;
  } else {                                                   // a green site; yr: in a red row
    g = own;
    const int row = 10 * c + 8 * H1 - 2 * D - 2 * H2 + V2, col = 10 * c + 8 * V1 - 2 * D - 2 * V2 + H2;
    r = yr ? row : col;
    b = yr ? col : row;
  }
  return BayerRgb{bayer_round(r), bayer_round(g), bayer_round(b)};
}

// bytes 2..9 of three consecutive dwords: the columns x - 2 .. x + 5 of a block at x, the dwords starting at x - 4
__device__ __forceinline__ void bayer_unpack(uint32_t d0, uint32_t d1, uint32_t d2, int (&w)[8]) {
  w[0] = int((d0 >> 16) & 0xffu);
  w[1] = int(d0 >> 24);
  w[2] = int(d1 & 0xffu);
  w[3] = int((d1 >> 8) & 0xffu);
  w[4] = int((d1 >> 16) & 0xffu);
  w[5] = int(d1 >> 24);
  w[6] = int(d2 & 0xffu);
  w[7] = int((d2 >> 8) & 0xffu);
}

// The 4 x 2 block at even (x, y) from its window w (rows y - 2 .. y + 3, columns x - 2 .. x + 5) as R | G << 8 | B << 16.
// tone_l: the table in LDS, read when has_tone (uniform).
__device__ __forceinline__ void bayer_block(const int (&w)[6][8], int rx, int ry, bool has_tone, const uint8_t* tone_l,
                                            uint32_t (&out)[2][4]) {
#pragma unroll
  for (int py = 0; py < 2; ++py)
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      const int r = py + 2, q = px + 2;
      BayerRgb v = bayer_px(w[r][q], w[r][q - 1] + w[r][q + 1], w[r - 1][q] + w[r + 1][q],
                            w[r - 1][q - 1] + w[r - 1][q + 1] + w[r + 1][q - 1] + w[r + 1][q + 1],
                            w[r][q - 2] + w[r][q + 2], w[r - 2][q] + w[r + 2][q], (px & 1) == rx, (py & 1) == ry);
      if (has_tone) {
        v.r = tone_l[v.r];
        v.g = tone_l[256 + v.g];
        v.b = tone_l[512 + v.b];
      }
      out[py][px] = uint32_t(v.r) | (uint32_t(v.g) << 8) | (uint32_t(v.b) << 16);
    }
}

__device__ __forceinline__ void bayer_stage_tone(const uint8_t* __restrict__ tone, uint8_t* tone_l) {
  if (tone)                                                  // uniform
    for (int i = threadIdx.x; i < 768; i += 256) tone_l[i] = tone[i];
}

struct alignas(4) BayerB12 { uint32_t w[3]; };              // four packed pixels: one 12-byte store

constexpr int kBayerTW = 256, kBayerTH = 8;                  // pixels of a k_demosaic_bayer workgroup: 64 x 4 blocks

__global__ void __launch_bounds__(256)
k_demosaic_bayer(const uint8_t* __restrict__ raw, int Hs, int Ws, BayerPrm q, const uint8_t* __restrict__ tone,
                 int tiles_x, int tiles_y, uint8_t* __restrict__ rgb) {
  __shared__ uint8_t tone_l[768];
  bayer_stage_tone(tone, tone_l);
  __syncthreads();
  const int t = threadIdx.x;
  const long bid = blockIdx.x;
  const int tx = int(bid % tiles_x), ty = int((bid / tiles_x) % tiles_y), n = int(bid / (long(tiles_x) * tiles_y));
  const int x = tx * kBayerTW + (t & 63) * 4, y = ty * kBayerTH + (t >> 6) * 2;
  if (x >= Ws || y >= Hs) return;
  const uint8_t* f = raw + long(n) * q.frame;
  int w[6][8];
  const bool inner = x >= 4 && x + 8 <= Ws;                  // the three dwords x - 4 .. x + 7 lie inside the row
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const uint8_t* row = f + long(bayer_reflect(y - 2 + r, Hs)) * q.pitch;
    if (inner && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
      const uint32_t* d = reinterpret_cast<const uint32_t*>(row + x - 4);
      bayer_unpack(d[0], d[1], d[2], w[r]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) w[r][k] = row[bayer_reflect(x - 2 + k, Ws)];
    }
  }
  uint32_t o[2][4];
  bayer_block(w, q.rx, q.ry, tone != nullptr, tone_l, o);
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    uint8_t* p = rgb + ((long(n) * Hs + y + py) * Ws + x) * 3;
    if (x + 4 <= Ws && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
      BayerB12 v;
      v.w[0] = o[py][0] | (o[py][1] << 24);
      v.w[1] = (o[py][1] >> 8) | (o[py][2] << 16);
      v.w[2] = (o[py][2] >> 16) | (o[py][3] << 8);
      *reinterpret_cast<BayerB12*>(p) = v;
    } else {
#pragma unroll
      for (int px = 0; px < 4; ++px)
        if (x + px < Ws) {
          p[3 * px] = uint8_t(o[py][px]);
          p[3 * px + 1] = uint8_t(o[py][px] >> 8);
          p[3 * px + 2] = uint8_t(o[py][px] >> 16);
        }
    }
  }
}

__device__ __forceinline__ IngestPx bayer_unpack_px(uint32_t v) {
  return IngestPx{{float(v & 0xffu), float((v >> 8) & 0xffu), float((v >> 16) & 0xffu)}};
}

// Any matrix: a tap demosaics its own pixel from 13 byte loads through L1.
__global__ void __launch_bounds__(256)
k_ingest_bayer_gather(const uint8_t* __restrict__ raw, int N, int Hs, int Ws, BayerPrm q, const uint8_t* __restrict__ tone,
                      IngestPrm p, int H, int W, uint16_t* __restrict__ nhwc8, float* __restrict__ nchw) {
  __shared__ uint8_t tone_l[768];
  bayer_stage_tone(tone, tone_l);
  __syncthreads();
  const long i = long(blockIdx.x) * 256 + threadIdx.x;       // one thread per pixel PAIR
  const int w2 = W / 2;
  if (i >= long(N) * H * w2) return;
  const int n = int(i / (long(H) * w2));
  const int r = int(i - long(n) * H * w2);
  const int y = r / w2, xp = r - y * w2;
  const uint8_t* f = raw + long(n) * q.frame;
  const bool has_tone = tone != nullptr;
  ingest_pair(p, Hs, Ws, H, W, n, y, xp, nhwc8, nchw, [&](int yy, int xx) {
    const uint8_t* r0 = f + long(yy) * q.pitch;
    const uint8_t* ra = f + long(bayer_reflect(yy - 1, Hs)) * q.pitch;
    const uint8_t* rb = f + long(bayer_reflect(yy + 1, Hs)) * q.pitch;
    const uint8_t* ra2 = f + long(bayer_reflect(yy - 2, Hs)) * q.pitch;
    const uint8_t* rb2 = f + long(bayer_reflect(yy + 2, Hs)) * q.pitch;
    const int xa = bayer_reflect(xx - 1, Ws), xb = bayer_reflect(xx + 1, Ws);
    const int xa2 = bayer_reflect(xx - 2, Ws), xb2 = bayer_reflect(xx + 2, Ws);
    BayerRgb v = bayer_px(r0[xx], int(r0[xa]) + int(r0[xb]), int(ra[xx]) + int(rb[xx]),
                          int(ra[xa]) + int(ra[xb]) + int(rb[xa]) + int(rb[xb]), int(r0[xa2]) + int(r0[xb2]),
                          int(ra2[xx]) + int(rb2[xx]), (xx & 1) == q.rx, (yy & 1) == q.ry);
    if (has_tone) {
      v.r = tone_l[v.r];
      v.g = tone_l[256 + v.g];
      v.b = tone_l[512 + v.b];
    }
    return IngestPx{{float(v.r), float(v.g), float(v.b)}};
  });
}

constexpr int kBayerDW = 64, kBayerDH = 8;                   // destination pixels of a k_ingest_bayer_lds workgroup

// LDS: rgb [RH][RW] dwords (R | G << 8 | B << 16 of source pixel (ox + j, oy + i)), then raw [RH + 4][RW + 8] bytes (source
// rows oy - 2 .., columns ox - 4 .., reflected).  ox is a multiple of 4, oy even, RW a multiple of 4, RH even; RW x RH is
// bayer_lds_plan()'s bound on every tile's rectangle.
__global__ void __launch_bounds__(256)
k_ingest_bayer_lds(const uint8_t* __restrict__ raw, int Hs, int Ws, BayerPrm q, const uint8_t* __restrict__ tone,
                   IngestPrm p, int H, int W, int tiles_x, int tiles_y, int RW, int RH, uint16_t* __restrict__ nhwc8,
                   float* __restrict__ nchw) {
  HIP_DYNAMIC_SHARED(uint32_t, rgbl)
  __shared__ uint8_t tone_l[768];
  uint32_t* rawl = rgbl + RH * RW;
  const int rawd = (RW + 8) / 4;                             // dwords of a raw row in LDS
  const int t = threadIdx.x;
  const long bid = blockIdx.x;
  const int tx = int(bid % tiles_x), ty = int((bid / tiles_x) % tiles_y), n = int(bid / (long(tiles_x) * tiles_y));
  const int X0 = tx * kBayerDW, Y0 = ty * kBayerDH;
  const int X1 = X0 + kBayerDW - 1 < W - 1 ? X0 + kBayerDW - 1 : W - 1, Y1 = Y0 + kBayerDH - 1 < H - 1 ? Y0 + kBayerDH - 1 : H - 1;
  // floor of the source coordinates at the tile's four corners: the extremes over the tile
  float lox = 0.0f, hix = 0.0f, loy = 0.0f, hiy = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cx = (k & 1) ? X1 : X0, cy = (k & 2) ? Y1 : Y0;
    const float fx = floorf(ingest_coord(p.inv[0], p.inv[1], p.inv[2], cx, cy));
    const float fy = floorf(ingest_coord(p.inv[3], p.inv[4], p.inv[5], cx, cy));
    lox = k ? fminf(lox, fx) : fx;
    hix = k ? fmaxf(hix, fx) : fx;
    loy = k ? fminf(loy, fy) : fy;
    hiy = k ? fmaxf(hiy, fy) : fy;
  }
  // in-frame taps: columns max(lox, 0) .. min(hix + 1, Ws - 1), rows alike; empty when the tile is outside the frame
  const int x0 = int(fminf(fmaxf(lox, 0.0f), float(Ws))), x1 = int(fminf(fmaxf(hix + 1.0f, -1.0f), float(Ws - 1)));
  const int y0 = int(fminf(fmaxf(loy, 0.0f), float(Hs))), y1 = int(fminf(fmaxf(hiy + 1.0f, -1.0f), float(Hs - 1)));
  const int ox = x0 & ~3, oy = y0 & ~1;
  int rw = 0, rh = 0;
  if (x1 >= x0 && y1 >= y0) {
    rw = (x1 + 1 - ox + 3) & ~3;
    rh = (y1 + 1 - oy + 1) & ~1;
    rw = rw < RW ? rw : RW;                                  // never acts (bayer_lds_plan); keeps LDS indices inside
    rh = rh < RH ? rh : RH;
  }
  const uint8_t* f = raw + long(n) * q.frame;
  bayer_stage_tone(tone, tone_l);
  const int nd = (rw + 8) / 4;
  for (int i = t; i < (rh + 4) * nd && rw; i += 256) {
    const int r = i / nd, j = i - r * nd, cx = ox - 4 + 4 * j;
    const uint8_t* row = f + long(bayer_reflect(oy - 2 + r, Hs)) * q.pitch;
    uint32_t v;
    if (cx >= 0 && cx + 4 <= Ws && (reinterpret_cast<uintptr_t>(row) & 3) == 0) {
      v = *reinterpret_cast<const uint32_t*>(row + cx);
    } else {
      v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= uint32_t(row[bayer_reflect(cx + k, Ws)]) << (8 * k);
    }
    rawl[r * rawd + j] = v;
  }
  __syncthreads();
  const int nbx = rw / 4;
  for (int i = t; i < nbx * (rh / 2); i += 256) {
    const int by = i / nbx, bx = i - by * nbx;
    int w[6][8];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const uint32_t* d = rawl + (by * 2 + r) * rawd + bx;
      bayer_unpack(d[0], d[1], d[2], w[r]);
    }
    uint32_t o[2][4];
    bayer_block(w, q.rx, q.ry, tone != nullptr, tone_l, o);
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 4; ++px) rgbl[(by * 2 + py) * RW + bx * 4 + px] = o[py][px];
  }
  __syncthreads();
  const int xp = X0 / 2 + (t & 31), y = Y0 + (t >> 5);
  if (2 * xp >= W || y >= H) return;
  ingest_pair(p, Hs, Ws, H, W, n, y, xp, nhwc8, nchw,
              [&](int yy, int xx) { return bayer_unpack_px(rgbl[(yy - oy) * RW + (xx - ox)]); });
}

// ---- poses back onto the camera frames (fvp_draw_poses, include/fvp.h) ---------------------------------------------------
// Third image kernel of this file, the only one that WRITES frames.  Tile-centric: a workgroup owns 64 x 16 pixels of one
// frame (a wave's lanes are 64 consecutive x of one row: 192 contiguous bytes), walks the frame's N * (J + L) primitives in
// chunks of the block size - a thread builds one primitive in Q4 from `views` and appends it to a list in LDS when its
// bounding box meets the tile - and every pixel thread runs the list and ORs 1 << n into a coverage mask per pixel (hence
// N <= 32).  A pixel with a non-zero mask loads its three bytes, blends the persons in ascending bit order and stores them;
// a tile whose lists stay empty never touches the frame.  A wave per limb writing its own pixels would race wherever two
// people overlap, and the blend order would depend on scheduling.
// All coverage arithmetic is exact integer arithmetic (a disc is the capsule with a == b).
struct DrawPrm {
  uint8_t limb[64][2];
  uint8_t pal[64][3];
};
constexpr int kDrawTW = 64, kDrawTH = 16, kDrawThreads = 256;
constexpr int kDrawRows = kDrawTH / (kDrawThreads / kDrawTW);                        // pixels (rows) per thread
constexpr int kDrawMaxN = 32, kDrawMaxL = 64, kDrawMaxP = 64, kDrawMaxR = 1024;
constexpr int kDrawMaxChunks = (kDrawMaxN * (FVP_MAX_JOINTS + kDrawMaxL) + kDrawThreads - 1) / kDrawThreads;

// Q4 position of joint `vj` (index into views / 4) when it is drawable.  |.| <= 32768 fails for NaN and Inf.
__device__ __forceinline__ bool draw_joint(const float* __restrict__ views, const float* __restrict__ conf, float conf_min,
                                           long vj, long cj, int& qx, int& qy) {
  const float px = views[4 * vj], py = views[4 * vj + 1], depth = views[4 * vj + 2];
  bool ok = depth > 0.0f && fabsf(px) <= 32768.0f && fabsf(py) <= 32768.0f;
  if (conf) ok = ok && conf[cj] >= conf_min;
  qx = ok ? int(rintf(px * 16.0f)) : 0;                   // exact product, round-half-even
  qy = ok ? int(rintf(py * 16.0f)) : 0;
  return ok;
}

// Pixel centre p against the capsule of half-width rad around a-b (include/fvp.h).  Coordinates are below 2^20 in
// magnitude, so t, dd and the cross product stay below 2^42 and rad^2 * dd below 2^62: everything but the square of the
// cross product fits 64 bits.  That square is a 128-bit product (c_hi 2^32 + c_lo)^2; whenever c_hi != 0 it is >= 2^64 and
// exceeds the right-hand side, otherwise it is c_lo * c_lo, which fits - so only the low product is ever formed.
__device__ __forceinline__ bool draw_covers(int px, int py, int ax, int ay, int bx, int by, int rad) {
  const long long dx = bx - ax, dy = by - ay, wx = px - ax, wy = py - ay;
  const long long r2 = (long long)rad * rad;
  const long long t = wx * dx + wy * dy, dd = dx * dx + dy * dy;
  if (t <= 0) return wx * wx + wy * wy <= r2;
  if (t >= dd) {
    const long long ex = px - bx, ey = py - by;
    return ex * ex + ey * ey <= r2;
  }
  const long long c = wx * dy - wy * dx;
  const unsigned long long a = (unsigned long long)(c < 0 ? -c : c);
  return (a >> 32) == 0 && a * a <= (unsigned long long)r2 * (unsigned long long)dd;
}

// the CPU emulation's read fences (tests/hipemu) see the frame bytes a pixel thread is about to load: the test of "pixels
// that nothing covers are not read"; nothing on the device
__device__ __forceinline__ void draw_note_read(const uint8_t* p) {
#if defined(HIPEMU)
  if (hipemu::nfences) hipemu::fenced_read_check(p);
#else
  (void)p;
#endif
}

// LDS of a draw kernel.  cnt[c]: hits of chunk c (never reset: no barrier between a chunk's readers and the next chunk's
// writers); the lists alternate, chunk c + 2 rewrites list c & 1 only after the barrier of chunk c + 1, which every reader of
// c has passed
struct DrawLds {
  int cnt[kDrawMaxChunks];
  int seg[2][kDrawThreads][4];
  int tag[2][kDrawThreads];                            // person | radius << 8
  unsigned pcol[kDrawMaxN];                            // three colour bytes | drawn << 24
};

// Before the first barrier: empty lists, and thread n looks up person n's colour (prm.pal is in the surface's own channels)
__device__ __forceinline__ void draw_begin(DrawLds& s, int tid, const int32_t* __restrict__ ids, int b, int N, int P,
                                           const DrawPrm& prm) {
  if (tid < kDrawMaxChunks) s.cnt[tid] = 0;
  if (tid < N) {
    const int key = ids ? ids[long(b) * N + tid] : tid;
    unsigned col = 0;
    if (key >= 0) {
      const uint8_t* c = prm.pal[key % P];
      col = unsigned(c[0]) | (unsigned(c[1]) << 8) | (unsigned(c[2]) << 16) | (1u << 24);
    }
    s.pcol[tid] = col;
  }
}

// Primitive i of frame f (person i / (J + L); its joints first, then its limbs) built in Q4 and appended to list c & 1 when
// its bounding box meets the tile [x0, x1] x [y0, y1]
__device__ __forceinline__ void draw_collect(DrawLds& s, int c, int i, int f, int b, const float* __restrict__ views,
                                             const float* __restrict__ conf, float conf_min, int N, int J, int L,
                                             const DrawPrm& prm, int R, int W, int x0, int y0, int x1, int y1) {
  const int per = J + L;
  if (i >= N * per) return;
  const int n = i / per, r = i - n * per;
  if (!(s.pcol[n] >> 24)) return;
  int j0 = r, j1 = r, rad = R;
  if (r >= J) {
    j0 = prm.limb[r - J][0];
    j1 = prm.limb[r - J][1];
    rad = W;
  }
  const long vrow = (long(f) * N + n) * J, crow = (long(b) * N + n) * J;
  int ax, ay, bx, by;
  bool ok = draw_joint(views, conf, conf_min, vrow + j0, crow + j0, ax, ay);
  bx = ax;
  by = ay;
  if (j1 != j0) {
    const bool ok1 = draw_joint(views, conf, conf_min, vrow + j1, crow + j1, bx, by);
    ok = ok && ok1;
  }
  const int lox = (ax < bx ? ax : bx) - rad, hix = (ax < bx ? bx : ax) + rad;
  const int loy = (ay < by ? ay : by) - rad, hiy = (ay < by ? by : ay) + rad;
  if (ok && hix >= 16 * x0 && lox <= 16 * x1 && hiy >= 16 * y0 && loy <= 16 * y1) {
    const int k = atomicAdd(&s.cnt[c], 1);
    int* e = s.seg[c & 1][k];
    e[0] = ax;
    e[1] = ay;
    e[2] = bx;
    e[3] = by;
    s.tag[c & 1][k] = n | (rad << 8);
  }
}

// The thread's K pixel centres (Q4) against list c & 1, behind the barrier that follows draw_collect: bit n of mask[e] is set
// when a primitive of person n covers pixel e
template <int K>
__device__ __forceinline__ void draw_scan(const DrawLds& s, int c, const int (&px)[K], const int (&py)[K], unsigned (&mask)[K]) {
  const int m = s.cnt[c];
  for (int k = 0; k < m; ++k) {
    const int* e = s.seg[c & 1][k];
    const int ax = e[0], ay = e[1], bx = e[2], by = e[3], tg = s.tag[c & 1][k];
    const unsigned bit = 1u << (tg & 31);
#pragma unroll
    for (int r = 0; r < K; ++r)
      if (draw_covers(px[r], py[r], ax, ay, bx, by, tg >> 8)) mask[r] |= bit;
  }
}

__global__ void __launch_bounds__(kDrawThreads)
k_draw_poses(uint8_t* __restrict__ frames, int V, int Hs, int Ws, const float* __restrict__ views,
             const int32_t* __restrict__ ids, const float* __restrict__ conf, int N, int J, int L, int P, DrawPrm prm,
             int R, int W, int alpha, float conf_min) {
  __shared__ DrawLds s;
  const int tid = threadIdx.x;
  const int f = blockIdx.z, b = f / V;                 // frame b * V + v
  const int x0 = blockIdx.x * kDrawTW, y0 = blockIdx.y * kDrawTH;
  const int x1 = (x0 + kDrawTW < Ws ? x0 + kDrawTW : Ws) - 1, y1 = (y0 + kDrawTH < Hs ? y0 + kDrawTH : Hs) - 1;
  draw_begin(s, tid, ids, b, N, P, prm);
  __syncthreads();
  const int x = x0 + (tid & (kDrawTW - 1)), yb = y0 + tid / kDrawTW;      // this thread's pixels: rows yb + 4 r
  unsigned mask[kDrawRows];
  int px[kDrawRows], py[kDrawRows];
#pragma unroll
  for (int r = 0; r < kDrawRows; ++r) {
    mask[r] = 0u;
    px[r] = 16 * x;
    py[r] = 16 * (yb + r * (kDrawThreads / kDrawTW));
  }
  const int NP = N * (J + L);
  for (int base = 0, c = 0; base < NP; base += kDrawThreads, ++c) {
    draw_collect(s, c, base + tid, f, b, views, conf, conf_min, N, J, L, prm, R, W, x0, y0, x1, y1);
    __syncthreads();
    draw_scan(s, c, px, py, mask);
  }
  if (x >= Ws) return;
  const int na = 256 - alpha;
#pragma unroll
  for (int r = 0; r < kDrawRows; ++r) {
    const int y = yb + r * (kDrawThreads / kDrawTW);
    if (mask[r] == 0u || y >= Hs) continue;
    uint8_t* p = frames + ((size_t(f) * Hs + y) * Ws + x) * 3;
    draw_note_read(p);
    int c0 = p[0], c1 = p[1], c2 = p[2];
    for (int n = 0; n < N; ++n)
      if ((mask[r] >> n) & 1u) {
        const unsigned col = s.pcol[n];
        c0 = (int(col & 255u) * alpha + c0 * na + 128) >> 8;
        c1 = (int((col >> 8) & 255u) * alpha + c1 * na + 128) >> 8;
        c2 = (int((col >> 16) & 255u) * alpha + c2 * na + 128) >> 8;
      }
    p[0] = uint8_t(c0);
    p[1] = uint8_t(c1);
    p[2] = uint8_t(c2);
  }
}

// The same overlay on an NV12 surface (fvp_draw_poses_nv12, include/fvp.h): the tile, the lists and the coverage test are
// those of k_draw_poses; a thread owns one 2 x 2 luma quad and the (U, V) pair that serves it, so the chroma's box-filtered
// coverage k_n needs no other lane.  A tile is 32 x 8 quads: a wave holds two quad rows - 64 contiguous luma bytes on each of
// four rows, 64 contiguous chroma bytes on each of two.  Luma goes byte by byte (only covered bytes are touched), a chroma
// pair as one 2-byte load and one 2-byte store.  Tiles start at even coordinates and Hs, Ws are even: a quad is inside the
// frame or outside it as a whole, and no two workgroups touch the same byte.  prm.pal holds (Yc, Uc, Vc).
struct DrawNv12Prm {
  long y_pitch, uv_pitch, y_frame, uv_frame;
};

__global__ void __launch_bounds__(kDrawThreads)
k_draw_poses_nv12(uint8_t* __restrict__ yp, uint8_t* __restrict__ uvp, DrawNv12Prm q, int V, int Hs, int Ws,
                  const float* __restrict__ views, const int32_t* __restrict__ ids, const float* __restrict__ conf, int N,
                  int J, int L, int P, DrawPrm prm, int R, int W, int alpha, float conf_min) {
  __shared__ DrawLds s;
  const int tid = threadIdx.x;
  const int f = blockIdx.z, b = f / V;                 // frame b * V + v
  const int x0 = blockIdx.x * kDrawTW, y0 = blockIdx.y * kDrawTH;
  const int x1 = (x0 + kDrawTW < Ws ? x0 + kDrawTW : Ws) - 1, y1 = (y0 + kDrawTH < Hs ? y0 + kDrawTH : Hs) - 1;
  draw_begin(s, tid, ids, b, N, P, prm);
  __syncthreads();
  const int x = x0 + 2 * (tid & (kDrawTW / 2 - 1)), y = y0 + 2 * (tid / (kDrawTW / 2));      // the quad's top-left pixel
  unsigned mask[4];                                    // pixel e of the quad: (x + (e & 1), y + (e >> 1))
  int px[4], py[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mask[e] = 0u;
    px[e] = 16 * (x + (e & 1));
    py[e] = 16 * (y + (e >> 1));
  }
  const int NP = N * (J + L);
  for (int base = 0, c = 0; base < NP; base += kDrawThreads, ++c) {
    draw_collect(s, c, base + tid, f, b, views, conf, conf_min, N, J, L, prm, R, W, x0, y0, x1, y1);
    __syncthreads();
    draw_scan(s, c, px, py, mask);
  }
  const unsigned any = mask[0] | mask[1] | mask[2] | mask[3];
  if (x >= Ws || y >= Hs || any == 0u) return;
  uint8_t* pl = yp + long(f) * q.y_frame + long(y) * q.y_pitch + x;
  uint16_t* pc = reinterpret_cast<uint16_t*>(uvp + long(f) * q.uv_frame + long(y >> 1) * q.uv_pitch + x);
  int lum[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lum[e] = 0;
    if (mask[e]) {
      const uint8_t* p = pl + (e >> 1) * q.y_pitch + (e & 1);
      draw_note_read(p);
      lum[e] = *p;
    }
  }
  draw_note_read(reinterpret_cast<const uint8_t*>(pc));
  const unsigned w = *pc;
  int u = int(w & 255u), v = int(w >> 8);
  const int na = 256 - alpha;
  for (int n = 0; n < N; ++n)
    if ((any >> n) & 1u) {
      const unsigned col = s.pcol[n];
      const int yc = int(col & 255u) * alpha + 128;
      int k = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((mask[e] >> n) & 1u) {
          lum[e] = (yc + lum[e] * na) >> 8;
          ++k;
        }
      const int a = alpha * k;                         // 1 .. 1024: the share of the quad person n covers
      u = (int((col >> 8) & 255u) * a + u * (1024 - a) + 512) >> 10;
      v = (int((col >> 16) & 255u) * a + v * (1024 - a) + 512) >> 10;
    }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (mask[e]) pl[(e >> 1) * q.y_pitch + (e & 1)] = uint8_t(lum[e]);
  *pc = uint16_t(unsigned(u) | (unsigned(v) << 8));
}

// ---- faces out of the camera frames (fvp_anonymise_rois, fvp_anonymise_rois_nv12; include/fvp.h, ABI 23) --------------------
// The second pair of kernels that WRITE frames.  A workgroup owns a 64 x 32 pixel tile of one frame - whole cells for every
// permitted cell size (2 .. 32), cells being anchored at the frame's origin.  Thread k < rois_per_frame loads ROI k of the
// frame, derives the ellipse's terms and decides whether the ROI can cover a pixel of the tile (RECT: the box against the
// tile's pixel centres; ELLIPSE: the tile pixel nearest the centre - every fp32 operation of the coverage test is monotone in
// |dx| and in |dy|, so that pixel is covered whenever any pixel of the tile is); a tile no ROI meets leaves, uniformly, before
// any frame address is formed.  Otherwise: coverage of the thread's pixels (a bit per pixel, in registers), the touched cells
// marked in LDS, barrier, the ORIGINAL bytes of every in-frame pixel of a touched cell summed into LDS (integer adds commute:
// the sums do not depend on the schedule), barrier, the covered pixels written.  IN PLACE IS SAFE BECAUSE every read of a cell
// precedes that last barrier, every write follows it, and both happen in the one workgroup that owns the cell; no two
// workgroups touch the same byte.  FILL reads no frame byte and needs neither LDS sums nor the two barriers.
constexpr int kAnonTW = 64, kAnonTH = 32, kAnonThreads = 256, kAnonMaxRois = 64;
constexpr int kAnonRows = kAnonTH / (kAnonThreads / kAnonTW);                         // pixels (rows) per thread, RGB
constexpr int kAnonMaxCells = (kAnonTW / 2) * (kAnonTH / 2);                          // cell == 2

struct AnonLds {
  float box[kAnonMaxRois][4];                          // x0, y0, x1, y1
  float ell[kAnonMaxRois][5];                          // cx, cy, hw * hw, hh * hh, (hw * hw) * (hh * hh)
  int meets[kAnonMaxRois];                             // active, and may cover a pixel of this tile
  int touched[kAnonMaxCells];
  int sum[kAnonMaxCells][3];                           // R, G, B or Y, U, V
};

// include/fvp.h, "Coverage"; this TU is compiled with -ffp-contract=off: every * + - is rounded on its own
__device__ __forceinline__ bool anon_covers(const AnonLds& s, int k, int shape, float xc, float yc) {
  if (shape == FVP_ANON_RECT) return s.box[k][0] <= xc && xc < s.box[k][2] && s.box[k][1] <= yc && yc < s.box[k][3];
  const float dx = xc - s.ell[k][0], dy = yc - s.ell[k][1];
  return (dx * dx) * s.ell[k][3] + (dy * dy) * s.ell[k][2] <= s.ell[k][4];
}

// Before the first barrier: thread k takes ROI k of frame f against the tile's in-frame pixels [tx0, tx1] x [ty0, ty1]
__device__ __forceinline__ void anon_begin(AnonLds& s, int tid, const float* __restrict__ rois, int f, int rpf, int shape,
                                           int tx0, int ty0, int tx1, int ty1) {
  if (tid >= rpf) return;
  const float* r = rois + 4 * (long(f) * rpf + tid);
  const float x0 = r[0], y0 = r[1], x1 = r[2], y1 = r[3];
  const float big = 65536.0f;                            // a NaN or an Inf fails the compare
  const bool active = fabsf(x0) <= big && fabsf(y0) <= big && fabsf(x1) <= big && fabsf(y1) <= big && x1 > x0 && y1 > y0;
  const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f, hw = (x1 - x0) * 0.5f, hh = (y1 - y0) * 0.5f;
  const float hw2 = hw * hw, hh2 = hh * hh;
  s.box[tid][0] = x0;
  s.box[tid][1] = y0;
  s.box[tid][2] = x1;
  s.box[tid][3] = y1;
  s.ell[tid][0] = cx;
  s.ell[tid][1] = cy;
  s.ell[tid][2] = hw2;
  s.ell[tid][3] = hh2;
  s.ell[tid][4] = hw2 * hh2;
  bool meets = false;
  if (active) {
    if (shape == FVP_ANON_RECT) {
      meets = x1 > float(tx0) + 0.5f && x0 <= float(tx1) + 0.5f && y1 > float(ty0) + 0.5f && y0 <= float(ty1) + 0.5f;
    } else {                                             // |cx|, |cy| <= 65536: the conversions are exact
      const int fx = int(floorf(cx)), fy = int(floorf(cy));
      const int xn = fx < tx0 ? tx0 : fx > tx1 ? tx1 : fx, yn = fy < ty0 ? ty0 : fy > ty1 ? ty1 : fy;
      const float dx = (float(xn) + 0.5f) - cx, dy = (float(yn) + 0.5f) - cy;
      meets = (dx * dx) * hh2 + (dy * dy) * hw2 <= hw2 * hh2;
    }
  }
  s.meets[tid] = meets ? 1 : 0;
}

// m = (2 S + n) / (2 n): the mean of n bytes, half up; S <= 1024 * 255
__device__ __forceinline__ int anon_mean(int S, int n) { return (2 * S + n) / (2 * n); }

// in-frame pixels of the cell that holds pixel p along an axis of extent `size`
__device__ __forceinline__ int anon_extent(int p, int sh, int size) {
  const int a = (p >> sh) << sh, b = a + (1 << sh);
  return (b < size ? b : size) - a;
}

__global__ void __launch_bounds__(kAnonThreads)
k_anonymise_rois(uint8_t* __restrict__ frames, int Hs, int Ws, const float* __restrict__ rois, int rpf, int sh, int shape,
                 int mode, unsigned colour) {
  __shared__ AnonLds s;
  const int tid = threadIdx.x, f = blockIdx.z;
  const int tx0 = blockIdx.x * kAnonTW, ty0 = blockIdx.y * kAnonTH;
  const int tx1 = (tx0 + kAnonTW < Ws ? tx0 + kAnonTW : Ws) - 1, ty1 = (ty0 + kAnonTH < Hs ? ty0 + kAnonTH : Hs) - 1;
  anon_begin(s, tid, rois, f, rpf, shape, tx0, ty0, tx1, ty1);
  __syncthreads();
  const int lx = tid & (kAnonTW - 1), ly = tid / kAnonTW;        // this thread's pixels: (lx, ly + 4 r) of the tile
  const int x = tx0 + lx;
  const float xc = float(x) + 0.5f;
  unsigned cov = 0u;
  bool any = false;
  for (int k = 0; k < rpf; ++k) {
    if (!s.meets[k]) continue;                         // uniform over the workgroup
    any = true;
#pragma unroll
    for (int r = 0; r < kAnonRows; ++r)
      if (anon_covers(s, k, shape, xc, float(ty0 + ly + 4 * r) + 0.5f)) cov |= 1u << r;
  }
  if (!any) return;                                    // uniform: no frame address has been formed
#pragma unroll
  for (int r = 0; r < kAnonRows; ++r)
    if (x >= Ws || ty0 + ly + 4 * r >= Hs) cov &= ~(1u << r);
  uint8_t* fr = frames + size_t(f) * Hs * Ws * 3;
  if (mode == FVP_ANON_FILL) {
#pragma unroll
    for (int r = 0; r < kAnonRows; ++r)
      if ((cov >> r) & 1u) {
        uint8_t* p = fr + (size_t(ty0 + ly + 4 * r) * Ws + x) * 3;
        p[0] = uint8_t(colour & 255u);
        p[1] = uint8_t((colour >> 8) & 255u);
        p[2] = uint8_t((colour >> 16) & 255u);
      }
    return;
  }
  const int ncw = kAnonTW >> sh, cells = ncw * (kAnonTH >> sh);
  for (int i = tid; i < cells; i += kAnonThreads) {
    s.touched[i] = 0;
    s.sum[i][0] = 0;
    s.sum[i][1] = 0;
    s.sum[i][2] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kAnonRows; ++r)
    if ((cov >> r) & 1u) s.touched[((ly + 4 * r) >> sh) * ncw + (lx >> sh)] = 1;
  __syncthreads();
  {                                                    // a thread's pixels share a column: consecutive ones of a cell are summed in registers
    int cur = -1, a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int r = 0; r < kAnonRows; ++r) {
      const int y = ty0 + ly + 4 * r, ci = ((ly + 4 * r) >> sh) * ncw + (lx >> sh);
      if (x >= Ws || y >= Hs || !s.touched[ci]) continue;
      if (ci != cur) {
        if (cur >= 0) {
          atomicAdd(&s.sum[cur][0], a0);
          atomicAdd(&s.sum[cur][1], a1);
          atomicAdd(&s.sum[cur][2], a2);
        }
        cur = ci;
        a0 = a1 = a2 = 0;
      }
      const uint8_t* p = fr + (size_t(y) * Ws + x) * 3;
      draw_note_read(p);
      a0 += p[0];
      a1 += p[1];
      a2 += p[2];
    }
    if (cur >= 0) {
      atomicAdd(&s.sum[cur][0], a0);
      atomicAdd(&s.sum[cur][1], a1);
      atomicAdd(&s.sum[cur][2], a2);
    }
  }
  __syncthreads();                                     // every read of the tile's cells is behind us
  if (cov == 0u) return;
  const int cw = anon_extent(x, sh, Ws);
#pragma unroll
  for (int r = 0; r < kAnonRows; ++r)
    if ((cov >> r) & 1u) {
      const int y = ty0 + ly + 4 * r, ci = ((ly + 4 * r) >> sh) * ncw + (lx >> sh);
      const int n = cw * anon_extent(y, sh, Hs);
      uint8_t* p = fr + (size_t(y) * Ws + x) * 3;
      p[0] = uint8_t(anon_mean(s.sum[ci][0], n));
      p[1] = uint8_t(anon_mean(s.sum[ci][1], n));
      p[2] = uint8_t(anon_mean(s.sum[ci][2], n));
    }
}

// The same on an NV12 surface: the tile, the ROI list and the coverage test are those of k_anonymise_rois; a thread owns two
// 2 x 2 luma quads (16 luma rows apart) and the (U, V) pair that serves each, as in k_draw_poses_nv12.  Cells and tiles start
// at even coordinates and Hs, Ws are even: a quad lies in one cell, and inside the frame or outside it as a whole; the chroma
// cell of a luma cell is the pairs of its quads.  Luma goes byte by byte, a pair as one 2-byte load and one 2-byte store.
// `colour` holds (Yc, Uc, Vc).
constexpr int kAnonQuads = (kAnonTW / 2) * (kAnonTH / 2) / kAnonThreads;              // quads per thread

__global__ void __launch_bounds__(kAnonThreads)
k_anonymise_rois_nv12(uint8_t* __restrict__ yp, uint8_t* __restrict__ uvp, DrawNv12Prm q, int Hs, int Ws,
                      const float* __restrict__ rois, int rpf, int sh, int shape, int mode, unsigned colour) {
  __shared__ AnonLds s;
  const int tid = threadIdx.x, f = blockIdx.z;
  const int tx0 = blockIdx.x * kAnonTW, ty0 = blockIdx.y * kAnonTH;
  const int tx1 = (tx0 + kAnonTW < Ws ? tx0 + kAnonTW : Ws) - 1, ty1 = (ty0 + kAnonTH < Hs ? ty0 + kAnonTH : Hs) - 1;
  anon_begin(s, tid, rois, f, rpf, shape, tx0, ty0, tx1, ty1);
  __syncthreads();
  const int lx = 2 * (tid & (kAnonTW / 2 - 1)), ly = 2 * (tid / (kAnonTW / 2));      // quad r: top-left (lx, ly + 16 r) of the tile
  const int x = tx0 + lx;
  unsigned cov = 0u;                                   // bit 4 r + e: pixel (x + (e & 1), y_r + (e >> 1))
  bool any = false;
  for (int k = 0; k < rpf; ++k) {
    if (!s.meets[k]) continue;                         // uniform over the workgroup
    any = true;
#pragma unroll
    for (int i = 0; i < 4 * kAnonQuads; ++i)
      if (anon_covers(s, k, shape, float(x + (i & 1)) + 0.5f, float(ty0 + ly + 16 * (i >> 2) + ((i >> 1) & 1)) + 0.5f))
        cov |= 1u << i;
  }
  if (!any) return;                                    // uniform: no surface address has been formed
#pragma unroll
  for (int r = 0; r < kAnonQuads; ++r)
    if (x >= Ws || ty0 + ly + 16 * r >= Hs) cov &= ~(15u << (4 * r));
  uint8_t* fy = yp + long(f) * q.y_frame;
  uint8_t* fuv = uvp + long(f) * q.uv_frame;
  if (mode == FVP_ANON_FILL) {
#pragma unroll
    for (int r = 0; r < kAnonQuads; ++r) {
      const unsigned c4 = (cov >> (4 * r)) & 15u;
      if (!c4) continue;
      const int y = ty0 + ly + 16 * r;
      uint8_t* pl = fy + long(y) * q.y_pitch + x;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((c4 >> e) & 1u) pl[(e >> 1) * q.y_pitch + (e & 1)] = uint8_t(colour & 255u);
      *reinterpret_cast<uint16_t*>(fuv + long(y >> 1) * q.uv_pitch + x) = uint16_t(colour >> 8);
    }
    return;
  }
  const int ncw = kAnonTW >> sh, cells = ncw * (kAnonTH >> sh);
  for (int i = tid; i < cells; i += kAnonThreads) {
    s.touched[i] = 0;
    s.sum[i][0] = 0;
    s.sum[i][1] = 0;
    s.sum[i][2] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kAnonQuads; ++r)
    if ((cov >> (4 * r)) & 15u) s.touched[((ly + 16 * r) >> sh) * ncw + (lx >> sh)] = 1;
  __syncthreads();
  {
    int cur = -1, a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int r = 0; r < kAnonQuads; ++r) {
      const int y = ty0 + ly + 16 * r, ci = ((ly + 16 * r) >> sh) * ncw + (lx >> sh);
      if (x >= Ws || y >= Hs || !s.touched[ci]) continue;
      if (ci != cur) {
        if (cur >= 0) {
          atomicAdd(&s.sum[cur][0], a0);
          atomicAdd(&s.sum[cur][1], a1);
          atomicAdd(&s.sum[cur][2], a2);
        }
        cur = ci;
        a0 = a1 = a2 = 0;
      }
      const uint8_t* pl = fy + long(y) * q.y_pitch + x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint8_t* p = pl + (e >> 1) * q.y_pitch + (e & 1);
        draw_note_read(p);
        a0 += *p;
      }
      const uint8_t* pc = fuv + long(y >> 1) * q.uv_pitch + x;
      draw_note_read(pc);
      const unsigned w = *reinterpret_cast<const uint16_t*>(pc);
      a1 += int(w & 255u);
      a2 += int(w >> 8);
    }
    if (cur >= 0) {
      atomicAdd(&s.sum[cur][0], a0);
      atomicAdd(&s.sum[cur][1], a1);
      atomicAdd(&s.sum[cur][2], a2);
    }
  }
  __syncthreads();                                     // every read of the tile's cells is behind us
  if (cov == 0u) return;
  const int cw = anon_extent(x, sh, Ws);
#pragma unroll
  for (int r = 0; r < kAnonQuads; ++r) {
    const unsigned c4 = (cov >> (4 * r)) & 15u;
    if (!c4) continue;
    const int y = ty0 + ly + 16 * r, ci = ((ly + 16 * r) >> sh) * ncw + (lx >> sh);
    const int n = cw * anon_extent(y, sh, Hs);         // luma pixels of the cell; its pairs: n / 4
    const int my = anon_mean(s.sum[ci][0], n), mu = anon_mean(s.sum[ci][1], n >> 2), mv = anon_mean(s.sum[ci][2], n >> 2);
    uint8_t* pl = fy + long(y) * q.y_pitch + x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((c4 >> e) & 1u) pl[(e >> 1) * q.y_pitch + (e & 1)] = uint8_t(my);
    *reinterpret_cast<uint16_t*>(fuv + long(y >> 1) * q.uv_pitch + x) = uint16_t(unsigned(mu) | (unsigned(mv) << 8));
  }
}

// ---- person crops out (fvp_person_rois, fvp_crop_rois, fvp_crop_rois_nv12; include/fvp.h, ABI 16) -----------------------
// One box per (frame, view, person) from the per-view pixels of fvp_joint_evidence: one thread per box walks the person's
// joints in ascending order (min / max of the usable ones, their count, the sum of their heatmap samples).  A few hundred
// boxes of at most 32 joints: launch latency, nothing to tune.  A usable joint is a drawable joint of the overlay
// (draw_joint's compares, restated on the floats) whose mask bit is set.
struct RoiPrm {
  uint32_t mask;
  int min_joints;
  float scale, pad_px, aspect, conf_min;
};

__global__ void __launch_bounds__(64)
k_person_rois(const float* __restrict__ views, const int32_t* __restrict__ ids, const float* __restrict__ conf, int total,
              int V, int N, int J, RoiPrm p, float* __restrict__ rois, int32_t* __restrict__ roi_count,
              float* __restrict__ roi_score) {
  const int i = blockIdx.x * 64 + threadIdx.x;          // box (f = b * V + v, n)
  if (i >= total) return;
  const int f = i / N, n = i - f * N, b = f / V;
  const bool selected = !ids || ids[long(b) * N + n] >= 0;
  int k = 0;
  float xmin = 0.0f, xmax = 0.0f, ymin = 0.0f, ymax = 0.0f, sum = 0.0f;
  if (selected) {
    const float* vj = views + long(i) * J * 4;
    const float* cj = conf ? conf + (long(b) * N + n) * J : nullptr;
    for (int j = 0; j < J; ++j) {
      if (!((p.mask >> j) & 1u)) continue;
      const float px = vj[4 * j], py = vj[4 * j + 1], depth = vj[4 * j + 2];
      bool ok = depth > 0.0f && fabsf(px) <= 32768.0f && fabsf(py) <= 32768.0f;
      if (cj) ok = ok && cj[j] >= p.conf_min;
      if (!ok) continue;
      if (k == 0) {
        xmin = xmax = px;
        ymin = ymax = py;
      } else {
        xmin = px < xmin ? px : xmin;
        xmax = px > xmax ? px : xmax;
        ymin = py < ymin ? py : ymin;
        ymax = py > ymax ? py : ymax;
      }
      sum = sum + vj[4 * j + 3];
      ++k;
    }
  }
  const bool valid = selected && k >= p.min_joints;
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f, sc = 0.0f;
  if (valid) {
    const float cx = (xmin + xmax) * 0.5f, cy = (ymin + ymax) * 0.5f;
    float hw = ((xmax - xmin) * 0.5f) * p.scale + p.pad_px, hh = ((ymax - ymin) * 0.5f) * p.scale + p.pad_px;
    if (hw < hh * p.aspect)
      hw = hh * p.aspect;
    else
      hh = __fdiv_rn(hw, p.aspect);
    r0 = cx - hw;
    r1 = cy - hh;
    r2 = cx + hw;
    r3 = cy + hh;
    sc = __fdiv_rn(sum, float(k));
  }
  if (rois) {
    float* o = rois + long(i) * 4;
    o[0] = r0;
    o[1] = r1;
    o[2] = r2;
    o[3] = r3;
  }
  if (roi_count) roi_count[i] = valid ? k : 0;
  if (roi_score) roi_score[i] = sc;
}

// Crop + resize: ROI r (blockIdx.x, a grid dimension of its own) of frame r / rois_per_frame -> an h x w patch.  The ROI's
// four floats and the matrix derived from them are the same for every lane of the workgroup (scalar loads), and from the
// matrix on the arithmetic IS ingest_pair: one lane per destination pixel pair, one 16-byte store.  A workgroup of a
// non-croppable ROI stores zeros and returns before any frame address is formed.
__device__ __forceinline__ bool crop_matrix(const float* __restrict__ rois, int r, int h, int w, float (&inv)[6]) {
  const float x0 = rois[4 * long(r)], y0 = rois[4 * long(r) + 1], x1 = rois[4 * long(r) + 2], y1 = rois[4 * long(r) + 3];
  const float big = 3.402823466e+38f;                    // FLT_MAX: a NaN or an Inf fails the compare
  if (!(fabsf(x0) <= big && fabsf(y0) <= big && fabsf(x1) <= big && fabsf(y1) <= big && x1 > x0 && y1 > y0)) return false;
  const float ax = __fdiv_rn(x1 - x0, float(w)), ay = __fdiv_rn(y1 - y0, float(h));
  inv[0] = ax;
  inv[1] = 0.0f;
  inv[2] = (x0 + 0.5f * ax) - 0.5f;                      // pixel centres map to pixel centres
  inv[3] = 0.0f;
  inv[4] = ay;
  inv[5] = (y0 + 0.5f * ay) - 0.5f;
  return true;
}

__device__ __forceinline__ void crop_zero_pair(int h, int w, int r, int y, int xp, uint16_t* __restrict__ nhwc8,
                                               float* __restrict__ nchw) {
  if (nchw) {
    const long hw = long(h) * w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = nchw + (long(r) * 3 + c) * hw + long(y) * w + 2 * xp;
      o[0] = 0.0f;
      o[1] = 0.0f;
    }
  }
  if (nhwc8) *reinterpret_cast<IngestB16*>(nhwc8 + ((long(r) * h + y) * (w / 2) + xp) * 8) = IngestB16{{0u, 0u, 0u, 0u}};
}

struct CropNorm {
  float mean[3], stdv[3];
};

__global__ void __launch_bounds__(256)
k_crop_rois(const uint8_t* __restrict__ frames, int Hs, int Ws, const float* __restrict__ rois, int rpf, CropNorm nm, int h,
            int w, int swap, uint16_t* __restrict__ nhwc8, float* __restrict__ nchw) {
  const int r = blockIdx.x;                              // the ROI: uniform over the workgroup
  const int i = int(blockIdx.y) * 256 + threadIdx.x;     // one thread per pixel PAIR of the patch
  const int w2 = w / 2;
  if (i >= h * w2) return;
  const int y = i / w2, xp = i - y * w2;
  IngestPrm p;
  if (!crop_matrix(rois, r, h, w, p.inv)) {
    crop_zero_pair(h, w, r, y, xp, nhwc8, nchw);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = nm.mean[c];
    p.stdv[c] = nm.stdv[c];
  }
  const uint8_t* f = frames + long(r / rpf) * Hs * Ws * 3;
  const int c0 = swap ? 2 : 0, c2 = 2 - c0;
  ingest_pair(p, Hs, Ws, h, w, r, y, xp, nhwc8, nchw, [&](int yy, int xx) {
    const uint8_t* q = f + (long(yy) * Ws + xx) * 3;
    draw_note_read(q);
    return IngestPx{{float(q[c0]), float(q[1]), float(q[c2])}};
  });
}

__global__ void __launch_bounds__(256)
k_crop_rois_nv12(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp, int Hs, int Ws, Nv12Prm q,
                 const float* __restrict__ rois, int rpf, CropNorm nm, int h, int w, uint16_t* __restrict__ nhwc8,
                 float* __restrict__ nchw) {
  const int r = blockIdx.x;                              // the ROI: uniform over the workgroup
  const int i = int(blockIdx.y) * 256 + threadIdx.x;     // one thread per pixel PAIR of the patch
  const int w2 = w / 2;
  if (i >= h * w2) return;
  const int y = i / w2, xp = i - y * w2;
  IngestPrm p;
  if (!crop_matrix(rois, r, h, w, p.inv)) {
    crop_zero_pair(h, w, r, y, xp, nhwc8, nchw);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = nm.mean[c];
    p.stdv[c] = nm.stdv[c];
  }
  const uint8_t* fy = yp + long(r / rpf) * q.y_frame;
  const uint8_t* fuv = uvp + long(r / rpf) * q.uv_frame;
  ingest_pair(p, Hs, Ws, h, w, r, y, xp, nhwc8, nchw, [&](int yy, int xx) {   // the tap of k_ingest_nv12
    const uint8_t* pl = fy + long(yy) * q.y_pitch + xx;
    const uint8_t* pc = fuv + long(yy >> 1) * q.uv_pitch + 2 * (xx >> 1);
    draw_note_read(pl);
    draw_note_read(pc);
    const int luma = *pl;
    const uint32_t wd = *reinterpret_cast<const uint16_t*>(pc);
    const int c = luma > q.yoff ? luma - q.yoff : 0, d = int(wd & 0xffu) - 128, e = int(wd >> 8) - 128;
    const int l = q.cy * c + (1 << 19);
    return IngestPx{{ingest_clip8(l + q.crv * e), ingest_clip8(l + q.cgu * d + q.cgv * e), ingest_clip8(l + q.cbu * d)}};
  });
}

// ---- person signature (fvp_person_signature; include/fvp.h, ABI 20) -------------------------------------------------------
// A colour histogram per person and body part from the frame pixels under the person's limbs.  One workgroup per (b, n): item
// (v, l, m) - sample m of limb l in view v - is strided over the threads, each tests its limb's two joints (draw_joint's
// compares, restated on the floats, and the occluder table), interpolates, rounds and reads ONE pixel; the P x 64 counters sit
// in LDS behind integer atomics, so the result does not depend on the order, and go out coalesced.  V * L * K <= 16384 items of
// a few dependent loads each: latency-bound, nothing is tuned.  The limb tables are kernel arguments (SGPRs / the kernarg
// segment), as the overlay's are; no per-thread array exists, so nothing can become scratch.
struct SigPrm {
  uint8_t limb[64][2];
  uint8_t part[64];
};
constexpr int kSigThreads = 256, kSigMaxL = 64, kSigMaxK = 32;

__device__ __forceinline__ bool sig_joint(const float* __restrict__ views, const float* __restrict__ conf,
                                          const int32_t* __restrict__ occ, float conf_min, long vj, long cj, float& px,
                                          float& py) {
  px = views[4 * vj];
  py = views[4 * vj + 1];
  bool ok = views[4 * vj + 2] > 0.0f && fabsf(px) <= 32768.0f && fabsf(py) <= 32768.0f;
  if (conf) ok = ok && conf[cj] >= conf_min;
  if (occ) ok = ok && occ[vj] == -1;
  return ok;
}

__global__ void __launch_bounds__(kSigThreads)
k_person_signature(const uint8_t* __restrict__ frames, int V, int Hs, int Ws, const float* __restrict__ views,
                   const int32_t* __restrict__ ids, const float* __restrict__ conf, const int32_t* __restrict__ occ, int N,
                   int J, int L, int P, int K, SigPrm prm, float conf_min, int32_t* __restrict__ sig,
                   int32_t* __restrict__ sig_count) {
  __shared__ int s_hist[FVP_SIG_MAX_PARTS * FVP_SIG_BINS];
  const int bn = blockIdx.x, b = bn / N, n = bn - b * N, tid = threadIdx.x;
  const int cells = P * FVP_SIG_BINS;
  if (tid < cells) s_hist[tid] = 0;                      // cells <= kSigThreads
  __syncthreads();
  if (!ids || ids[bn] >= 0) {                            // uniform over the workgroup
    const int LK = L * K, items = V * LK;
    const float fK = float(K);
    const long crow = long(bn) * J;
#pragma unroll 1
    for (int it = tid; it < items; it += kSigThreads) {
      const int v = it / LK, r = it - v * LK, l = r / K, m = r - l * K;
      const long f = long(b) * V + v, vrow = (f * N + n) * J;
      const int j0 = prm.limb[l][0], j1 = prm.limb[l][1];
      float ax, ay, bx, by;
      const bool ok0 = sig_joint(views, conf, occ, conf_min, vrow + j0, crow + j0, ax, ay);
      const bool ok1 = sig_joint(views, conf, occ, conf_min, vrow + j1, crow + j1, bx, by);
      if (!(ok0 && ok1)) continue;
      const float t = __fdiv_rn(__fadd_rn(float(m), 0.5f), fK);
      const float x = __fadd_rn(ax, __fmul_rn(t, __fsub_rn(bx, ax))), y = __fadd_rn(ay, __fmul_rn(t, __fsub_rn(by, ay)));
      const int xi = int(rintf(x)), yi = int(rintf(y));  // |x|, |y| <= 32768: the conversion is exact; round-half-even
      if (xi < 0 || xi >= Ws || yi < 0 || yi >= Hs) continue;
      const uint8_t* p = frames + ((f * Hs + yi) * Ws + xi) * 3;
      draw_note_read(p);
      const int bin = (p[0] >> 6) * 16 + (p[1] >> 6) * 4 + (p[2] >> 6);
      atomicAdd(&s_hist[prm.part[l] * FVP_SIG_BINS + bin], 1);
    }
  }
  __syncthreads();
  if (sig && tid < cells) sig[long(bn) * cells + tid] = s_hist[tid];
  if (sig_count && tid < P) {
    int c = 0;
#pragma unroll 1
    for (int i = 0; i < FVP_SIG_BINS; ++i) c += s_hist[tid * FVP_SIG_BINS + i];
    sig_count[long(bn) * P + tid] = c;
  }
}

}  // namespace fvp

using namespace fvp;

extern "C" int fvp_rasterise_heatmaps(const double* joints, const int32_t* num_people, int nimg, int P, int J, int W,
                                      int H, double feat_stride_x, double feat_stride_y, double sigma,
                                      float* heat_nchw, float* heat_cl, int JP, fvp_stream_t s) {
  FVP_REQUIRE(joints && num_people && (heat_nchw || heat_cl) && nimg >= 0 && P >= 0 && J > 0 && W > 0 && H > 0);
  FVP_REQUIRE(feat_stride_x > 0 && feat_stride_y > 0 && sigma > 0 && (!heat_cl || JP >= J));
  FVP_REQUIRE(std::isfinite(feat_stride_x) && std::isfinite(feat_stride_y) && std::isfinite(sigma));
  if (nimg == 0) return 0;
  FVP_LIMIT(size_t(J) * W * sizeof(float) <= 32 * 1024 && P <= 64 && P * J <= 1024);
  int RB = 4;                                          // rows per band: the band of all joints fits 64 KB of LDS
  while (RB > 1 && size_t(J) * RB * W * sizeof(float) > 44 * 1024) RB >>= 1;   // + 18 KB of static LDS
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_rasterise, dim3(ceil_div(H, RB), nimg), dim3(256), size_t(J) * RB * W * sizeof(float),
                     as_stream(s), joints, num_people, P, J, W, H, RB, feat_stride_x, feat_stride_y, sigma, heat_nchw,
                     heat_cl, JP);
  return launch_status();
}

extern "C" int fvp_ingest_frames(const uint8_t* frames, int N, int Hs, int Ws, const float inv[6], const float mean[3],
                                 const float stdv[3], int H, int W, int flags, uint16_t* nhwc8, float* nchw,
                                 fvp_stream_t s) {
  FVP_REQUIRE(frames && inv && mean && stdv && (nhwc8 || nchw));
  FVP_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && W % 2 == 0);
  FVP_REQUIRE((flags & ~(FVP_INGEST_SWAP_RB | FVP_INGEST_GENERAL)) == 0);
  IngestPrm p;
  for (int i = 0; i < 6; ++i) {
    FVP_REQUIRE(std::isfinite(inv[i]));
    p.inv[i] = inv[i];
  }
  for (int c = 0; c < 3; ++c) {
    FVP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdv[c]) && stdv[c] != 0.0f);
    p.mean[c] = mean[c];
    p.stdv[c] = stdv[c];
  }
  if (N == 0) return 0;
  FVP_LIMIT(Hs < (1 << 24) && Ws < (1 << 24) && H < (1 << 24) && W < (1 << 24));   // pixel indices exact in fp32
  const int swap = (flags & FVP_INGEST_SWAP_RB) ? 1 : 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  const long pairs = long(N) * H * (W / 2);
  FVP_LIMIT((pairs + 255) / 256 < (1l << 31));
  hipLaunchKernelGGL(k_ingest_gather, dim3(unsigned((pairs + 255) / 256)), dim3(256), 0, as_stream(s), frames, N, Hs, Ws,
                     p, H, W, swap, nhwc8, nchw);
  return launch_status();
}

extern "C" int fvp_ingest_nv12(const uint8_t* y, const uint8_t* uv, int N, int Hs, int Ws, long y_pitch, long uv_pitch,
                               long y_frame_stride, long uv_frame_stride, int standard, const float inv[6],
                               const float mean[3], const float stdv[3], int H, int W, uint16_t* nhwc8, float* nchw,
                               fvp_stream_t s) {
  static const int coeffs[4][6] = {FVP_YUV_BT601_LIMITED_COEFFS, FVP_YUV_BT709_LIMITED_COEFFS, FVP_YUV_BT601_FULL_COEFFS,
                                   FVP_YUV_BT709_FULL_COEFFS};
  FVP_REQUIRE(y && uv && inv && mean && stdv && (nhwc8 || nchw));
  FVP_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hs % 2 == 0 && Ws % 2 == 0 && W % 2 == 0);
  FVP_REQUIRE(y_pitch >= Ws && uv_pitch >= Ws);
  // a (U, V) pair is one 2-byte load
  FVP_REQUIRE(uv_pitch % 2 == 0 && uv_frame_stride % 2 == 0 && reinterpret_cast<uintptr_t>(uv) % 2 == 0);
  FVP_REQUIRE(standard >= 0 && standard < 4);
  IngestPrm p;
  for (int i = 0; i < 6; ++i) {
    FVP_REQUIRE(std::isfinite(inv[i]));
    p.inv[i] = inv[i];
  }
  for (int c = 0; c < 3; ++c) {
    FVP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdv[c]) && stdv[c] != 0.0f);
    p.mean[c] = mean[c];
    p.stdv[c] = stdv[c];
  }
  if (N == 0) return 0;
  FVP_LIMIT(Hs < (1 << 24) && Ws < (1 << 24) && H < (1 << 24) && W < (1 << 24));   // pixel indices exact in fp32
  const int* k = coeffs[standard];
  const Nv12Prm q = {y_pitch, uv_pitch, y_frame_stride, uv_frame_stride, k[0], k[1], k[2], k[3], k[4], k[5]};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  const long pairs = long(N) * H * (W / 2);
  FVP_LIMIT((pairs + 255) / 256 < (1l << 31));
  hipLaunchKernelGGL(k_ingest_nv12, dim3(unsigned((pairs + 255) / 256)), dim3(256), 0, as_stream(s), y, uv, N, Hs, Ws, q,
                     p, H, W, nhwc8, nchw);
  return launch_status();
}

// The dispatch rule of fvp_ingest_bayer, a function of inv, H, W, Hs, Ws only: a bound RW x RH on the source rectangle of
// every 64 x 8 destination tile as k_ingest_bayer_lds lays it out, and whether it fits the LDS budget.  Per axis the taps of
// a tile span at most floor(|a| (tw - 1) + |b| (th - 1) + 2 err) + 3 pixels: the exact spread, err for the (at most four)
// fp32 roundings of a coordinate of magnitude <= M, one for the floors, one for the second tap; never more than the frame.
// The rectangle starts at a multiple of 4 (2 in y) and ends on one: + 3 and rounded up (+ 1 and rounded up).
constexpr size_t kBayerLdsBytes = 47 * 1024;
static bool bayer_lds_plan(const float inv[6], int H, int W, int Hs, int Ws, int* RW, int* RH) {
  int dims[2];
  const int tw = (W < kBayerDW ? W : kBayerDW) - 1, th = (H < kBayerDH ? H : kBayerDH) - 1;
  for (int a = 0; a < 2; ++a) {
    const double ka = std::fabs(double(inv[3 * a])), kb = std::fabs(double(inv[3 * a + 1]));
    const double M = ka * (W - 1) + kb * (H - 1) + std::fabs(double(inv[3 * a + 2]));
    const double e = std::floor(ka * tw + kb * th + 2.0 * (5.0 * M * 0x1p-24)) + 3.0;
    const int n = a ? Hs : Ws;
    dims[a] = e < double(n) ? int(e) : n;
  }
  *RW = (dims[0] + 6) & ~3;
  *RH = (dims[1] + 2) & ~1;
  return size_t(*RH) * size_t(*RW) * 4 + size_t(*RH + 4) * size_t(*RW + 8) <= kBayerLdsBytes;
}

// argument checks both Bayer exports share
static int bayer_args(const uint8_t* raw, int N, int Hs, int Ws, long pitch, int pattern) {
  FVP_REQUIRE(raw && N >= 0 && Hs >= 4 && Ws >= 4 && Hs % 2 == 0 && Ws % 2 == 0 && pitch >= Ws);
  FVP_REQUIRE(pattern >= FVP_BAYER_RGGB && pattern <= FVP_BAYER_BGGR);
  return 0;
}

extern "C" int fvp_demosaic_bayer(const uint8_t* raw, int N, int Hs, int Ws, long pitch, long frame_stride, int pattern,
                                  const uint8_t* tone, int flags, uint8_t* rgb, fvp_stream_t s) {
  if (int rc = bayer_args(raw, N, Hs, Ws, pitch, pattern)) return rc;
  FVP_REQUIRE(rgb && flags == 0);
  if (N == 0) return 0;
  FVP_LIMIT(Hs <= 16384 && Ws <= 16384);
  const int tiles_x = ceil_div(Ws, kBayerTW), tiles_y = ceil_div(Hs, kBayerTH);
  const long blocks = long(tiles_x) * tiles_y * N;
  FVP_LIMIT(blocks < (1l << 31));
  const BayerPrm q = {pitch, frame_stride, pattern & 1, pattern >> 1};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_demosaic_bayer, dim3(unsigned(blocks)), dim3(256), 0, as_stream(s), raw, Hs, Ws, q, tone, tiles_x,
                     tiles_y, rgb);
  return launch_status();
}

extern "C" int fvp_ingest_bayer(const uint8_t* raw, int N, int Hs, int Ws, long pitch, long frame_stride, int pattern,
                                const uint8_t* tone, const float inv[6], const float mean[3], const float stdv[3], int H,
                                int W, uint16_t* nhwc8, float* nchw, fvp_stream_t s) {
  if (int rc = bayer_args(raw, N, Hs, Ws, pitch, pattern)) return rc;
  FVP_REQUIRE(inv && mean && stdv && (nhwc8 || nchw) && H > 0 && W > 0 && W % 2 == 0);
  IngestPrm p;
  for (int i = 0; i < 6; ++i) {
    FVP_REQUIRE(std::isfinite(inv[i]));
    p.inv[i] = inv[i];
  }
  for (int c = 0; c < 3; ++c) {
    FVP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdv[c]) && stdv[c] != 0.0f);
    p.mean[c] = mean[c];
    p.stdv[c] = stdv[c];
  }
  if (N == 0) return 0;
  FVP_LIMIT(Hs < (1 << 24) && Ws < (1 << 24) && H < (1 << 24) && W < (1 << 24));   // pixel indices exact in fp32
  const BayerPrm q = {pitch, frame_stride, pattern & 1, pattern >> 1};
  const long pairs = long(N) * H * (W / 2);
  FVP_LIMIT((pairs + 255) / 256 < (1l << 31));
  int RW = 0, RH = 0;
  const bool staged = bayer_lds_plan(p.inv, H, W, Hs, Ws, &RW, &RH);
  const int tiles_x = ceil_div(W, kBayerDW), tiles_y = ceil_div(H, kBayerDH);
  const long blocks = long(tiles_x) * tiles_y * N;
  FVP_LIMIT(!staged || blocks < (1l << 31));
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  if (staged) {
    const size_t lds = size_t(RH) * RW * 4 + size_t(RH + 4) * (RW + 8);
    hipLaunchKernelGGL(k_ingest_bayer_lds, dim3(unsigned(blocks)), dim3(256), lds, as_stream(s), raw, Hs, Ws, q, tone, p, H,
                       W, tiles_x, tiles_y, RW, RH, nhwc8, nchw);
  } else {
    hipLaunchKernelGGL(k_ingest_bayer_gather, dim3(unsigned((pairs + 255) / 256)), dim3(256), 0, as_stream(s), raw, N, Hs,
                       Ws, q, tone, p, H, W, nhwc8, nchw);
  }
  return launch_status();
}

// argument checks both draw exports share; limbs go into prm
static int draw_args(int B, int V, int Hs, int Ws, const float* views, int N, int J, const int32_t* limbs, int L,
                     const uint8_t* palette, int P, int joint_radius_q4, int limb_half_q4, int alpha, float conf_min,
                     DrawPrm& prm) {
  FVP_REQUIRE(views && palette && (limbs || L <= 0));
  FVP_REQUIRE(B >= 0 && V >= 0 && N >= 1 && J >= 1 && Hs >= 1 && Ws >= 1 && P >= 1 && L >= 0);
  FVP_REQUIRE(alpha >= 1 && alpha <= 256 && joint_radius_q4 >= 0 && joint_radius_q4 <= kDrawMaxR && limb_half_q4 >= 0 &&
              limb_half_q4 <= kDrawMaxR && !std::isnan(conf_min));
  FVP_LIMIT(N <= kDrawMaxN && J <= FVP_MAX_JOINTS && V <= FVP_MAX_VIEWS && L <= kDrawMaxL && P <= kDrawMaxP);
  FVP_LIMIT(Hs <= 16384 && Ws <= 16384 && long(B) * V <= 65535);
  for (int l = 0; l < L; ++l)
    for (int e = 0; e < 2; ++e) {
      FVP_REQUIRE(limbs[2 * l + e] >= 0 && limbs[2 * l + e] < J);
      prm.limb[l][e] = uint8_t(limbs[2 * l + e]);
    }
  return 0;
}

extern "C" int fvp_draw_poses(uint8_t* frames, int B, int V, int Hs, int Ws, const float* views, const int32_t* ids,
                              const float* joint_conf, int N, int J, const int32_t* limbs, int L, const uint8_t* palette,
                              int P, int joint_radius_q4, int limb_half_q4, int alpha, float conf_min, fvp_stream_t s) {
  FVP_REQUIRE(frames);
  DrawPrm prm = {};
  if (const int rc = draw_args(B, V, Hs, Ws, views, N, J, limbs, L, palette, P, joint_radius_q4, limb_half_q4, alpha,
                               conf_min, prm))
    return rc;
  for (int i = 0; i < 3 * P; ++i) prm.pal[i / 3][i % 3] = palette[i];
  if (long(B) * V == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_draw_poses, dim3(ceil_div(Ws, kDrawTW), ceil_div(Hs, kDrawTH), unsigned(B * V)), dim3(kDrawThreads),
                     0, as_stream(s), frames, V, Hs, Ws, views, ids, joint_conf, N, J, L, P, prm, joint_radius_q4,
                     limb_half_q4, alpha, conf_min);
  return launch_status();
}

// what the calls that write an NV12 surface in place (fvp_draw_poses_nv12, fvp_anonymise_rois_nv12) require of it; F frames
static int nv12_write_args(const uint8_t* uv, long F, int Hs, int Ws, long y_pitch, long uv_pitch, long y_frame_stride,
                           long uv_frame_stride, int standard) {
  FVP_REQUIRE(Hs % 2 == 0 && Ws % 2 == 0 && y_pitch >= Ws && uv_pitch >= Ws);
  // a (U, V) pair is one 2-byte load and one 2-byte store
  FVP_REQUIRE(uv_pitch % 2 == 0 && uv_frame_stride % 2 == 0 && reinterpret_cast<uintptr_t>(uv) % 2 == 0);
  FVP_REQUIRE(standard >= 0 && standard < 4);
  FVP_REQUIRE(F <= 1 || (y_frame_stride >= (Hs - 1) * y_pitch + Ws && uv_frame_stride >= (Hs / 2 - 1) * uv_pitch + Ws));
  return 0;
}

// R, G, B -> (Yc, Uc, Vc) of a standard, include/fvp.h; >> is arithmetic
static void rgb_to_yuv(int standard, const uint8_t rgb[3], uint8_t yuv[3]) {
  static const int coeffs[4][12] = {FVP_RGB2YUV_BT601_LIMITED_COEFFS, FVP_RGB2YUV_BT709_LIMITED_COEFFS,
                                    FVP_RGB2YUV_BT601_FULL_COEFFS, FVP_RGB2YUV_BT709_FULL_COEFFS};
  const int* k = coeffs[standard];
  const int r = rgb[0], g = rgb[1], bl = rgb[2];
  for (int c = 0; c < 3; ++c) {
    const int v = k[4 * c] + ((k[4 * c + 1] * r + k[4 * c + 2] * g + k[4 * c + 3] * bl + 32768) >> 16);
    yuv[c] = uint8_t(v < 0 ? 0 : v > 255 ? 255 : v);
  }
}

extern "C" int fvp_draw_poses_nv12(uint8_t* y, uint8_t* uv, int B, int V, int Hs, int Ws, long y_pitch, long uv_pitch,
                                   long y_frame_stride, long uv_frame_stride, int standard, const float* views,
                                   const int32_t* ids, const float* joint_conf, int N, int J, const int32_t* limbs, int L,
                                   const uint8_t* palette, int P, int joint_radius_q4, int limb_half_q4, int alpha,
                                   float conf_min, fvp_stream_t s) {
  FVP_REQUIRE(y && uv);
  DrawPrm prm = {};
  if (const int rc = draw_args(B, V, Hs, Ws, views, N, J, limbs, L, palette, P, joint_radius_q4, limb_half_q4, alpha,
                               conf_min, prm))
    return rc;
  if (const int rc = nv12_write_args(uv, long(B) * V, Hs, Ws, y_pitch, uv_pitch, y_frame_stride, uv_frame_stride, standard))
    return rc;
  for (int i = 0; i < P; ++i) rgb_to_yuv(standard, palette + 3 * i, prm.pal[i]);
  if (long(B) * V == 0) return 0;
  const DrawNv12Prm q = {y_pitch, uv_pitch, y_frame_stride, uv_frame_stride};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_draw_poses_nv12, dim3(ceil_div(Ws, kDrawTW), ceil_div(Hs, kDrawTH), unsigned(B * V)),
                     dim3(kDrawThreads), 0, as_stream(s), y, uv, q, V, Hs, Ws, views, ids, joint_conf, N, J, L, P, prm,
                     joint_radius_q4, limb_half_q4, alpha, conf_min);
  return launch_status();
}

// argument checks both anonymiser exports share; the cell size goes out as its log2
static int anon_args(int F, int Hs, int Ws, const float* rois, int R, int rois_per_frame, int cell, int shape, int mode,
                     const uint8_t* colour, int& sh) {
  FVP_REQUIRE(rois && F >= 0 && R >= 0 && Hs >= 1 && Ws >= 1);
  FVP_REQUIRE(rois_per_frame >= 1 && long(R) == long(F) * rois_per_frame);
  FVP_REQUIRE(cell == 2 || cell == 4 || cell == 8 || cell == 16 || cell == 32);
  FVP_REQUIRE(shape == FVP_ANON_RECT || shape == FVP_ANON_ELLIPSE);
  FVP_REQUIRE(mode == FVP_ANON_MOSAIC || (mode == FVP_ANON_FILL && colour));
  FVP_LIMIT(rois_per_frame <= kAnonMaxRois && Hs <= 16384 && Ws <= 16384 && F <= 65535);
  for (sh = 1; (1 << sh) < cell; ++sh) {
  }
  return 0;
}

extern "C" int fvp_anonymise_rois(uint8_t* frames, int F, int Hs, int Ws, const float* rois, int R, int rois_per_frame,
                                  int cell, int shape, int mode, const uint8_t* colour, fvp_stream_t s) {
  FVP_REQUIRE(frames);
  int sh = 0;
  if (const int rc = anon_args(F, Hs, Ws, rois, R, rois_per_frame, cell, shape, mode, colour, sh)) return rc;
  if (R == 0) return 0;
  const unsigned col = mode == FVP_ANON_FILL ? unsigned(colour[0]) | (unsigned(colour[1]) << 8) | (unsigned(colour[2]) << 16) : 0u;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_anonymise_rois, dim3(ceil_div(Ws, kAnonTW), ceil_div(Hs, kAnonTH), unsigned(F)), dim3(kAnonThreads), 0,
                     as_stream(s), frames, Hs, Ws, rois, rois_per_frame, sh, shape, mode, col);
  return launch_status();
}

extern "C" int fvp_anonymise_rois_nv12(uint8_t* y, uint8_t* uv, int F, int Hs, int Ws, long y_pitch, long uv_pitch,
                                       long y_frame_stride, long uv_frame_stride, int standard, const float* rois, int R,
                                       int rois_per_frame, int cell, int shape, int mode, const uint8_t* colour,
                                       fvp_stream_t s) {
  FVP_REQUIRE(y && uv);
  int sh = 0;
  if (const int rc = anon_args(F, Hs, Ws, rois, R, rois_per_frame, cell, shape, mode, colour, sh)) return rc;
  if (const int rc = nv12_write_args(uv, F, Hs, Ws, y_pitch, uv_pitch, y_frame_stride, uv_frame_stride, standard)) return rc;
  if (R == 0) return 0;
  unsigned col = 0u;
  if (mode == FVP_ANON_FILL) {                           // converted once, on the host, as fvp_draw_poses_nv12 converts its palette
    uint8_t yuv[3];
    rgb_to_yuv(standard, colour, yuv);
    col = unsigned(yuv[0]) | (unsigned(yuv[1]) << 8) | (unsigned(yuv[2]) << 16);
  }
  const DrawNv12Prm q = {y_pitch, uv_pitch, y_frame_stride, uv_frame_stride};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_anonymise_rois_nv12, dim3(ceil_div(Ws, kAnonTW), ceil_div(Hs, kAnonTH), unsigned(F)),
                     dim3(kAnonThreads), 0, as_stream(s), y, uv, q, Hs, Ws, rois, rois_per_frame, sh, shape, mode, col);
  return launch_status();
}

extern "C" int fvp_person_rois(const float* views, const int32_t* ids, const float* joint_conf, int B, int V, int N, int J,
                               uint32_t joint_mask, int min_joints, float scale, float pad_px, float aspect, float conf_min,
                               float* rois, int32_t* roi_count, float* roi_score, fvp_stream_t s) {
  FVP_REQUIRE(views && (rois || roi_count || roi_score));
  FVP_REQUIRE(B >= 0 && V >= 0 && N >= 1 && J >= 1 && min_joints >= 1);
  // a NaN fails each of these compares
  FVP_REQUIRE(scale > 0.0f && std::isfinite(scale) && pad_px >= 0.0f && std::isfinite(pad_px) && aspect > 0.0f &&
              std::isfinite(aspect) && !std::isnan(conf_min));
  FVP_LIMIT(N <= kDrawMaxN && J <= FVP_MAX_JOINTS && V <= FVP_MAX_VIEWS);
  const long total = long(B) * V * N;
  if (long(B) * V == 0) return 0;
  FVP_LIMIT(total < (1l << 31));
  const RoiPrm p = {joint_mask, min_joints, scale, pad_px, aspect, conf_min};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_person_rois, dim3(unsigned((total + 63) / 64)), dim3(64), 0, as_stream(s), views, ids, joint_conf,
                     int(total), V, N, J, p, rois, roi_count, roi_score);
  return launch_status();
}

// argument checks both crop exports share (those of the ingest calls, and the ROI list's)
static int crop_args(int F, int Hs, int Ws, const float* rois, int R, int rois_per_frame, const float mean[3],
                     const float stdv[3], int h, int w, const void* nhwc8, const void* nchw, CropNorm& nm) {
  FVP_REQUIRE(rois && mean && stdv && (nhwc8 || nchw));
  FVP_REQUIRE(F >= 0 && R >= 0 && Hs > 0 && Ws > 0 && h > 0 && w > 0 && w % 2 == 0);
  FVP_REQUIRE(rois_per_frame >= 1 && long(R) == long(F) * rois_per_frame);
  for (int c = 0; c < 3; ++c) {
    FVP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdv[c]) && stdv[c] != 0.0f);
    nm.mean[c] = mean[c];
    nm.stdv[c] = stdv[c];
  }
  return 0;
}

extern "C" int fvp_crop_rois(const uint8_t* frames, int F, int Hs, int Ws, const float* rois, int R, int rois_per_frame,
                             const float mean[3], const float stdv[3], int h, int w, int flags, uint16_t* nhwc8,
                             float* nchw, fvp_stream_t s) {
  FVP_REQUIRE(frames);
  CropNorm nm;
  if (const int rc = crop_args(F, Hs, Ws, rois, R, rois_per_frame, mean, stdv, h, w, nhwc8, nchw, nm)) return rc;
  FVP_REQUIRE((flags & ~FVP_INGEST_SWAP_RB) == 0);
  if (R == 0) return 0;
  FVP_LIMIT(Hs < (1 << 24) && Ws < (1 << 24) && h < (1 << 24) && w < (1 << 24));   // pixel indices exact in fp32
  const long blocks = (long(h) * (w / 2) + 255) / 256;
  FVP_LIMIT(blocks <= 65535);                            // grid: (ROI, blocks of 256 pixel pairs)
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_crop_rois, dim3(unsigned(R), unsigned(blocks)), dim3(256), 0, as_stream(s), frames, Hs, Ws, rois,
                     rois_per_frame, nm, h, w, (flags & FVP_INGEST_SWAP_RB) ? 1 : 0, nhwc8, nchw);
  return launch_status();
}

extern "C" int fvp_crop_rois_nv12(const uint8_t* y, const uint8_t* uv, int F, int Hs, int Ws, long y_pitch, long uv_pitch,
                                  long y_frame_stride, long uv_frame_stride, int standard, const float* rois, int R,
                                  int rois_per_frame, const float mean[3], const float stdv[3], int h, int w,
                                  uint16_t* nhwc8, float* nchw, fvp_stream_t s) {
  static const int coeffs[4][6] = {FVP_YUV_BT601_LIMITED_COEFFS, FVP_YUV_BT709_LIMITED_COEFFS, FVP_YUV_BT601_FULL_COEFFS,
                                   FVP_YUV_BT709_FULL_COEFFS};
  FVP_REQUIRE(y && uv);
  CropNorm nm;
  if (const int rc = crop_args(F, Hs, Ws, rois, R, rois_per_frame, mean, stdv, h, w, nhwc8, nchw, nm)) return rc;
  FVP_REQUIRE(Hs % 2 == 0 && Ws % 2 == 0 && y_pitch >= Ws && uv_pitch >= Ws);
  // a (U, V) pair is one 2-byte load
  FVP_REQUIRE(uv_pitch % 2 == 0 && uv_frame_stride % 2 == 0 && reinterpret_cast<uintptr_t>(uv) % 2 == 0);
  FVP_REQUIRE(standard >= 0 && standard < 4);
  if (R == 0) return 0;
  FVP_LIMIT(Hs < (1 << 24) && Ws < (1 << 24) && h < (1 << 24) && w < (1 << 24));   // pixel indices exact in fp32
  const long blocks = (long(h) * (w / 2) + 255) / 256;
  FVP_LIMIT(blocks <= 65535);                            // grid: (ROI, blocks of 256 pixel pairs)
  const int* k = coeffs[standard];
  const Nv12Prm q = {y_pitch, uv_pitch, y_frame_stride, uv_frame_stride, k[0], k[1], k[2], k[3], k[4], k[5]};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_crop_rois_nv12, dim3(unsigned(R), unsigned(blocks)), dim3(256), 0, as_stream(s), y, uv, Hs, Ws, q,
                     rois, rois_per_frame, nm, h, w, nhwc8, nchw);
  return launch_status();
}

extern "C" int fvp_person_signature(const uint8_t* frames, int B, int V, int Hs, int Ws, const float* views,
                                    const int32_t* ids, const float* joint_conf, const int32_t* occluder, int N, int J,
                                    const int32_t* limbs, const int32_t* limb_part, int L, int P, int K, float conf_min,
                                    int32_t* sig, int32_t* sig_count, fvp_stream_t s) {
  FVP_REQUIRE(frames && views && limbs && limb_part && (sig || sig_count));
  FVP_REQUIRE(B >= 0 && V >= 0 && N >= 1 && J >= 1 && Hs >= 1 && Ws >= 1 && L >= 1 && P >= 1);
  FVP_REQUIRE(K >= 1 && K <= kSigMaxK && !std::isnan(conf_min));
  FVP_LIMIT(N <= kDrawMaxN && J <= FVP_MAX_JOINTS && V <= FVP_MAX_VIEWS && L <= kSigMaxL && P <= FVP_SIG_MAX_PARTS);
  FVP_LIMIT(Hs <= 16384 && Ws <= 16384);
  SigPrm prm = {};
  for (int l = 0; l < L; ++l) {
    for (int e = 0; e < 2; ++e) {
      FVP_REQUIRE(limbs[2 * l + e] >= 0 && limbs[2 * l + e] < J);
      prm.limb[l][e] = uint8_t(limbs[2 * l + e]);
    }
    FVP_REQUIRE(limb_part[l] >= 0 && limb_part[l] < P);
    prm.part[l] = uint8_t(limb_part[l]);
  }
  if (long(B) * V == 0) return 0;
  FVP_LIMIT(long(B) * N < (1l << 31));                   // one workgroup per (b, n)
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_person_signature, dim3(unsigned(B * N)), dim3(kSigThreads), 0, as_stream(s), frames, V, Hs, Ws, views,
                     ids, joint_conf, occluder, N, J, L, P, K, prm, conf_min, sig, sig_count);
  return launch_status();
}
