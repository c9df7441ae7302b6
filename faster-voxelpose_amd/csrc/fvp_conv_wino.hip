// 3x3 stride-1 'same' conv as Winograd F(2x2,3x3) on the fp32 matrix cores (P2PNet's res-blocks,
// lib/models/cnns_2d.py:12-71, are >90 % of the path's FLOPs).  Its own translation unit since round 5
// (compiled with -fno-slp-vectorize: no packed-f32 VALU beside the MFMAs, MI355X_MICROARCH.md "price of one filler").
//
//   Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A      2x2 outputs from a 4x4 input patch,
//
// i.e. 16 independent GEMMs  M_p[cout][tile] = sum_ci U_p[cout][ci] * V_p[ci][tile]  (p = 4*xi+nu):
// 16 multiplies per 4 outputs instead of 36.  Mapping on v_mfma_f32_16x16x4_f32 (4 channels per
// instruction, 4 accumulator registers per 16x16 tile):
//   A operand = U_p   lane l: cout l&15, channel ci + (l>>4)     (pre-transformed by k_pack_wino)
//   B operand = V_p   lane l: tile l&15, channel ci + (l>>4)     (transformed in registers from the
//                                                                 lane's own 4x4 patch in LDS; on
//                                                                 16- and 32-wide maps from its two
//                                                                 own patch columns and the row
//                                                                 neighbours' first pass: k_conv_wsc)
//   D         = M_p   lane l: tile l&15, couts 4*(l>>4) + r
// A wave owns 32 couts x 16 tiles: 2 x 16 accumulator tiles = 128 registers, so two waves fit a
// SIMD and one wave's patch transform / LDS reads overlap the other's MFMAs.  For a fixed
// (cout, tile) all 16 M_p sit in the same lane and register slot: the output transform and the
// bias/BN/residual/ReLU epilogue are pure per-lane arithmetic, stored as float2 rows.
//
// Workgroup = 8 (or 4) waves = WC cout blocks (32) x WT tile blocks (16).  LDS per chunk of CC channels
// (three slots filled by the LDS-DMA two chunks ahead):
//   Xs[CC][TN][TH+2][4 + W]   zero-margin dense rows (halo reads need no masking)
//   Ws[CC][32*WC][16]         quad q of row `co` stored at quad q ^ ((co>>2)&3): the four
//                             ds_read_b128 of a lane (xi = 0..3) are bank-conflict free unpadded
// (That is the A operand.  The B operand's patch reads are NOT conflict-free in the own-patch form, k_conv_wino: a patch
// starts at image x - 1 = an odd column of the row slot, the 16 tile lanes step by two floats and the four channel groups by
// a multiple of four, so an instruction's 64 lanes share the 32 odd banks - SQ_LDS_BANK_CONFLICT reads 2.9 cycles per LDS
// instruction in the 64-128-channel variants; DESIGN.md section 8 says why the layout stays.  The shared-column form,
// k_conv_wsc - the 32- and 16-wide maps, where the 16 lanes of a DPP row are whole tile rows - never reads the two outer
// patch columns: a lane reads the 8-byte-aligned pair at x, x + 1 (one ds_read_b64 per patch row, all 32 banks) and takes the
// first pass of the outer columns from the tiles to its left and right, which computed the same values from the same
// operands, as the DPP source operand of the second pass's subtractions: 24 adds and 4 patch reads per step of 4 channels
// instead of 32 and 8, the same bits.)
//
// Round 5 rewrite of the control structure (same arithmetic, same bits).  The round-4 kernel spilled 20-64 SGPRs in
// every variant (243 v_readlane in the 64-cout form), carried ~470 scalar compares / branches and 159 s_waitcnt per chunk
// loop (run-time DMA item counts, 64-way vmcnt ladders) and packed-f32 adds in the K loop.  Now:
//   * the number of DMA items per wave and chunk (NI input + NW weight instructions) is a template parameter: the chunk
//     body is straight-line code and every counted wait is an immediate;
//   * the per-unit part of a DMA item is 'inside the image or not' only: the lane's byte offset relative to the unit's
//     descriptor base never changes, the validity is bit 31 of that offset (fails the buffer range check -> the
//     hardware writes zeros), recomputed per unit from the lane number (a dozen vector instructions per item, no
//     exec-mask branches, nothing kept in registers for it);
//   * arguments that only the epilogue or the cursor needs are re-read from the kernarg segment where they are used
//     (fresh_args) instead of living in SGPRs across the K loop;
//   * the validity flags of the plane groups (persons) are staged in LDS: the cursor's look-ahead no longer issues a
//     global load (vmcnt) in the middle of the DMA ring;
//   * both chunks staged by the prologue are waited for before the first barrier, so the first chunk barrier of EVERY
//     unit needs no vmcnt wait (the epilogue's single vmcnt(0) covers it, see there);
//   * the epilogue's residual loads / stores are raw-buffer accesses (one per-lane offset + a running scalar row offset);
//   * CW = 1 forms (one 16-cout block per wave): quarter-size units for launches that cannot fill the chip (B = 1), and -
//     diagnostics build only, measured 10-20 % slower - the 16-wave / four-waves-per-SIMD form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "fvp_conv_args.h"

// Ablation switches of the kernel (FVP_CONV_ABLATE bits: 1 no DMA, 4 no MFMA, 8 no epilogue, 16 no residual loads, 32 no
// stores, 128 no chunk barrier, 256 no A reads, 512 no input transform, 1024 epilogue traffic inside 1 MB) exist only in a
// variant built with -DFVP_WINO_ABLATE=1 (tools/build_variant.sh): as run-time flags they cost the diagnostics build 43-87
// spilled VGPRs per instance (round 5: its 32-channel layers ran at half speed, which distorted every A/B made through it).
#ifndef FVP_WINO_ABLATE
#define FVP_WINO_ABLATE 0
#endif

namespace fvp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// s_waitcnt vmcnt(N) with an immediate (lgkmcnt / expcnt untouched)
template <int N>
__device__ __forceinline__ void wait_vmcnt_imm() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt(0x0f70 | (N & 15) | ((N >> 4) << 14));
}

constexpr unsigned kWinoOOB = 0x80000000u;   // offset bit that fails the buffer range check (num_records 0x7ffffff0)

// RESW: the whole Winograd-domain weight tensor of the workgroup's cout block ([cinp][CBW][16], <= 64 KB)
// stays resident in LDS behind the three input slots (loaded once per persistent workgroup) instead of
// streaming through the slots chunk by chunk: for the 32-channel layers the weight chunks were more than
// half of the LDS-DMA traffic of a unit.
// CW = cout blocks (of 16) per wave: 2 = the 128-accumulator wave tile above (two waves per SIMD); 1 = 16 couts x 16 tiles,
// 64 accumulators, <= 128 registers: a 16-wave workgroup, FOUR waves per SIMD (round 5: more waves to cover each other's
// LDS / DMA / barrier waits, at twice the patch transforms per MFMA).  WC = wave groups along the couts.
// SH = form of the input transform, the planner's choice from the layer shape (ConvArgs::shcols; two-block waves only).
// 0: every lane transforms its own 4x4 patch.  1 / 2: the shared-column form - the 16 lanes of a DPP row hold whole tile
// rows, and a tile takes the outer columns of its transform's first pass from its left / right neighbour instead of reading
// and transforming them itself (`columns` in the kernel body):
//   1: rows of 16 tiles (W = 32) - lane = tile column, the neighbour is the adjacent lane;
//   2: rows of 8 tiles (W = 16) - a DPP row holds two tile rows, interleaved: lane 2 * tx + row, the neighbour is two lanes
//      away.  Either way both image borders of every tile row fall on the ends of a DPP row.
// The (workgroup, chunk, DMA rounds) combinations a shared-column unit can have: one plane, 8 (W = 32) or 16 (W = 16) input
// rows + 2 per 64 tiles of 2 x 2 - 10 x 9 or 18 x 5 quads (+ 1) per channel for the 8-wave cout-pair and the 4-wave
// workgroups, twice the rows for the 8-wave 32-cout one.  Only these are instantiated; the planner asks before it picks the form.
constexpr bool wino_shared_instance(int WC, int WT, int CC, int NI) {
  return WC == 2 ? (WT == 4 && NI == (CC == 8 ? 2 : 1)) : WT == 4 ? (CC == 4 && NI == 2) : (WT == 8 && NI == (CC == 8 ? 3 : 2));
}

// The kernel body is fvp_conv_wino_body.h, included into both kernels below.
template <int WC, int WT, int CC, int NI, bool HAS_RES, bool RESW, int SH>
__global__ void k_conv_wsc(ConvArgs a);

// The own-patch form: every shape the planner takes.  (The CPU emulation of the kernels has this one entry per instance -
// its launch log names k_conv_wino<...> - and takes the shared-column forms from the launch argument here; the GPU build
// launches them as kernels of their own, k_conv_wsc: no instance carries a form it does not run.)
template <int WC, int WT, int CC, int NI, bool HAS_RES, bool RESW, int CW = 2>
__global__ void __launch_bounds__(WC * WT * 64, (WC * WT == 16 ? 4 : 2)) k_conv_wino(ConvArgs a) {
#if defined(HIPEMU)
  if constexpr (CW == 2 && wino_shared_instance(WC, WT, CC, NI)) {
    if (a.shcols == 1) return k_conv_wsc<WC, WT, CC, NI, HAS_RES, RESW, 1>(a);
    if (a.shcols == 2) return k_conv_wsc<WC, WT, CC, NI, HAS_RES, RESW, 2>(a);
  }
#endif
  constexpr int SH = 0;
  constexpr int SKIP = 0;
#include "fvp_conv_wino_body.h"
}

// The shared-column forms (SH = 1: W = 32, SH = 2: W = 16), two-block waves.
template <int WC, int WT, int CC, int NI, bool HAS_RES, bool RESW, int SH>
__global__ void __launch_bounds__(WC * WT * 64, 2) k_conv_wsc(ConvArgs a) {
  constexpr int CW = 2;
  constexpr int SKIP = 0;
#include "fvp_conv_wino_body.h"
}

// The same two kernels with the res-block's 1x1 skip conv fused into the epilogue (SKIP in the body): the residual
// s = BN(conv1x1(x)) is computed from x by 16x16x4 MFMAs instead of being read back (ConvArgs::skip_*).  Kernels of their
// own names: the instances without a fused skip keep their code.
// SKIP = the skip's MFMA steps: 4 (16 channels) or 8 (32).
template <int WC, int WT, int CC, int NI, bool RESW, int SH, int SKIP>
__global__ void k_conv_wsc_skip(ConvArgs a);

template <int WC, int WT, int CC, int NI, bool RESW, int CW, int SKIP>
__global__ void __launch_bounds__(WC * WT * 64, (WC * WT == 16 ? 4 : 2)) k_conv_wino_skip(ConvArgs a) {
#if defined(HIPEMU)
  if constexpr (CW == 2 && wino_shared_instance(WC, WT, CC, NI)) {
    if (a.shcols == 1) return k_conv_wsc_skip<WC, WT, CC, NI, RESW, 1, SKIP>(a);
    if (a.shcols == 2) return k_conv_wsc_skip<WC, WT, CC, NI, RESW, 2, SKIP>(a);
  }
#endif
  constexpr int SH = 0;
  constexpr bool HAS_RES = true;
#include "fvp_conv_wino_body.h"
}

template <int WC, int WT, int CC, int NI, bool RESW, int SH, int SKIP>
__global__ void __launch_bounds__(WC * WT * 64, 2) k_conv_wsc_skip(ConvArgs a) {
  constexpr int CW = 2;
  constexpr bool HAS_RES = true;
#include "fvp_conv_wino_body.h"
}

// state_dict weight [cout][cin][3][3] -> Winograd-domain U = G g G^T, layout [cinp][coutp][16]
// with quad xi of row `co` stored at quad xi ^ ((co>>2)&3).
__global__ void __launch_bounds__(256)
k_pack_wino(const float* __restrict__ w, int cin, int cout, int cinp, int coutp, float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cinp * coutp) return;
  const int co = i % coutp, ci = i / coutp;
  float g[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
      g[ky][kx] = (co < cout && ci < cin) ? w[(size_t(co) * cin + ci) * 9 + ky * 3 + kx] : 0.0f;
  float gg[4][3];                                   // G g
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const float e = g[0][kx] + g[2][kx];
    gg[0][kx] = g[0][kx];
    gg[1][kx] = 0.5f * (e + g[1][kx]);
    gg[2][kx] = 0.5f * (e - g[1][kx]);
    gg[3][kx] = g[2][kx];
  }
  float* out = dst + size_t(i) * 16;
  const int swz = (co >> 2) & 3;
#pragma unroll
  for (int xi = 0; xi < 4; ++xi) {                   // (G g) G^T
    const float e = gg[xi][0] + gg[xi][2];
    float* o = out + 4 * (xi ^ swz);
    o[0] = gg[xi][0];
    o[1] = 0.5f * (e + gg[xi][1]);
    o[2] = 0.5f * (e - gg[xi][1]);
    o[3] = gg[xi][2];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
static const size_t kWinoLdsBudget = env_size("FVP_WINO_LDS_KB", 152) * 1024;
static const int kWinoGeneric = int(env_size("FVP_WINO_GENERIC", 0));
constexpr int kWinoMaskedMinW = 40;     // narrowest non-power-of-two row that takes masked Winograd tiles (netspec.WINO_MASKED_MIN_W)
static const int kWinoWC1 = int(env_size("FVP_WINO_WC1", 0));        // diagnostics: 32-cout blocks for every layer
// 4-wave workgroups (32 couts x 64 tiles, <= 78 KB of LDS, two per CU) instead of one 8-wave workgroup per CU:
// half-size work units.  Slower per FLOP when the launch has plenty of units (more LDS-DMA traffic per MFMA), but
// a small batch (B = 1: 30 planes) has only 60-120 full-size units for 256 CUs.  FVP_WINO_HALF: 0 = automatic
// (half-size units when the full-size ones cannot fill the CUs), 1 = always, 2 = never.  Both tilings perform the
// same arithmetic in the same order, so the result does not depend on the choice (i.e. on the batch).
static const int kWinoHalf = int(env_size("FVP_WINO_HALF", 0));
static const int kWinoNoResW = int(env_size("FVP_WINO_NO_RESW", 0)); // diagnostics: stream the weights of the 32-channel layers too
static const int kWinoAblate = int(env_size("FVP_CONV_ABLATE", 0));
#ifndef FVP_WINO_W16_DEFAULT
#define FVP_WINO_W16_DEFAULT 0
#endif

int persistent_workgroups() {
  static int n = 0;
  if (!n) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    n = int(env_size("FVP_WINO_WGS", size_t(cus)));
  }
  return n;
}

// Shapes the Winograd kernel covers: 3x3, even H, W a power of two in [8, 64*4] with W/2 dividing
// a wave's 32 tiles or vice versa.  Decided from the layer SHAPE only (never from the number of
// planes), so a frame's result does not depend on the batch it is computed in.
static bool wino_tiling(int h, int w, int cinp, int coutp, int* WC, int* WT, int* TN, int* TR, bool half = false) {
  if (h < 2 || (h & 1) || w < 8 || (w & 3) || (coutp != 32 && coutp % 64 != 0) || cinp % 4 != 0) return false;
  // Maps whose rows do not divide the workgroup tile (CenterNet's 80x80 / 40x40 / 20x20 levels) run with masked tiles.
  // Until round 5 they stayed on the direct kernel (582 vs 564 us for CenterNet at B = 8 in round 3: launch-latency bound
  // either way).  Since round 5's rewrite of this kernel the masked form wins on the 80- and 40-wide levels at every batch
  // (round 6, same box: 3x3 layers 23 -> 14.7 / 19.5 -> 13.8 us at B = 8, 11.5 -> 8 / 18.5 -> 13.2 us at B = 1; CenterNet
  // 496 -> ~420 us per pass at B = 8, 379 -> ~330 us at B = 1), while the 20-wide level is faster on the split-K direct form
  // at B = 1 (17 vs 22 us; one or two workgroups of tiles).  So: rows of >= 40 columns take masked tiles, narrower ones the
  // direct kernel - a SHAPE rule, never the batch.  The detection map moves by fp32 rounding only: the GPU suite (top-k
  // indices, proposal centres and valid flags exact on every golden and sweep) is green with it and the joints do not change
  // by a bit (the joint stage reads nothing of CenterNet's float values).  FVP_WINO_GENERIC=1 (diagnostics build) takes
  // every width.
  if ((w & (w - 1)) && w < kWinoMaskedMinW && !kWinoGeneric) return false;
  *WC = (coutp == 32 || kWinoWC1 || half) ? 1 : 2;
  *WT = (half ? 4 : 8) / *WC;
  // a unit = TN planes x TR tile rows x (w/2) tiles <= the workgroup's 16*WT tiles; tiles beyond that product
  // (maps whose row length does not divide the workgroup tile: 80x80, 40x40, 20x20) are masked lanes
  const int tpr = w / 2, TT = 16 * *WT, rows = h / 2;
  if (tpr > TT) return false;
  if (rows * tpr >= TT) {
    *TN = 1;
    *TR = TT / tpr;
  } else {
    *TN = TT / (rows * tpr);
    *TR = rows;
  }
  return true;
}

bool wino_shape_ok(int h, int w, int cinp, int coutp) {
  int WC, WT, TN, TR;
  return wino_tiling(h, w, cinp, coutp, &WC, &WT, &TN, &TR);
}

#if defined(HIPEMU)
template <int SH> void wino_shared_columns_form() {}   // a name for the emulation's launch log
#endif
template <int WC, int WT, int CC, int NI, bool RES, bool RESW, int SH>
static int launch_wsc(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  static LdsOptIn optin;
  auto k = &k_conv_wsc<WC, WT, CC, NI, RES, RESW, SH>;
  if (int e = lds_opt_in(optin, reinterpret_cast<const void*>(k), 160 * 1024)) return e;
  hipLaunchKernelGGL(k, grid, dim3(WC * WT * 64), lds, s, a);
  return launch_status();
}
// the instance with the fused skip (ConvArgs::skip_src set): the own-patch kernel or, as in launch_wino3, its shared-column form
template <int WC, int WT, int CC, int NI, bool RESW, int CW, int SKIP>
static int launch_wino_skip(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
#if !defined(HIPEMU)
  if constexpr (CW == 2 && wino_shared_instance(WC, WT, CC, NI)) {
    if (a.shcols == 1 || a.shcols == 2) {
      static LdsOptIn optin[2];
      auto k = a.shcols == 1 ? &k_conv_wsc_skip<WC, WT, CC, NI, RESW, 1, SKIP> : &k_conv_wsc_skip<WC, WT, CC, NI, RESW, 2, SKIP>;
      if (int e = lds_opt_in(optin[a.shcols - 1], reinterpret_cast<const void*>(k), 160 * 1024)) return e;
      hipLaunchKernelGGL(k, grid, dim3(WC * WT * 64), lds, s, a);
      return launch_status();
    }
  }
  if (a.shcols) return FVP_EINVAL;
#else
  if (a.shcols == 1) hipemu::log_launch(reinterpret_cast<const void*>(&wino_shared_columns_form<1>));
  if (a.shcols == 2) hipemu::log_launch(reinterpret_cast<const void*>(&wino_shared_columns_form<2>));
#endif
  static LdsOptIn optin;
  auto k = &k_conv_wino_skip<WC, WT, CC, NI, RESW, CW, SKIP>;
  if (int e = lds_opt_in(optin, reinterpret_cast<const void*>(k), 160 * 1024)) return e;
  hipLaunchKernelGGL(k, grid, dim3(WC * WT * 64), lds, s, a);
  return launch_status();
}
template <int WC, int WT, int CC, int NI, bool RES, bool RESW, int CW = 2>
static int launch_wino3(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  if (a.skip_src) {                                    // (the planner fuses a skip into two-wave-per-SIMD residual forms only)
    if constexpr (RES && WC * WT != 16) {
      if (a.skip_cin == 16) return launch_wino_skip<WC, WT, CC, NI, RESW, CW, 4>(a, grid, lds, s);
      if (a.skip_cin == 32) return launch_wino_skip<WC, WT, CC, NI, RESW, CW, 8>(a, grid, lds, s);
    }
    return FVP_EINVAL;
  }
#if !defined(HIPEMU)
  if constexpr (CW == 2 && wino_shared_instance(WC, WT, CC, NI)) {
    if (a.shcols == 1) return launch_wsc<WC, WT, CC, NI, RES, RESW, 1>(a, grid, lds, s);
    if (a.shcols == 2) return launch_wsc<WC, WT, CC, NI, RES, RESW, 2>(a, grid, lds, s);
  }
  if (a.shcols) return FVP_EINVAL;                   // (the planner picked a form without an instance)
#else
  // (the emulation's launch log names the form too: tests/test_wino_shared_columns.py)
  if (a.shcols == 1) hipemu::log_launch(reinterpret_cast<const void*>(&wino_shared_columns_form<1>));
  if (a.shcols == 2) hipemu::log_launch(reinterpret_cast<const void*>(&wino_shared_columns_form<2>));
#endif
  static LdsOptIn optin;
  auto k = &k_conv_wino<WC, WT, CC, NI, RES, RESW, CW>;
  if (int e = lds_opt_in(optin, reinterpret_cast<const void*>(k), 160 * 1024)) return e;
  hipLaunchKernelGGL(k, grid, dim3(WC * WT * 64), lds, s, a);
  return launch_status();
}
template <int WC, int WT, int CC, bool RESW, int CW = 2>
static int launch_wino2(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  const bool res = a.flags & FVP_EPI_RES;
  switch (a.wino_ni) {
    case 1: return res ? launch_wino3<WC, WT, CC, 1, true, RESW, CW>(a, grid, lds, s) : launch_wino3<WC, WT, CC, 1, false, RESW, CW>(a, grid, lds, s);
    case 2: return res ? launch_wino3<WC, WT, CC, 2, true, RESW, CW>(a, grid, lds, s) : launch_wino3<WC, WT, CC, 2, false, RESW, CW>(a, grid, lds, s);
    case 3: return res ? launch_wino3<WC, WT, CC, 3, true, RESW, CW>(a, grid, lds, s) : launch_wino3<WC, WT, CC, 3, false, RESW, CW>(a, grid, lds, s);
    case 4: return res ? launch_wino3<WC, WT, CC, 4, true, RESW, CW>(a, grid, lds, s) : launch_wino3<WC, WT, CC, 4, false, RESW, CW>(a, grid, lds, s);
  }
  return FVP_ELIMIT;
}
#if FVP_DIAG
// 16-wave form (one 16-cout block per wave, four waves per SIMD): CC = 8, one or two input DMA rounds
template <int WC, int WT, bool RESW>
static int launch_wino16(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
  const bool res = a.flags & FVP_EPI_RES;
  if (a.wino_ni == 1)
    return res ? launch_wino3<WC, WT, 8, 1, true, RESW, 1>(a, grid, lds, s) : launch_wino3<WC, WT, 8, 1, false, RESW, 1>(a, grid, lds, s);
  if (a.wino_ni == 2)
    return res ? launch_wino3<WC, WT, 8, 2, true, RESW, 1>(a, grid, lds, s) : launch_wino3<WC, WT, 8, 2, false, RESW, 1>(a, grid, lds, s);
  return FVP_ELIMIT;
}
#endif
template <int WC, int WT>
static int launch_wino(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s, bool resw) {
  if (WC == 1 && WT == 8 && resw && a.CC == 8) return launch_wino2<1, 8, 8, true>(a, grid, lds, s);
  if (a.CC == 8) return launch_wino2<WC, WT, 8, false>(a, grid, lds, s);
  return launch_wino2<WC, WT, 4, false>(a, grid, lds, s);
}

// `skip`: the res-block's 1x1 skip conv whose output is this conv's residual, to be computed in the epilogue from
// a.skip_src (the caller's look-ahead, fused_skip() in fvp_conv.hip, found it); refused with FVP_ELIMIT where its LDS copy
// does not fit beside the ring the conv has without it - the caller then launches the skip on its own.  `plan_only`: that
// look-ahead's question - everything but the launch.
int wino_plan_and_launch(const FvpConvOp& op, ConvArgs a, const float* params, int planes, hipStream_t s, const FvpConvOp* skip,
                         bool plan_only) {
  int WC, WT, TN, TR;
  if (conv_form(op, planes, a.pool_dst != nullptr, a.w2 != nullptr) != ConvForm::Wino) return FVP_EINVAL;
  if (!wino_tiling(op.h, op.w, op.cinp, op.coutp, &WC, &WT, &TN, &TR, kWinoHalf == 1)) return FVP_EINVAL;
  if (kWinoHalf == 0) {
    // full-size units: (rows bands) x (plane groups) x (cout blocks); switch to half-size ones when they cannot fill the CUs
    const long units = long(ceil_div(op.h / 2, TR)) * ceil_div(planes, TN) * (op.coutp / (32 * WC));
    int wc, wt, tn, tr;
    if (units < persistent_workgroups() && wino_tiling(op.h, op.w, op.cinp, op.coutp, &wc, &wt, &tn, &tr, true)) {
      WC = wc; WT = wt; TN = tn; TR = tr;
    }
  }
  // 16-wave form (one 16-cout block per wave, four waves per SIMD) for full-size units: instantiated in the diagnostics
  // build only (FVP_WINO_W16=1).  Measured in round 5, same box, P2PNet at B = 8, per launch: 64 -> 64 @32x32 98 -> 109 us,
  // 128 -> 128 @16x16 85 -> 99 us, 32 -> 32 @64x64 with residual 119 -> 143 us, whole pass 1 916 -> 2 113 us, pipelined
  // 3 150 -> 2 960 frames/s: twice the patch transforms and A reads per MFMA cost more than four waves per SIMD hide.
#if FVP_DIAG
  static const int kW16 = int(env_size("FVP_WINO_W16", FVP_WINO_W16_DEFAULT));
#else
  constexpr int kW16 = 0;
#endif
  const bool w16 = kW16 && WC * WT == 8 && op.cinp % 8 == 0;
  // Quarter-size units (round 5): when even the half-size units (32 couts x 64 tiles) fill less than a quarter of the
  // chip's 512 slots - B = 1: the 128-channel 16x16 layers have 120 of them - a 4-wave workgroup takes 16 couts x 64 tiles
  // (one 16-cout block per wave: the accumulation chain of a (cout, tile) is the same, so the bits are) and the launch's
  // critical path, one unit, halves: 30 -> 23 us per launch, B = 1 serial 795 -> 822 frames/s (1.26 -> 1.22 ms) at 1 915 -> 1 883
  // with four batches in flight.  Applied to every layer below half the slots (240 units: the 32- / 64-channel layers at
  // B = 1 too) it reaches 825 serial but 1 845 in flight and costs B = 2 3 % (twice the patch transforms per MFMA on a chip that
  // IS full then): threshold 1/4.
  // FVP_WINO_QUARTER (diagnostics build): 0 = never, 1 = below a quarter of the slots (default), 2 = below half.
  static const int kQuarter = int(env_size("FVP_WINO_QUARTER", 1));
  bool quarter = false;
  if (kQuarter && !w16 && WC * WT == 4 && op.cinp % 4 == 0) {
    const long units_half = long(ceil_div(op.h / 2, TR)) * ceil_div(planes, TN) * (op.coutp / 32);
    quarter = units_half * (kQuarter == 2 ? 1 : 2) < persistent_workgroups();
  }
  const int CW = (w16 || quarter) ? 1 : 2;
  if (w16) WC *= 2;                                  // wave groups along the couts: 16 couts each
  // Shared-column input transform (k_conv_wsc): the maps whose tile rows fill the DPP rows of a wave - W = 32
  // (16 tiles: one row per 16 lanes) and W = 16 (8 tiles: two rows, interleaved) - in one-plane units of two-block waves.  A
  // SHAPE rule like the tiling itself: full- and half-size units take it, at every batch (the quarter-size and 16-wave forms,
  // CW = 1, keep the own-patch form).  Wider rows (the neighbouring tile lives in another wave), masked rows and several
  // planes per unit keep the own-patch form.  FVP_WINO_SHARED_COLS (diagnostics build): bit 0 = W = 32, bit 1 = W = 16.
  static const int kSharedCols = int(env_size("FVP_WINO_SHARED_COLS", 3));
  a.ablate = kWinoAblate;
  a.wts = params + op.wino_off;
  a.TN = TN;
  a.TH = 2 * TR;
  a.TW = op.w;
  a.tiles_x = 1;
  a.tiles_y = ceil_div(op.h / 2, TR);
  a.tpp = TR * (op.w / 2);
  a.m_tpp = make_magic(a.tpp);
  a.tpr = op.w / 2;
  a.m_tpr = make_magic(a.tpr);
  a.vec = a.dma = 1;
  a.zeros = params;
  const int CBW = 16 * CW * WC;
  // channels per chunk: 8 when it divides cinp and three slots fit, else 4
  // resident weights: one 32-cout block covers all couts and [cinp][32][16] fits beside the three input slots
  const size_t resw_bytes = size_t(op.cinp) * CBW * 64;
  const size_t budget = WC * WT == 4 ? std::min<size_t>(kWinoLdsBudget, 78 * 1024) : kWinoLdsBudget;   // two workgroups per CU
  const size_t epi_bytes = size_t(3) * op.coutp * 4;     // bias | scale | shift in LDS
  // validity flags of the plane groups (one byte each, only consulted for one-plane units)
  a.nflags = (a.plane_valid && TN == 1) ? ceil_div(planes, a.valid_div) : 0;
  a.m_vd = make_magic(a.valid_div);
  const size_t flag_bytes = size_t(a.nflags + 15) & ~size_t(15);
  bool resw = CBW == 32 && WT == 8 && op.coutp == 32 && op.cinp % 8 == 0 && resw_bytes <= 64 * 1024 && !kWinoNoResW;
  auto slot_bytes = [&](int cc, int* ni, bool rw) {
    const size_t quads = size_t(cc) * TN * (a.TH + 2) * (op.w / 4 + 1) + 1;
    const size_t per_round = size_t(WC) * WT * 64;       // one 16-byte item per thread and round
    *ni = int((quads + per_round - 1) / per_round);
    return size_t(*ni) * per_round * 16 + (rw ? 0 : size_t(cc) * CBW * 64);
  };
  const size_t fixed = 64 + epi_bytes + flag_bytes;
  int CC = op.cinp % 8 == 0 ? 8 : 4, ni = 0;
  size_t slot = slot_bytes(CC, &ni, resw);
  if (resw && (3 * slot + resw_bytes + fixed > budget || ni > 4)) {
    resw = false;
    slot = slot_bytes(CC, &ni, false);
  }
  if (CC == 8 && !resw && (3 * slot + fixed > budget || ni > 4)) {
    CC = 4;
    slot = slot_bytes(CC, &ni, false);
  }
  if (3 * slot + (resw ? resw_bytes : 0) + fixed > budget || ni > 4) return FVP_ELIMIT;
  a.CC = CC;
  a.wino_ni = ni;
  a.shcols = 0;
  if (CW == 2 && !w16 && TN == 1 && wino_shared_instance(WC, WT, CC, ni)) {
    if (op.w == 32 && (kSharedCols & 1)) a.shcols = 1;
    if (op.w == 16 && TR % 2 == 0 && (kSharedCols & 2)) a.shcols = 2;
  }
  if (!buf_dma_range_ok(TN, op.cin, op.h, op.w, double(op.cinp) * op.coutp * 16)) return FVP_ELIMIT;
  // the epilogue's per-lane byte offset spans the unit's TN planes of the output (bit 31 is the 'masked' flag)
  if ((double(TN) + 1.0) * op.cout * op.h * op.w * 4.0 >= 2147483648.0) return FVP_ELIMIT;
  a.m_qpr = make_magic(op.w / 4 + 1);
  a.m_rpc = make_magic(TN * (a.TH + 2));
  a.m_thp = make_magic(a.TH + 2);
  size_t lds = 16 + 3 * slot + (resw ? resw_bytes : 0) + epi_bytes + flag_bytes;
  double skip_flops = 0.0;
  a.skip_src = skip ? a.skip_src : nullptr;
  if (skip) {
    // The fused skip's BN vectors and weights [skip_cin][coutp] behind the flags.  The ring (chunk size, DMA rounds, resident
    // weights) stays what the conv has without the skip - planned against `budget` above - and the copy has to fit in what
    // the CU has left: 160 KB for the one-per-CU workgroups, half of it for the two-per-CU ones.
    if (w16 || !(a.flags & FVP_EPI_RES) || (skip->cin != 16 && skip->cin != 32) || skip->coutp != op.coutp)
      return FVP_ELIMIT;
    a.skip_off = int(lds / sizeof(float));
    a.skip_cin = skip->cin;
    a.skip_wts = params + skip->w_off;
    a.skip_epi = params + skip->e_off;
    const int sg = (skip->cin + 15) / 16;
    lds += (size_t(3) * op.coutp + size_t(op.coutp) * 16 * sg) * sizeof(float);
    if (lds > (WC * WT == 4 ? 80 : 160) * size_t(1024)) return FVP_ELIMIT;
    skip_flops = 2.0 * skip->cin * skip->cout * double(op.h) * op.w * planes;
  }
  if (plan_only) return 0;
  a.ysplit = op.coutp / CBW;
  a.nunits = a.tiles_y * ceil_div(planes, TN) * a.ysplit;
  a.m_ys = make_magic(a.ysplit);
  a.m_ty = make_magic(a.tiles_y);
  // One workgroup per slot.  FVP_WINO_BALANCED=1 (diagnostics build): ceil(units / rounds) workgroups that all do the same
  // number of units (240 instead of 256 for 240 planes), leaving 16 CUs to the other streams for the whole launch.
  static const int kBalanced = int(env_size("FVP_WINO_BALANCED", 0));
  const int slots = persistent_workgroups() * (WC * WT == 4 ? 2 : 1);
  dim3 grid(kBalanced ? ceil_div(a.nunits, ceil_div(a.nunits, slots)) : std::min(a.nunits, slots), 1, 1);
  ProfScope ps(a.nunits < slots ? FVP_K_CONV_WINO_SMALL : FVP_K_CONV_WINO, s, 2.0 * op.cin * op.cout * 9.0 * op.h * op.w * planes + skip_flops, 1,
               prof_level() >= 2);
#if FVP_DIAG
  if (w16) {
    if (CC != 8 || ni > 2) return FVP_ELIMIT;        // (shapes outside the 16-wave instances)
    if (CBW == 32) return resw ? launch_wino16<2, 8, true>(a, grid, lds, s) : launch_wino16<2, 8, false>(a, grid, lds, s);
    return launch_wino16<4, 4, false>(a, grid, lds, s);
  }
#endif
  if (quarter) return a.CC == 8 ? launch_wino2<1, 4, 8, false, 1>(a, grid, lds, s) : launch_wino2<1, 4, 4, false, 1>(a, grid, lds, s);
  if (WC * WT == 4) return launch_wino<1, 4>(a, grid, lds, s, false);
  return WC == 1 ? launch_wino<1, 8>(a, grid, lds, s, resw) : launch_wino<2, 4>(a, grid, lds, s, false);
}

int wino_pack(const float* weight, const FvpConvOp& op, float* params, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_wino, dim3(ceil_div(op.cinp * op.coutp, 256)), dim3(256), 0, s, weight, op.cin, op.cout,
                     op.cinp, op.coutp, params + op.wino_off);
  return launch_status();
}

}  // namespace fvp
