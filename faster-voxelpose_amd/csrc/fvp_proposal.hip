// Proposal path (gfx950): 3x3 NMS + exact top-k, gathers at the selected cells, z arg-max and
// proposal packing.  Integer / index results are bit-exact with the reference
// (lib/core/proposal.py:13-33, lib/models/human_detection_net.py:44-65, :85-102).
// Tie rule (torch.topk leaves ties unspecified): value descending, then lowest flat index.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "fvp_common.h"

namespace fvp {

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// One workgroup (1024 threads) per frame.  The map is copied to LDS once (coalesced), the 3x3 NMS reads its nine
// neighbours from there, then N rounds of block arg-max over the kept values.  REG = true (X * Y <= 16 384, every
// shipped config): every thread owns <= 16 cells in registers, a round is a register scan + shuffle tree + one
// 16-entry LDS stage.  REG = false (larger maps, up to the LDS limit of ~40 000 cells, e.g. 200 x 200): the keep
// decisions are taken for all cells first (one bit per cell in two registers), then the map is overwritten in
// place by keep * x and the rounds scan the thread's cells in LDS.  Same results either way.
constexpr int kNmsThreads = 1024, kNmsCells = 16, kNmsMaxCellsLds = 64;
template <bool REG>
__global__ void __launch_bounds__(kNmsThreads)
k_nms_topk(const float* __restrict__ hm, int X, int Y, int N, float* __restrict__ vals, long long* __restrict__ idx,
           long long* __restrict__ flat) {
  HIP_DYNAMIC_SHARED(float, raw)                // [X*Y] raw map | 16 values | 16 indices
  const int b = blockIdx.x, t = threadIdx.x, n = X * Y;
  const float* m = hm + size_t(b) * n;
  float* wv = raw + n;
  int* wi = reinterpret_cast<int*>(raw + n + 16);
  for (int i = t; i < n; i += kNmsThreads) raw[i] = m[i];
  __syncthreads();
  // keep = (x == max).float(); keep * x   (core/proposal.py:23-25)
  auto kept = [&](int i) {
    const int x = i / Y, y = i - x * Y;
    const float cv = raw[i];
    float mx = cv;
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy) {
        const int xx = x + dx, yy = y + dy;
        if (xx >= 0 && xx < X && yy >= 0 && yy < Y) mx = fmaxf(mx, raw[xx * Y + yy]);
      }
    return cv == mx;
  };
  // kept value of this thread's cells i = t + 1024 c
  float kv[kNmsCells];
  if (REG) {
#pragma unroll
    for (int c = 0; c < kNmsCells; ++c) {
      const int i = t + c * kNmsThreads;
      kv[c] = -INFINITY;
      if (i < n) kv[c] = __fmul_rn(kept(i) ? 1.0f : 0.0f, raw[i]);
    }
  } else {
    unsigned long long bits = 0;                // host: n <= kNmsMaxCellsLds * 1024
    for (int c = 0, i = t; i < n; ++c, i += kNmsThreads) bits |= (unsigned long long)(kept(i) ? 1 : 0) << c;
    __syncthreads();                            // every neighbourhood has been read: overwrite in place
    for (int c = 0, i = t; i < n; ++c, i += kNmsThreads) raw[i] = __fmul_rn(((bits >> c) & 1) ? 1.0f : 0.0f, raw[i]);
    // (each thread re-reads only its own cells below: no barrier needed)
  }
  for (int k = 0; k < N; ++k) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (REG) {
#pragma unroll
      for (int c = 0; c < kNmsCells; ++c) {
        const int i = t + c * kNmsThreads;
        if (i < n && better(kv[c], i, bv, bi)) { bv = kv[c]; bi = i; }
      }
    } else {
      for (int i = t; i < n; i += kNmsThreads)
        if (better(raw[i], i, bv, bi)) { bv = raw[i]; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((t & 63) == 0) { wv[t >> 6] = bv; wi[t >> 6] = bi; }
    __syncthreads();
    // every thread reduces the 16 wave winners (broadcast reads) so the winner is known everywhere without a second barrier
    bv = wv[0];
    bi = wi[0];
    for (int w = 1; w < kNmsThreads / 64; ++w)
      if (better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    if (bi == 0x7fffffff) bi = 0;               // N > number of finite cells: degenerate, pick cell 0 (value -inf)
    if (t == 0) {
      vals[size_t(b) * N + k] = bv;
      flat[size_t(b) * N + k] = bi;
      // the reference unravels with shape[1] = X for both coordinates (core/proposal.py:16-17)
      idx[(size_t(b) * N + k) * 2 + 0] = bi / X;
      idx[(size_t(b) * N + k) * 2 + 1] = bi % X;
    }
    if (REG) {
#pragma unroll
      for (int c = 0; c < kNmsCells; ++c)
        if (t + c * kNmsThreads == bi) kv[c] = -INFINITY;   // the owner retires the winner
    } else if ((bi & (kNmsThreads - 1)) == t) {
      raw[bi] = -INFINITY;                       // the owner's own cell: visible to its next scan without a barrier
    }
    __syncthreads();                              // wv / wi are rewritten next round
  }
}

__global__ void __launch_bounds__(256)
k_gather(const float* __restrict__ bbox_map, const float* __restrict__ cubes, const long long* __restrict__ flat, int B,
         int J, int XY, int Z, int N, float* __restrict__ bbox_flat, float* __restrict__ match_bbox,
         float* __restrict__ feat1d) {
  const long i = long(blockIdx.x) * 256 + threadIdx.x;
  if (bbox_flat && i < long(B) * XY * 2) {      // [B][XY][2] <- [B][2][XY]
    const int c = int(i % 2);
    const long r = i / 2;
    const int cell = int(r % XY), b = int(r / XY);
    bbox_flat[i] = bbox_map[(size_t(b) * 2 + c) * XY + cell];
  }
  if (i < long(B) * N * 2) {
    const int c = int(i % 2);
    const long r = i / 2;
    const int b = int(r / N);
    match_bbox[i] = bbox_map[(size_t(b) * 2 + c) * XY + flat[r]];
  }
  if (cubes && i < long(B) * N * J * Z) {       // feat1d[b*N+k][j][z] = cubes[b][j][flat][z]
    const int z = int(i % Z);
    long r = i / Z;
    const int j = int(r % J);
    r /= J;
    const int b = int(r / N);
    feat1d[i] = cubes[((size_t(b) * J + j) * XY + flat[r]) * Z + z];
  }
}

__global__ void __launch_bounds__(64)
k_proposals(const float* __restrict__ hm1d, const float* __restrict__ conf2d, const long long* __restrict__ idx2d,
            const float* __restrict__ match_bbox, const float* __restrict__ sb, float min_score, int BN, int Z,
            long long* __restrict__ topk_index, float* __restrict__ centers, unsigned char* __restrict__ valid) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= BN) return;
  const float* h = hm1d + size_t(i) * Z;
  float bv = h[0];
  int bz = 0;
  for (int z = 1; z < Z; ++z)
    if (h[z] > bv) { bv = h[z]; bz = z; }       // first maximum
  const long long ix = idx2d[size_t(i) * 2], iy = idx2d[size_t(i) * 2 + 1];
  if (topk_index) {
    topk_index[size_t(i) * 3 + 0] = ix;
    topk_index[size_t(i) * 3 + 1] = iy;
    topk_index[size_t(i) * 3 + 2] = bz;
  }
  const float conf = __fmul_rn(conf2d[i], bv);  // human_detection_net.py:101
  float* c = centers + size_t(i) * 7;
  // idx.float() * scale + bias: two roundings, no fma (human_detection_net.py:49)
  c[0] = __fadd_rn(__fmul_rn(float(ix), sb[0]), sb[3]);
  c[1] = __fadd_rn(__fmul_rn(float(iy), sb[1]), sb[4]);
  c[2] = __fadd_rn(__fmul_rn(float(bz), sb[2]), sb[5]);
  c[3] = (conf > min_score ? 1.0f : 0.0f) - 1.0f;
  c[4] = conf;
  c[5] = match_bbox[size_t(i) * 2];
  c[6] = match_bbox[size_t(i) * 2 + 1];
  if (valid) valid[i] = c[3] >= 0.0f;            // faster_voxelpose.py:45 (mask = proposal_centers[:, :, 3] >= 0)
}

// ProposalLayer.forward on its own (human_detection_net.py:44-65, eval branch): same arithmetic as the tail of k_proposals
__global__ void __launch_bounds__(64)
k_proposal_layer(const long long* __restrict__ topk_index, const float* __restrict__ topk_confs,
                 const float* __restrict__ match_bbox, const float* __restrict__ sb, float min_score, int BN,
                 float* __restrict__ centers) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= BN) return;
  const float conf = topk_confs[i];
  float* c = centers + size_t(i) * 7;
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = __fadd_rn(__fmul_rn(float(topk_index[size_t(i) * 3 + a]), sb[a]), sb[3 + a]);
  c[3] = (conf > min_score ? 1.0f : 0.0f) - 1.0f;
  c[4] = conf;
  c[5] = match_bbox[size_t(i) * 2];
  c[6] = match_bbox[size_t(i) * 2 + 1];
}

// ---- pose tracker (ABI 12): person identities across the frames of a camera sequence -----------------------------
// No reference counterpart (the reference returns a bag of poses per frame); the definition is in include/fvp.h.
// One workgroup of one wave per sequence.  Lane t owns track slot t (id and age in registers, T <= 64); the track poses,
// the frame's detections and the N x T cost matrix live in LDS.  The wave walks the batch's frames in order and skips the
// frames of other sequences, so a batch is one launch whatever B is; the state is read once at entry and written back
// once at exit.  Latency-bound like k_proposals (B * N * T * J distances, ~19 000 at the headline shape): nothing is tuned.
// The sets every lane needs (valid detections, live / matched tracks, matched detections) are wave-uniform bit masks.
// The strided loops are kept rolled (#pragma unroll 1): unrolled eight times with their remainder loops they cost 16 SGPR
// spills for loop-invariant predicates and buy nothing in a kernel that waits on one LDS read after another.
constexpr int kTrackDets = FVP_TRACK_MAX_DETS, kTrackSlots = FVP_TRACK_MAX_TRACKS;
static_assert(kTrackDets <= 32 && kTrackSlots <= 64, "masks: 32 detections, one lane per track slot");

__device__ __forceinline__ unsigned wave_or(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(64)
k_track_update(const float* __restrict__ poses, const int* __restrict__ frame_set, float* __restrict__ trk_pose,
               int* __restrict__ trk_id, int* __restrict__ trk_age, int* __restrict__ next_id, int* __restrict__ ids,
               int* __restrict__ slots, float* __restrict__ costs, int B, int N, int J, int nseq, int T, float gate,
               int max_age) {
  __shared__ float s_trk[kTrackSlots * FVP_MAX_JOINTS * 3];    // [T][J][3]
  __shared__ float s_det[kTrackDets * FVP_MAX_JOINTS * 3];     // [N][J][3] of the current frame
  __shared__ unsigned s_cost[kTrackDets * kTrackSlots];        // cost bits of entry n * T + t, ~0u = not eligible
  __shared__ int s_slot[kTrackDets], s_id[kTrackDets];         // per detection of the current frame
  __shared__ unsigned s_mcost[kTrackDets];
  const int s = blockIdx.x, lane = threadIdx.x, J3 = J * 3;
  const bool slot_lane = lane < T;
  int id = -1, age = 0;
  if (slot_lane) {
    id = trk_id[size_t(s) * T + lane];
    age = trk_age[size_t(s) * T + lane];
  }
  int next = next_id[s];
#pragma unroll 1
  for (int i = lane; i < T * J3; i += 64) s_trk[i] = trk_pose[size_t(s) * T * J3 + i];
  // entry e = n * T + t; this lane's entries are e = lane + 64 k: (n, t) advance by (q64, r64) with one carry
  const int n0 = lane / T, t0 = lane - n0 * T, q64 = 64 / T, r64 = 64 - q64 * T;
  const float fJ = float(J);

#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    const int fs = frame_set ? frame_set[b] : 0;
    if (fs != s) {
      // a frame of no sequence of this tracker: nobody owns it, workgroup 0 writes it as all invalid
      if (s == 0 && (fs < 0 || fs >= nseq) && lane < N) {
        ids[size_t(b) * N + lane] = -1;
        slots[size_t(b) * N + lane] = -1;
        costs[size_t(b) * N + lane] = -1.0f;
      }
      continue;
    }
    __syncthreads();                            // the previous frame's readers of s_det / s_slot are done
    const float* fp = poses + size_t(b) * N * J * 5;
#pragma unroll 1
    for (int i = lane; i < N * J; i += 64) {
      s_det[i * 3 + 0] = fp[size_t(i) * 5 + 0];
      s_det[i * 3 + 1] = fp[size_t(i) * 5 + 1];
      s_det[i * 3 + 2] = fp[size_t(i) * 5 + 2];
    }
    bool valid = false;
    if (lane < N) {
      valid = fp[size_t(lane) * J * 5 + 3] >= 0.0f;
      s_slot[lane] = -1;
    }
    const unsigned dets = wave_or(valid ? 1u << (lane & 31) : 0u);
    const bool live = slot_lane && id >= 0;
    const unsigned live_lo = wave_or(live && lane < 32 ? 1u << lane : 0u);
    const unsigned live_hi = wave_or(live && lane >= 32 ? 1u << (lane - 32) : 0u);
    const unsigned long long tracks = (unsigned long long)live_hi << 32 | live_lo;
    __syncthreads();

    // cost(n, t) = (d_0 + d_1 + ... + d_{J-1}) / J, every operation rounded on its own
#pragma unroll 1
    for (int e = lane, n = n0, t = t0; e < N * T; e += 64) {
      unsigned bits = ~0u;
      if ((dets >> n & 1u) && (tracks >> t & 1ull)) {
        const float* d = s_det + n * J3;
        const float* p = s_trk + t * J3;
        float sum = 0.0f;
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
          const float dx = __fsub_rn(d[3 * j], p[3 * j]), dy = __fsub_rn(d[3 * j + 1], p[3 * j + 1]),
                      dz = __fsub_rn(d[3 * j + 2], p[3 * j + 2]);
          const float dj = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
          sum = j == 0 ? dj : __fadd_rn(sum, dj);
        }
        const float cost = __fdiv_rn(sum, fJ);
        if (cost <= gate) bits = unsigned(__float_as_int(cost));      // (a NaN cost is never eligible)
      }
      s_cost[e] = bits;                         // read back by this lane only
      n += q64;
      t += r64;
      if (t >= T) { t -= T; ++n; }
    }

    // greedy assignment: the smallest (cost, n, t) among unassigned pairs, as the 64-bit key cost bits : n * T + t
    unsigned matched_d = 0;
    unsigned long long matched_t = 0;
    for (;;) {
      unsigned bc = ~0u, be = ~0u;
#pragma unroll 1
      for (int e = lane, n = n0, t = t0; e < N * T; e += 64) {
        const unsigned c = s_cost[e];
        if (c < bc && !(matched_d >> n & 1u) && !(matched_t >> t & 1ull)) { bc = c; be = unsigned(e); }   // (e ascends)
        n += q64;
        t += r64;
        if (t >= T) { t -= T; ++n; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned oc = __shfl_xor(bc, o), oe = __shfl_xor(be, o);
        if (oc < bc || (oc == bc && oe < be)) { bc = oc; be = oe; }
      }
      if (bc == ~0u) break;                     // wave-uniform
      const int n = int(be) / T, t = int(be) - n * T;
      matched_d |= 1u << n;
      matched_t |= 1ull << t;
      if (lane == t) {
        s_id[n] = id;
        s_slot[n] = t;
        s_mcost[n] = bc;
        age = 0;
      }
    }

    // unmatched live tracks age; past max_age the slot is free again, for this very frame's births
    if (live && !(matched_t >> lane & 1ull)) {
      ++age;
      if (age > max_age) id = -1;
    }
    // births in ascending n: the lowest free slot, else the live track of largest age (lowest slot on a tie).  T >= N: a
    // full table holds a track that was neither matched nor born in this frame, so the evicted one has age >= 1.
    const unsigned births = dets & ~matched_d;
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      if (!(births >> n & 1u)) continue;        // wave-uniform
      int ka = slot_lane ? (id < 0 ? int(0x80000000u) : -age) : 0x7fffffff, kl = lane;
      for (int o = 32; o > 0; o >>= 1) {
        const int oa = __shfl_xor(ka, o), ol = __shfl_xor(kl, o);
        if (oa < ka || (oa == ka && ol < kl)) { ka = oa; kl = ol; }
      }
      if (lane == kl) {
        id = next;
        age = 0;
        s_id[n] = next;
        s_slot[n] = kl;
        s_mcost[n] = unsigned(__float_as_int(-1.0f));
      }
      ++next;
    }
    __syncthreads();

    if (lane < N) {
      ids[size_t(b) * N + lane] = valid ? s_id[lane] : -1;
      slots[size_t(b) * N + lane] = valid ? s_slot[lane] : -1;
      costs[size_t(b) * N + lane] = valid ? __int_as_float(int(s_mcost[lane])) : -1.0f;
    }
    // every valid detection has a slot now (matched or born): its pose becomes the track's
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      const int t = s_slot[n];
      if (t < 0) continue;
#pragma unroll 1
      for (int r = lane; r < J3; r += 64) s_trk[t * J3 + r] = s_det[n * J3 + r];
    }
  }

  __syncthreads();
  if (slot_lane) {
    trk_id[size_t(s) * T + lane] = id;
    trk_age[size_t(s) * T + lane] = age;
  }
  if (lane == 0) next_id[s] = next;
#pragma unroll 1
  for (int i = lane; i < T * J3; i += 64) trk_pose[size_t(s) * T * J3 + i] = s_trk[i];
}

// ---- track smoother (ABI 13): a One-Euro filter per joint of every track slot ----------------------------------------
// The definition is in include/fvp.h.  Items (s, t, j) are independent over the whole batch: a thread owns one, keeps its
// six state floats and the slot's id / age in registers and walks the B frames in order, skipping the frames of other
// sequences - one launch per batch whatever B is, state read once at entry and written once at exit.  Every thread of a
// slot recomputes the slot's id / age transition (integer, deterministic); the j == 0 thread writes it.  The state is
// rewritten in place, so the J threads of a slot must all have read flt_id / flt_age before the j == 0 one stores them:
// a workgroup is one wave and holds 64 / J WHOLE slots (J <= 32: at least two; 60 of 64 lanes at J = 15), the loads of a
// wave precede its stores in program order, and no other wave touches the slot.  (The wave barrier behind the loads
// emits no instruction; it is the hand-over point the CPU emulation needs, whose lanes do not run in lock-step.)  No
// workgroup barrier, no LDS, no atomics.  Each element of smooth has one writer: the thread of the track slot a valid
// detection sits in, or thread t == n for an invalid one (T >= N).  Latency-bound like k_track_update (B dependent
// rounds of a few loads per thread): nothing is tuned.
constexpr int kSmoothThreads = 64;
static_assert(FVP_MAX_JOINTS <= kSmoothThreads, "a wave holds at least one whole slot");

__device__ __forceinline__ float one_euro_alpha(float fc, float rate) {
  const float r = __fdiv_rn(__fmul_rn(6.2831855f, fc), rate);
  return __fdiv_rn(r, __fadd_rn(r, 1.0f));
}

__global__ void __launch_bounds__(kSmoothThreads)
k_track_smooth(const float* __restrict__ poses, const int* __restrict__ frame_set, const int* __restrict__ ids,
               const int* __restrict__ slots, const float* __restrict__ conf, float* __restrict__ flt_pose,
               float* __restrict__ flt_vel, int* __restrict__ flt_id, int* __restrict__ flt_age,
               float* __restrict__ smooth, float* __restrict__ track_poses, int* __restrict__ track_state, int B, int N,
               int J, int nseq, int T, float rate, float min_cutoff, float beta, float d_cutoff, float conf_min,
               float damp, int max_age) {
  const int s = blockIdx.y, spb = kSmoothThreads / J, tl = int(threadIdx.x) / J;
  const int t = blockIdx.x * spb + tl, j = int(threadIdx.x) - tl * J;
  const bool active = tl < spb && t < T;
  const size_t st = size_t(s) * T + t, sj = (st * J + j) * 3;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
  int id = -1, age = 0;
  if (active) {
    x0 = flt_pose[sj]; x1 = flt_pose[sj + 1]; x2 = flt_pose[sj + 2];
    v0 = flt_vel[sj]; v1 = flt_vel[sj + 1]; v2 = flt_vel[sj + 2];
    id = flt_id[st];
    age = flt_age[st];
  }
  __builtin_amdgcn_wave_barrier();
  if (!active) return;
  const float dt = __fdiv_rn(1.0f, rate), a_d = one_euro_alpha(d_cutoff, rate);

#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    const int fs = frame_set ? frame_set[b] : 0;
    const size_t out = (size_t(b) * T + t) * J + j;            // this item's row of track_poses
    if (fs != s) {
      // a frame of no sequence: nobody owns it, the workgroups of sequence 0 write it as invalid
      if (s == 0 && (fs < 0 || fs >= nseq)) {
        if (track_poses) *reinterpret_cast<float4*>(track_poses + out * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (track_state && j == 0) {
          track_state[(size_t(b) * T + t) * 2] = -1;
          track_state[(size_t(b) * T + t) * 2 + 1] = 0;
        }
        if (smooth && t < N) {
          const size_t r = ((size_t(b) * N + t) * J + j) * 5;
#pragma unroll
          for (int c = 0; c < 5; ++c) smooth[r + c] = poses[r + c];
        }
      }
      continue;
    }
    // the detections of this frame that sit in track slot t (a bit per n; the lowest one is measured), and whether
    // detection slot n == t is an invalid one, which this thread copies through
    unsigned mine = 0;
    int first = -1;
    bool copy = false;
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      const int i = ids[size_t(b) * N + n], sl = slots[size_t(b) * N + n];
      const bool ok = i >= 0 && sl >= 0 && sl < T;
      if (ok && sl == t) {
        mine |= 1u << n;
        if (first < 0) first = n;
      }
      if (!ok && n == t) copy = true;
    }
    float flag = 0.0f;
    if (first >= 0) {
      const float* p = poses + ((size_t(b) * N + first) * J + j) * 5;
      const float m0 = p[0], m1 = p[1], m2 = p[2];
      const int nid = ids[size_t(b) * N + first];
      age = 0;
      if (id != nid) {                                         // a birth, a reuse or an eviction: the filter starts over
        id = nid;
        x0 = m0; x1 = m1; x2 = m2;
        v0 = v1 = v2 = 0.0f;
        flag = 1.0f;
      } else {
        const float e0 = __fsub_rn(m0, x0), e1 = __fsub_rn(m1, x1), e2 = __fsub_rn(m2, x2);
        bool measured = fabsf(e0) <= FLT_MAX && fabsf(e1) <= FLT_MAX && fabsf(e2) <= FLT_MAX;      // false for NaN, Inf
        if (measured && conf) measured = conf[(size_t(b) * N + first) * J + j] >= conf_min;
        if (measured) {
          v0 = __fadd_rn(v0, __fmul_rn(a_d, __fsub_rn(__fmul_rn(e0, rate), v0)));
          v1 = __fadd_rn(v1, __fmul_rn(a_d, __fsub_rn(__fmul_rn(e1, rate), v1)));
          v2 = __fadd_rn(v2, __fmul_rn(a_d, __fsub_rn(__fmul_rn(e2, rate), v2)));
          const float sp = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(v0, v0), __fmul_rn(v1, v1)), __fmul_rn(v2, v2)));
          const float a = one_euro_alpha(__fadd_rn(min_cutoff, __fmul_rn(beta, sp)), rate);
          x0 = __fadd_rn(x0, __fmul_rn(a, e0));
          x1 = __fadd_rn(x1, __fmul_rn(a, e1));
          x2 = __fadd_rn(x2, __fmul_rn(a, e2));
          flag = 1.0f;
        } else {
          v0 = __fmul_rn(v0, damp); v1 = __fmul_rn(v1, damp); v2 = __fmul_rn(v2, damp);
          x0 = __fadd_rn(x0, __fmul_rn(v0, dt));
          x1 = __fadd_rn(x1, __fmul_rn(v1, dt));
          x2 = __fadd_rn(x2, __fmul_rn(v2, dt));
        }
      }
    } else if (id >= 0) {
      ++age;
      if (age > max_age) {                                     // the slot is free
        id = -1;
        age = 0;
      } else {                                                 // coasting: the predicted update
        v0 = __fmul_rn(v0, damp); v1 = __fmul_rn(v1, damp); v2 = __fmul_rn(v2, damp);
        x0 = __fadd_rn(x0, __fmul_rn(v0, dt));
        x1 = __fadd_rn(x1, __fmul_rn(v1, dt));
        x2 = __fadd_rn(x2, __fmul_rn(v2, dt));
      }
    }
    if (smooth) {
#pragma unroll 1
      for (int n = first; n >= 0 && n < N; ++n) {
        if (!(mine >> n & 1u)) continue;
        const size_t r = ((size_t(b) * N + n) * J + j) * 5;
        smooth[r] = x0;
        smooth[r + 1] = x1;
        smooth[r + 2] = x2;
        smooth[r + 3] = poses[r + 3];
        smooth[r + 4] = poses[r + 4];
      }
      if (copy) {
        const size_t r = ((size_t(b) * N + t) * J + j) * 5;
#pragma unroll
        for (int c = 0; c < 5; ++c) smooth[r + c] = poses[r + c];
      }
    }
    const bool live = id >= 0;
    if (track_poses)
      *reinterpret_cast<float4*>(track_poses + out * 4) =
          live ? make_float4(x0, x1, x2, flag) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (track_state && j == 0) {
      track_state[(size_t(b) * T + t) * 2] = id;
      track_state[(size_t(b) * T + t) * 2 + 1] = age;
    }
  }

  flt_pose[sj] = x0; flt_pose[sj + 1] = x1; flt_pose[sj + 2] = x2;
  flt_vel[sj] = v0; flt_vel[sj + 1] = v1; flt_vel[sj + 2] = v2;
  if (j == 0) {
    flt_id[st] = id;
    flt_age[st] = age;
  }
}

// ---- limb model (ABI 22): bone lengths per track, and poses constrained to them ---------------------------------------------
// The definitions are in include/fvp.h.  k_limb_learn is k_track_smooth's shape with a limb where that has a joint: a thread
// owns one (s, t, l), keeps len, var, cnt, out and the slot's id in registers and walks the B frames in order - one launch per
// batch, state read once at entry and written once at exit.  Every thread of a slot recomputes the id transition; the l == 0
// thread stores limb_id.  The state is rewritten in place, so the same hazard applies: a workgroup is one wave that holds
// 64 / L WHOLE slots (56 of 64 lanes at L = 14, 57 at L = 19, one slot from L = 33 on), its loads precede its stores in
// program order, and no other wave touches the slot; the wave barrier behind the entry loads emits no instruction and is the
// hand-over point of the CPU emulation.  The limb table travels in the kernel's parameter block (uint8 pairs), as in the draw
// kernels.  Each element of the outputs has one writer: the thread of the track slot a valid detection sits in, or thread
// t == n for an invalid one (T >= N).  No LDS, no atomics, no workgroup barrier.  Latency-bound: nothing is tuned.
constexpr int kLimbThreads = 64;
static_assert(FVP_LIMB_MAX <= kLimbThreads, "a wave holds at least one whole slot");
static_assert(FVP_MAX_JOINTS <= 32, "k_limb_fit keeps the support mask in one register");

struct LimbPrm {
  uint8_t limb[FVP_LIMB_MAX][2];
};

__device__ __forceinline__ bool limb_finite(float x0, float x1, float x2) {
  return fabsf(x0) <= FLT_MAX && fabsf(x1) <= FLT_MAX && fabsf(x2) <= FLT_MAX;                     // false for NaN, Inf
}

__device__ __forceinline__ float limb_norm(float d0, float d1, float d2) {
  return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
}

__global__ void __launch_bounds__(kLimbThreads)
k_limb_learn(const float* __restrict__ poses, const int* __restrict__ frame_set, const int* __restrict__ ids,
             const int* __restrict__ slots, const float* __restrict__ conf, const LimbPrm prm, int L,
             float* __restrict__ limb_len, float* __restrict__ limb_var, int* __restrict__ limb_cnt,
             int* __restrict__ limb_out, int* __restrict__ limb_id, float* __restrict__ target,
             float* __restrict__ limb_obs, int* __restrict__ limb_state, int B, int N, int J, int nseq, int T,
             float conf_min, int min_frames, int window, float gate_sigma, float gate_mm, int relearn) {
  const int s = blockIdx.y, spb = kLimbThreads / L, tl = int(threadIdx.x) / L;
  const int t = blockIdx.x * spb + tl, l = int(threadIdx.x) - tl * L;
  const bool active = tl < spb && t < T;
  const size_t st = size_t(s) * T + t, sl = st * L + l;
  float len = 0.0f, var = 0.0f;
  int cnt = 0, nout = 0, id = -1;
  if (active) {
    len = limb_len[sl];
    var = limb_var[sl];
    cnt = limb_cnt[sl];
    nout = limb_out[sl];
    id = limb_id[st];
  }
  __builtin_amdgcn_wave_barrier();
  if (!active) return;
  const int ji = prm.limb[l][0], jk = prm.limb[l][1];

#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    const int fs = frame_set ? frame_set[b] : 0;
    if (fs != s) {
      // a frame of no sequence: nobody owns it, the workgroups of sequence 0 write it as invalid
      if (s == 0 && (fs < 0 || fs >= nseq) && t < N) {
        const size_t o = (size_t(b) * N + t) * L + l;
        target[o] = 0.0f;
        limb_obs[2 * o] = -1.0f;
        limb_obs[2 * o + 1] = 0.0f;
        limb_state[o] = FVP_LIMB_INVALID;
      }
      continue;
    }
    // the detections of this frame that sit in track slot t (a bit per n; the lowest one is measured), and whether
    // detection slot n == t is an invalid one, which this thread writes as such
    unsigned mine = 0;
    int first = -1;
    bool inval = false;
#pragma unroll 1
    for (int n = 0; n < N; ++n) {
      const int i = ids[size_t(b) * N + n], sn = slots[size_t(b) * N + n];
      const bool ok = i >= 0 && sn >= 0 && sn < T;
      if (ok && sn == t) {
        mine |= 1u << n;
        if (first < 0) first = n;
      }
      if (!ok && n == t) inval = true;
    }
    if (inval) {
      const size_t o = (size_t(b) * N + t) * L + l;
      target[o] = 0.0f;
      limb_obs[2 * o] = -1.0f;
      limb_obs[2 * o + 1] = 0.0f;
      limb_state[o] = FVP_LIMB_INVALID;
    }
    if (first < 0) continue;                                   // the lengths survive coasting
    const size_t row = (size_t(b) * N + first) * J;
    const int nid = ids[size_t(b) * N + first];
    if (id != nid) {                                           // a birth, a reuse or an eviction: every limb starts over
      id = nid;
      len = var = 0.0f;
      cnt = nout = 0;
    }
    const float* pi = poses + (row + ji) * 5;
    const float* pk = poses + (row + jk) * 5;
    const float a0 = pi[0], a1 = pi[1], a2 = pi[2], c0 = pk[0], c1 = pk[1], c2 = pk[2];
    bool measured = limb_finite(a0, a1, a2) && limb_finite(c0, c1, c2);
    if (measured && conf) measured = conf[row + ji] >= conf_min && conf[row + jk] >= conf_min;
    float d = -1.0f, e = 0.0f;
    int state = FVP_LIMB_NOT_MEASURED;
    if (measured) {
      const float dd = limb_norm(__fsub_rn(c0, a0), __fsub_rn(c1, a1), __fsub_rn(c2, a2));
      if (dd > 0.0f && dd <= FLT_MAX) {
        d = dd;
        e = __fsub_rn(d, len);
        bool pass = true;
        if (cnt >= min_frames) pass = fabsf(e) <= fmaxf(__fmul_rn(gate_sigma, sqrtf(var)), gate_mm);
        if (pass) {
          nout = 0;
          cnt = cnt + 1 < window ? cnt + 1 : window;
          const float g = __fdiv_rn(1.0f, float(cnt));
          len = __fadd_rn(len, __fmul_rn(g, e));
          var = __fadd_rn(var, __fmul_rn(g, __fsub_rn(__fmul_rn(e, __fsub_rn(d, len)), var)));
          state = cnt >= min_frames ? FVP_LIMB_LEARNED : FVP_LIMB_LEARNING;
        } else if (++nout > relearn) {
          len = d;
          var = 0.0f;
          cnt = 1;
          nout = 0;
          state = FVP_LIMB_RELEARNED;
        } else {
          state = FVP_LIMB_OUTLIER;
        }
      }
    }
    const float tg = cnt >= min_frames ? len : 0.0f;
#pragma unroll 1
    for (int n = first; n < N; ++n) {
      if (!(mine >> n & 1u)) continue;
      const size_t o = (size_t(b) * N + n) * L + l;
      target[o] = tg;
      limb_obs[2 * o] = d;
      limb_obs[2 * o + 1] = e;
      limb_state[o] = state;
    }
  }

  limb_len[sl] = len;
  limb_var[sl] = var;
  limb_cnt[sl] = cnt;
  limb_out[sl] = nout;
  if (l == 0) limb_id[st] = id;
}

// k_limb_fit: one lane per person (b, n), 64 people per workgroup (one wave).  The sweeps index joints dynamically, which in a
// register array would become scratch, so the workgroup stages its poses in LDS as [J * 3][64], lane-minor: a lane's LDS
// access always hits bank = lane, conflict-free on the 64 x 4 B banks; 24 KB at J = 32.  The [J][5] rows of the 64 people are
// one contiguous piece of memory: loaded coalesced by the whole workgroup and transposed on the way in, written back the same
// way (columns 3:5 straight from the input), so fitted may be poses itself - a workgroup has read all of its rows before it
// writes one and no other workgroup touches them.  The support mask is one register per lane; the limb pair of step l is
// uniform over the wave, a scalar load from the parameter block; target is read from global memory in every sweep (a load
// whose address does not depend on the chain).  Latency-bound: iters * L dependent steps per lane of one sqrt, one divide
// and a dozen LDS accesses each; nothing beyond the one launch is tuned.
__global__ void __launch_bounds__(kLimbThreads)
k_limb_fit(const float* poses, const int* __restrict__ ids, const float* __restrict__ conf,
           const float* __restrict__ target, const LimbPrm prm, int L, float* fitted, float* __restrict__ resid, int BN, int J,
           float conf_min, float stiffness, int iters) {
  __shared__ float s_y[FVP_MAX_JOINTS * 3 * kLimbThreads];
  const int lane = threadIdx.x, base = blockIdx.x * kLimbThreads, row = J * 5;
  const int np = BN - base < kLimbThreads ? BN - base : kLimbThreads, total = np * row;
  const size_t g0 = size_t(base) * row;
#pragma unroll 1
  for (int i = lane; i < total; i += kLimbThreads) {
    const int p = i / row, r = i - p * row, j = r / 5, c = r - j * 5;
    if (c < 3) s_y[(j * 3 + c) * kLimbThreads + p] = poses[g0 + i];
  }
  __syncthreads();

  const size_t me = size_t(base) + lane;
  float* y = s_y + lane;
  bool valid = false;
  if (lane < np) valid = poses[me * row + 3] >= 0.0f && (!ids || ids[me] >= 0);
  if (valid) {
    unsigned m = 0;                                            // bit j: joint j of the input pose is supported
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
      bool ok = limb_finite(y[(j * 3) * kLimbThreads], y[(j * 3 + 1) * kLimbThreads], y[(j * 3 + 2) * kLimbThreads]);
      if (ok && conf) ok = conf[me * J + j] >= conf_min;
      m |= unsigned(ok) << j;
    }
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll 1
      for (int l = 0; l < L; ++l) {
        const float tg = target[me * L + l];
        if (!(tg > 0.0f)) continue;                            // unconstrained: 0, negative, NaN
        const int i = prm.limb[l][0], k = prm.limb[l][1];
        float* yi = y + i * 3 * kLimbThreads;
        float* yk = y + k * 3 * kLimbThreads;
        const float i0 = yi[0], i1 = yi[kLimbThreads], i2 = yi[2 * kLimbThreads];
        const float k0 = yk[0], k1 = yk[kLimbThreads], k2 = yk[2 * kLimbThreads];
        const float d0 = __fsub_rn(k0, i0), d1 = __fsub_rn(k1, i1), d2 = __fsub_rn(k2, i2);
        const float d = limb_norm(d0, d1, d2);
        if (!(d > 0.0f && d <= FLT_MAX)) continue;
        const float sc = __fdiv_rn(__fmul_rn(stiffness, __fsub_rn(d, tg)), d);
        const bool mi = m >> i & 1u, mk = m >> k & 1u;
        const float wi = mi == mk ? 0.5f : (mi ? 0.0f : 1.0f), wk = mi == mk ? 0.5f : (mi ? 1.0f : 0.0f);
        const float si = __fmul_rn(wi, sc), sk = __fmul_rn(wk, sc);
        yi[0] = __fadd_rn(i0, __fmul_rn(si, d0));
        yi[kLimbThreads] = __fadd_rn(i1, __fmul_rn(si, d1));
        yi[2 * kLimbThreads] = __fadd_rn(i2, __fmul_rn(si, d2));
        yk[0] = __fsub_rn(k0, __fmul_rn(sk, d0));
        yk[kLimbThreads] = __fsub_rn(k1, __fmul_rn(sk, d1));
        yk[2 * kLimbThreads] = __fsub_rn(k2, __fmul_rn(sk, d2));
      }
    }
  }
  if (resid && lane < np) {
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
      float r = 0.0f;
      const float tg = target[me * L + l];
      if (valid && tg > 0.0f) {
        const float* yi = y + prm.limb[l][0] * 3 * kLimbThreads;
        const float* yk = y + prm.limb[l][1] * 3 * kLimbThreads;
        const float d = limb_norm(__fsub_rn(yk[0], yi[0]), __fsub_rn(yk[kLimbThreads], yi[kLimbThreads]),
                                  __fsub_rn(yk[2 * kLimbThreads], yi[2 * kLimbThreads]));
        if (d > 0.0f && d <= FLT_MAX) r = __fsub_rn(d, tg);
      }
      resid[me * L + l] = r;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int i = lane; i < total; i += kLimbThreads) {
    const int p = i / row, r = i - p * row, j = r / 5, c = r - j * 5;
    fitted[g0 + i] = c < 3 ? s_y[(j * 3 + c) * kLimbThreads + p] : poses[g0 + i];
  }
}

// ---- person re-identification (ABI 20): a gallery of retired tracks per sequence -----------------------------------------
// The definition is in include/fvp.h.  One workgroup of 256 threads per sequence walks the batch's frames in order and skips
// the frames of other sequences, as k_track_update does.  Thread (p, bin) = tid owns counter (p, bin) of EVERY slot and gallery
// signature of its sequence: accumulating, halving, storing a retired slot in the gallery and clearing are thread-private
// read-modify-writes of global memory with no hand-over between threads, so the signatures (up to 2 x 64 KB) need no LDS.  A
// part is a wave (64 bins): its sums Ca, Cg and the int64 intersection are wave reductions over shuffles.  The scalars of the
// slots and of the gallery live in LDS; every thread reads them and takes the same branches, thread 0 alone writes them.  The
// slot scalars are double-buffered per frame (read copy `cur`, written copy `cur ^ 1`; every slot is rewritten every frame), so
// a wave that lags at the start of slot t never sees thread 0's end-of-slot write; the gallery scalars change between two
// barriers.  Latency-bound: B * T dependent rounds of a few loads, and a decision (G rounds of shuffles) once per track.
constexpr int kReidThreads = FVP_SIG_MAX_PARTS * FVP_SIG_BINS, kReidGallery = FVP_REID_MAX_GALLERY;
static_assert(FVP_SIG_BINS == 64, "a wave sums a part");

struct ReidPrm {
  int max_age, min_samples, min_frames, window, gallery_max_age;
  float sim_min, margin;
};

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ long long wave_sum64(long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = unsigned(__shfl_xor(int(v), o)), hi = unsigned(__shfl_xor(int(v >> 32), o));
    v += (long long)((unsigned long long)hi << 32 | lo);
  }
  return v;
}

__global__ void __launch_bounds__(kReidThreads)
k_track_reid(const int* __restrict__ ids, const int* __restrict__ slots, const int* __restrict__ sig,
             const int* __restrict__ sig_count, const int* __restrict__ frame_set, int* __restrict__ slot_sig,
             int* __restrict__ slot_tid, int* __restrict__ slot_pid, int* __restrict__ slot_frames,
             int* __restrict__ slot_age, float* __restrict__ slot_sim, int* __restrict__ gal_sig, int* __restrict__ gal_pid,
             int* __restrict__ gal_age, int* __restrict__ pids, int* __restrict__ reid_state, float* __restrict__ reid_sim,
             int B, int N, int nseq, int T, int G, int P, ReidPrm q) {
  __shared__ int s_st[2][5][kTrackSlots];                  // slot scalars: tid, pid, frames, age, sim bits
  __shared__ int s_n[kTrackSlots];                         // the frame's detection of every slot, -1 = none
  __shared__ int s_gpid[kReidGallery], s_gage[kReidGallery], s_gfreed[kReidGallery];
  __shared__ long long s_inter[kReidGallery][FVP_SIG_MAX_PARTS];
  __shared__ int s_cg[kReidGallery][FVP_SIG_MAX_PARTS], s_ca[FVP_SIG_MAX_PARTS];
  __shared__ float s_sim[kReidGallery];
  const int s = blockIdx.x, tid = threadIdx.x, p = tid >> 6, lane = tid & 63, cells = P * FVP_SIG_BINS;
  const bool active = p < P;                               // wave-uniform
  const int none = __float_as_int(-1.0f);
  int* ssig = slot_sig + size_t(s) * T * cells + tid;      // this thread's counter of slot t: ssig[t * cells]
  int* gsig = gal_sig + size_t(s) * G * cells + tid;
  // The state and output pointers become per-thread addresses in vector registers here, opaque to the optimiser: kept as
  // seventeen scalar bases they are live from the first load to the last store and the kernel spills scalar registers.
  int* p_tid = slot_tid + size_t(s) * T + tid;
  int* p_pid = slot_pid + size_t(s) * T + tid;
  int* p_frames = slot_frames + size_t(s) * T + tid;
  int* p_age = slot_age + size_t(s) * T + tid;
  float* p_sim = slot_sim + size_t(s) * T + tid;
  int* p_gpid = gal_pid + size_t(s) * G + tid;
  int* p_gage = gal_age + size_t(s) * G + tid;
  int* o_pid = pids + tid;
  int* o_state = reid_state + tid;
  float* o_sim = reid_sim + tid;
  FVP_OPAQUE_V(ssig); FVP_OPAQUE_V(gsig); FVP_OPAQUE_V(p_tid); FVP_OPAQUE_V(p_pid); FVP_OPAQUE_V(p_frames);
  FVP_OPAQUE_V(p_age); FVP_OPAQUE_V(p_sim); FVP_OPAQUE_V(p_gpid); FVP_OPAQUE_V(p_gage);
  FVP_OPAQUE_V(o_pid); FVP_OPAQUE_V(o_state); FVP_OPAQUE_V(o_sim);
  const int* v_sig = sig + tid;                            // (the two signature inputs likewise)
  const int* v_cnt = sig_count;
  FVP_OPAQUE_V(v_sig); FVP_OPAQUE_V(v_cnt);
  if (tid < T) {
    s_st[0][0][tid] = *p_tid;
    s_st[0][1][tid] = *p_pid;
    s_st[0][2][tid] = *p_frames;
    s_st[0][3][tid] = *p_age;
    s_st[0][4][tid] = __float_as_int(*p_sim);
  }
  if (tid < G) {
    s_gpid[tid] = *p_gpid;
    s_gage[tid] = *p_gage;
  }
  int cur = 0;

#pragma unroll 1
  for (int b = 0; b < B; ++b) {
    const int fs = frame_set ? frame_set[b] : 0;
    if (fs != s) {
      // a frame of no sequence: nobody owns it, workgroup 0 writes it as all invalid
      if (s == 0 && (fs < 0 || fs >= nseq) && tid < N) {
        o_pid[size_t(b) * N] = -1;
        o_state[size_t(b) * N] = -1;
        o_sim[size_t(b) * N] = -1.0f;
      }
      continue;
    }
    const int* fid = ids + size_t(b) * N;
    const int* fsl = slots + size_t(b) * N;
    __syncthreads();                                       // the state as loaded / as the previous frame left it
    if (tid < T) {
      int first = -1;
#pragma unroll 1
      for (int n = N - 1; n >= 0; --n)
        if (fid[n] >= 0 && fsl[n] == tid) first = n;
      s_n[tid] = first;
    }
    if (tid < G) {                                         // 1. gallery ageing
      int freed = 0;
      if (s_gpid[tid] >= 0) {
        const int age = s_gage[tid] + 1;
        freed = q.gallery_max_age > 0 && age > q.gallery_max_age;
        s_gage[tid] = freed ? 0 : age;
        if (freed) s_gpid[tid] = -1;
      }
      s_gfreed[tid] = freed;
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < G; ++g)
      if (s_gfreed[g] && active) gsig[size_t(g) * cells] = 0;

#pragma unroll 1
    for (int t = 0; t < T; ++t) {                          // 2. the slots in ascending order; every branch is uniform
      const int n = s_n[t];
      int id = s_st[cur][0][t], pid = s_st[cur][1][t], frames = s_st[cur][2][t], age = s_st[cur][3][t];
      int simb = s_st[cur][4][t];
      const int nid = n >= 0 ? fid[n] : -1;
      if (id >= 0 && (n >= 0 ? nid != id : age + 1 > q.max_age)) {           // a. retire
        if (frames >= q.min_frames) {
          int gsel = -1, oldest = -1, gold = 0;
#pragma unroll 1
          for (int g = 0; g < G; ++g) {
            if (s_gpid[g] < 0) {
              if (gsel < 0) gsel = g;                                         // the lowest free entry
            } else if (s_gage[g] > oldest) {                                  // else the largest age, lowest index on a tie
              oldest = s_gage[g];
              gold = g;
            }
          }
          if (gsel < 0) gsel = gold;
          if (active) gsig[size_t(gsel) * cells] = ssig[size_t(t) * cells];
          __syncthreads();                                 // every thread has scanned the gallery scalars
          if (tid == 0) {
            s_gpid[gsel] = pid >= 0 ? pid : id;
            s_gage[gsel] = 0;
          }
          __syncthreads();
        }
        if (active) ssig[size_t(t) * cells] = 0;
        id = -1; pid = -1; frames = 0; age = 0; simb = none;
      }
      if (n < 0 && id >= 0) ++age;                                            // b. coast
      if (n >= 0) {
        if (id != nid) id = nid;                                              // c. birth: the slot is in the cleared state
        age = 0;                                                              // d. accumulate
        int cnt = 0;
#pragma unroll 1
        for (int pp = 0; pp < P; ++pp) cnt += v_cnt[(size_t(b) * N + n) * P + pp];
        if (cnt >= q.min_samples) {
          if (active) {
            int a = ssig[size_t(t) * cells];
            if (frames == q.window) a >>= 1;
            ssig[size_t(t) * cells] = a + v_sig[(size_t(b) * N + n) * cells];
          }
          if (frames == q.window) frames = q.window >> 1;
          ++frames;
        }
      }
      if (id >= 0 && pid == -1 && frames >= q.min_frames) {                   // e. decide
        const int a = active ? ssig[size_t(t) * cells] : 0;
        const int Ca = wave_sum(a);
        if (lane == 0) s_ca[p] = Ca;
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
          if (s_gpid[g] < 0) continue;
          const int gv = active ? gsig[size_t(g) * cells] : 0;
          const int Cg = wave_sum(gv);
          const long long x = (long long)a * Cg, y = (long long)gv * Ca;
          const long long inter = wave_sum64(x < y ? x : y);
          if (lane == 0) {
            s_inter[g][p] = inter;
            s_cg[g][p] = Cg;
          }
        }
        __syncthreads();
        if (tid < G && s_gpid[tid] >= 0) {
          double acc = 0.0;
          int parts = 0;
#pragma unroll 1
          for (int pp = 0; pp < P; ++pp) {
            const int ca = s_ca[pp], cg = s_cg[tid][pp];
            if (ca > 0 && cg > 0) {
              acc = acc + double(s_inter[tid][pp]) / (double(ca) * double(cg));
              ++parts;
            }
          }
          s_sim[tid] = parts ? float(acc / double(parts)) : 0.0f;
        }
        __syncthreads();
        int best = -1;
        float sb = 0.0f, s2 = 0.0f;
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
          if (s_gpid[g] < 0) continue;
          const float v = s_sim[g];
          if (best < 0) {
            best = g;
            sb = v;
          } else if (v > sb) {                             // (a tie keeps the lower g)
            s2 = sb;
            best = g;
            sb = v;
          } else if (v > s2) {
            s2 = v;
          }
        }
        if (best >= 0 && sb >= q.sim_min && __fsub_rn(sb, s2) >= q.margin) {  // adopt: the entry is freed
          pid = s_gpid[best];
          if (active) gsig[size_t(best) * cells] = 0;
          __syncthreads();                                 // every thread has read the gallery scalars
          if (tid == 0) {
            s_gpid[best] = -1;
            s_gage[best] = 0;
          }
          __syncthreads();
        } else {
          pid = id;
        }
        simb = best >= 0 ? __float_as_int(sb) : none;
      }
      if (tid == 0) {
        s_st[cur ^ 1][0][t] = id;
        s_st[cur ^ 1][1][t] = pid;
        s_st[cur ^ 1][2][t] = frames;
        s_st[cur ^ 1][3][t] = age;
        s_st[cur ^ 1][4][t] = simb;
      }
    }
    cur ^= 1;
    __syncthreads();
    if (tid < N) {                                         // 3. outputs
      const int t = fsl[tid];
      int op = -1, os = -1, ob = none;
      if (fid[tid] >= 0 && t >= 0 && t < T) {
        const int id = s_st[cur][0][t], pid = s_st[cur][1][t];
        op = pid >= 0 ? pid : id;
        os = pid < 0 ? 0 : pid == id ? 1 : 2;
        ob = s_st[cur][4][t];
      }
      o_pid[size_t(b) * N] = op;
      o_state[size_t(b) * N] = os;
      o_sim[size_t(b) * N] = __int_as_float(ob);
    }
  }

  __syncthreads();
  if (tid < T) {
    *p_tid = s_st[cur][0][tid];
    *p_pid = s_st[cur][1][tid];
    *p_frames = s_st[cur][2][tid];
    *p_age = s_st[cur][3][tid];
    *p_sim = __int_as_float(s_st[cur][4][tid]);
  }
  if (tid < G) {
    *p_gpid = s_gpid[tid];
    *p_gage = s_gage[tid];
  }
}

}  // namespace fvp

using namespace fvp;

extern "C" int fvp_nms_topk(const float* hm2d, int B, int X, int Y, int N, float* vals, int64_t* idx, int64_t* flat,
                            fvp_stream_t s) {
  FVP_REQUIRE(hm2d && vals && idx && flat && B >= 0 && X > 0 && Y > 0 && N > 0);
  const size_t lds = size_t(X) * Y * 4 + 128;
  // limit: the map + 32 words must fit the CU's 160 KB of LDS (X * Y <= 40 928, e.g. 200 x 200)
  FVP_LIMIT(lds <= 160 * 1024 && N <= X * Y && X * Y <= kNmsMaxCellsLds * kNmsThreads);
  const bool reg = X * Y <= kNmsCells * kNmsThreads;
  auto k = reg ? &k_nms_topk<true> : &k_nms_topk<false>;
  static LdsOptIn optin[2];
  if (lds_opt_in(optin[reg], reinterpret_cast<const void*>(k), lds)) return FVP_ELIMIT;
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k, dim3(B), dim3(kNmsThreads), lds, as_stream(s), hm2d, X, Y, N, vals,
                     reinterpret_cast<long long*>(idx), reinterpret_cast<long long*>(flat));
  return launch_status();
}

extern "C" int fvp_gather_proposals(const float* bbox_map, const float* cubes, const int64_t* flat, int B, int J,
                                    int X, int Y, int Z, int N, float* bbox_flat, float* match_bbox, float* feat1d,
                                    fvp_stream_t s) {
  FVP_REQUIRE(bbox_map && flat && match_bbox && B >= 0 && (cubes != nullptr) == (feat1d != nullptr));
  if (B == 0) return 0;
  long total = cubes ? long(B) * N * J * Z : 0;
  if (bbox_flat && long(B) * X * Y * 2 > total) total = long(B) * X * Y * 2;
  if (long(B) * N * 2 > total) total = long(B) * N * 2;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_gather, dim3(unsigned((total + 255) / 256)), dim3(256), 0, as_stream(s), bbox_map, cubes,
                     reinterpret_cast<const long long*>(flat), B, J, X * Y, Z, N, bbox_flat, match_bbox, feat1d);
  return launch_status();
}

extern "C" int fvp_proposals(const float* hm1d, const float* conf2d, const int64_t* idx2d, const float* match_bbox,
                             const float* sb, float min_score, int B, int N, int Z, int64_t* topk_index,
                             float* centers, uint8_t* valid, fvp_stream_t s) {
  FVP_REQUIRE(hm1d && conf2d && idx2d && match_bbox && sb && centers && B >= 0 && N > 0 && Z > 0);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_proposals, dim3(ceil_div(B * N, 64)), dim3(64), 0, as_stream(s), hm1d, conf2d,
                     reinterpret_cast<const long long*>(idx2d), match_bbox, sb, min_score, B * N, Z,
                     reinterpret_cast<long long*>(topk_index), centers, valid);
  return launch_status();
}

extern "C" int fvp_proposal_layer(const int64_t* topk_index, const float* topk_confs, const float* match_bbox,
                                  const float* sb, float min_score, int B, int N, float* centers, fvp_stream_t s) {
  FVP_REQUIRE(topk_index && topk_confs && match_bbox && sb && centers && B >= 0 && N > 0);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_proposal_layer, dim3(ceil_div(B * N, 64)), dim3(64), 0, as_stream(s),
                     reinterpret_cast<const long long*>(topk_index), topk_confs, match_bbox, sb, min_score, B * N, centers);
  return launch_status();
}

extern "C" int fvp_track_update(const float* fused_poses, const int32_t* frame_set, float* trk_pose, int32_t* trk_id,
                                int32_t* trk_age, int32_t* next_id, int32_t* ids, int32_t* slots, float* costs, int B,
                                int N, int J, int nseq, int T, float gate_mm, int max_age, fvp_stream_t s) {
  FVP_REQUIRE(fused_poses && trk_pose && trk_id && trk_age && next_id && ids && slots && costs);
  FVP_REQUIRE(B >= 0 && N > 0 && J > 0 && nseq > 0 && T >= N && max_age >= 0);
  FVP_LIMIT(N <= kTrackDets && T <= kTrackSlots && J <= FVP_MAX_JOINTS);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_track_update, dim3(nseq), dim3(64), 0, as_stream(s), fused_poses, frame_set, trk_pose, trk_id,
                     trk_age, next_id, ids, slots, costs, B, N, J, nseq, T, gate_mm, max_age);
  return launch_status();
}

extern "C" int fvp_track_smooth(const float* fused_poses, const int32_t* frame_set, const int32_t* ids,
                                const int32_t* slots, const float* joint_conf, float* flt_pose, float* flt_vel,
                                int32_t* flt_id, int32_t* flt_age, float* smooth, float* track_poses,
                                int32_t* track_state, int B, int N, int J, int nseq, int T, float rate_hz,
                                float min_cutoff, float beta, float d_cutoff, float conf_min, float damp, int max_age,
                                fvp_stream_t s) {
  FVP_REQUIRE(fused_poses && ids && slots && flt_pose && flt_vel && flt_id && flt_age);
  FVP_REQUIRE(smooth || track_poses || track_state);
  FVP_REQUIRE(B >= 0 && N > 0 && J > 0 && nseq > 0 && T >= N && max_age >= 0);
  // written so that a NaN fails every one of them
  FVP_REQUIRE(rate_hz > 0.0f && min_cutoff > 0.0f && d_cutoff > 0.0f && beta >= 0.0f && damp >= 0.0f && damp <= 1.0f);
  FVP_LIMIT(N <= kTrackDets && T <= kTrackSlots && J <= FVP_MAX_JOINTS);
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_track_smooth, dim3(ceil_div(T, kSmoothThreads / J), nseq), dim3(kSmoothThreads), 0, as_stream(s),
                     fused_poses, frame_set, ids, slots, joint_conf, flt_pose, flt_vel, flt_id, flt_age, smooth,
                     track_poses, track_state, B, N, J, nseq, T, rate_hz, min_cutoff, beta, d_cutoff, conf_min, damp,
                     max_age);
  return launch_status();
}

// the checks of the limb table both limb exports share (behind their limit checks: L <= FVP_LIMB_MAX); the pairs go into prm
static int limb_table(const int32_t* limbs, int L, int J, LimbPrm& prm) {
  for (int l = 0; l < L; ++l) {
    const int i = limbs[2 * l], k = limbs[2 * l + 1];
    FVP_REQUIRE(i >= 0 && i < J && k >= 0 && k < J && i != k);
    prm.limb[l][0] = uint8_t(i);
    prm.limb[l][1] = uint8_t(k);
  }
  return 0;
}

extern "C" int fvp_limb_learn(const float* fused_poses, const int32_t* frame_set, const int32_t* ids, const int32_t* slots,
                              const float* joint_conf, const int32_t* limbs, int L, float* limb_len, float* limb_var,
                              int32_t* limb_cnt, int32_t* limb_out, int32_t* limb_id, float* target, float* limb_obs,
                              int32_t* limb_state, int B, int N, int J, int nseq, int T, float conf_min, int min_frames,
                              int window, float gate_sigma, float gate_mm, int relearn, fvp_stream_t s) {
  FVP_REQUIRE(fused_poses && ids && slots && limbs && limb_len && limb_var && limb_cnt && limb_out && limb_id);
  FVP_REQUIRE(target && limb_obs && limb_state);
  FVP_REQUIRE(B >= 0 && N > 0 && J > 0 && L > 0 && nseq > 0 && T >= N);
  FVP_REQUIRE(min_frames >= 1 && window >= min_frames && relearn >= 0);
  FVP_REQUIRE(gate_sigma >= 0.0f && gate_mm >= 0.0f);          // written so that a NaN fails
  FVP_LIMIT(L <= FVP_LIMB_MAX && J <= FVP_MAX_JOINTS && N <= kTrackDets && T <= kTrackSlots);
  LimbPrm prm = {};
  if (const int rc = limb_table(limbs, L, J, prm)) return rc;
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_limb_learn, dim3(ceil_div(T, kLimbThreads / L), nseq), dim3(kLimbThreads), 0, as_stream(s),
                     fused_poses, frame_set, ids, slots, joint_conf, prm, L, limb_len, limb_var, limb_cnt, limb_out, limb_id,
                     target, limb_obs, limb_state, B, N, J, nseq, T, conf_min, min_frames, window, gate_sigma, gate_mm,
                     relearn);
  return launch_status();
}

extern "C" int fvp_limb_fit(const float* poses, const int32_t* ids, const float* joint_conf, const float* target,
                            const int32_t* limbs, int L, float* fitted, float* resid, int B, int N, int J, float conf_min,
                            float stiffness, int iters, fvp_stream_t s) {
  FVP_REQUIRE(poses && target && limbs && fitted);
  FVP_REQUIRE(B >= 0 && N > 0 && J > 0 && L > 0 && iters >= 1 && iters <= 32);
  FVP_REQUIRE(stiffness >= 0.0f && stiffness <= 1.0f);          // written so that a NaN fails
  FVP_LIMIT(L <= FVP_LIMB_MAX && J <= FVP_MAX_JOINTS && N <= kTrackDets);
  LimbPrm prm = {};
  if (const int rc = limb_table(limbs, L, J, prm)) return rc;
  if (B == 0) return 0;
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_limb_fit, dim3(ceil_div(B * N, kLimbThreads)), dim3(kLimbThreads), 0, as_stream(s), poses, ids,
                     joint_conf, target, prm, L, fitted, resid, B * N, J, conf_min, stiffness, iters);
  return launch_status();
}

extern "C" int fvp_track_reid(const int32_t* ids, const int32_t* slots, const int32_t* sig, const int32_t* sig_count,
                              const int32_t* frame_set, int32_t* slot_sig, int32_t* slot_tid, int32_t* slot_pid,
                              int32_t* slot_frames, int32_t* slot_age, float* slot_sim, int32_t* gal_sig, int32_t* gal_pid,
                              int32_t* gal_age, int32_t* pids, int32_t* reid_state, float* reid_sim, int B, int N, int nseq,
                              int T, int G, int P, int max_age, int min_samples, int min_frames, int window, float sim_min,
                              float margin, int gallery_max_age, fvp_stream_t s) {
  FVP_REQUIRE(ids && slots && sig && sig_count && slot_sig && slot_tid && slot_pid && slot_frames && slot_age && slot_sim);
  FVP_REQUIRE(gal_sig && gal_pid && gal_age && pids && reid_state && reid_sim);
  FVP_REQUIRE(B >= 0 && N > 0 && nseq > 0 && G > 0 && P > 0 && T >= N);
  FVP_REQUIRE(max_age >= 0 && min_samples >= 0 && gallery_max_age >= 0 && min_frames >= 1 && window >= min_frames);
  FVP_REQUIRE(!std::isnan(sim_min) && !std::isnan(margin));
  FVP_LIMIT(N <= kTrackDets && T <= kTrackSlots && G <= kReidGallery && P <= FVP_SIG_MAX_PARTS);
  FVP_LIMIT(window <= FVP_REID_MAX_WINDOW);
  if (B == 0) return 0;
  const ReidPrm q = {max_age, min_samples, min_frames, window, gallery_max_age, sim_min, margin};
  ProfScope ps(FVP_K_OTHER, as_stream(s));
  hipLaunchKernelGGL(k_track_reid, dim3(nseq), dim3(kReidThreads), 0, as_stream(s), ids, slots, sig, sig_count, frame_set,
                     slot_sig, slot_tid, slot_pid, slot_frames, slot_age, slot_sim, gal_sig, gal_pid, gal_age, pids,
                     reid_state, reid_sim, B, N, nseq, T, G, P, q);
  return launch_status();
}
