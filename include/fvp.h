/*
 * fvp.h - C ABI of the MI355X-native Faster-VoxelPose inference hot path.
 *
 * One flat `extern "C"` entry point per operator group of the reference's hot path
 * (heatmaps -> project_layer -> HDN -> JLN -> 3D joints; AlvinYH/Faster-VoxelPose,
 * lib/models).  The reference has no FFI layer of its own (it is pure PyTorch); each
 * declaration below names the reference Python site (file:line under the reference
 * checkout) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch-ROCm storage);
 *     nothing is allocated, freed or retained by the library;
 *   - every call is asynchronous on the given `hipStream_t` (passed as void*; NULL = the
 *     null stream) and returns 0 or a hipError_t / FVP_E* code; no exceptions cross the ABI;
 *   - tensors are dense, row-major, fp32 unless stated; index tensors are int32 or int64
 *     as stated (int64 where the reference returns torch.int64);
 *   - thread-safe for calls on distinct streams with distinct output buffers.
 */
#ifndef FVP_H_
#define FVP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVP_ABI_VERSION 24
#define FVP_MAX_VIEWS 8
#define FVP_CAM_FLOATS 24 /* R[9] T[3] fx fy cx cy k[3] p[2] + 3 pad */
#define FVP_MAX_JOINTS 32
#define FVP_TRACK_MAX_DETS 32   /* fvp_track_update: person slots per frame (N)   */
#define FVP_TRACK_MAX_TRACKS 64 /* fvp_track_update: track slots per sequence (T) */
#define FVP_SIG_MAX_PARTS 4      /* fvp_person_signature, fvp_track_reid: body parts of a signature (P) */
#define FVP_SIG_BINS 64         /* fvp_person_signature, fvp_track_reid: colour bins per part, 2 bits per channel */
#define FVP_SIG_MAX_SAMPLES 16384 /* samples of one person in one frame: FVP_MAX_VIEWS * 64 limbs * 32 samples */
#define FVP_REID_MAX_GALLERY 64 /* fvp_track_reid: gallery entries per sequence (G) */
#define FVP_REID_MAX_WINDOW 1024 /* fvp_track_reid: frames a signature accumulates before it is halved (window) */
#define FVP_LIMB_MAX 64          /* fvp_limb_learn, fvp_limb_fit: limbs of the table (L) */
/* fvp_limb_learn: limb_state */
#define FVP_LIMB_LEARNED 1       /* the sample was accepted and the limb has min_frames samples: target is its length */
#define FVP_LIMB_LEARNING 2      /* the sample was accepted, fewer than min_frames so far: target is 0 */
#define FVP_LIMB_NOT_MEASURED 0  /* an end is unsupported, or the ends coincide / overflow: the statistics are unchanged */
#define FVP_LIMB_OUTLIER (-1)    /* the sample failed the gate: the statistics are unchanged, the outlier count grew */
#define FVP_LIMB_RELEARNED (-2)  /* more than `relearn` outliers in a row: the limb starts over from this sample */
#define FVP_LIMB_INVALID (-3)    /* an invalid slot, or a frame of no sequence */
#define FVP_VIS_MAX_PEOPLE 32  /* fvp_joint_visibility: person slots per frame (N) */
#define FVP_VIS_MAX_PRIMS 64    /* fvp_joint_visibility: body primitives per person (L) */
#define FVP_TRI_MAX_RADIUS 8    /* fvp_triangulate_joints: window half-size in heat-map cells */
/* fvp_triangulate_joints: view_state */
#define FVP_TRI_USED 1           /* the view is part of the joint's final solve */
#define FVP_TRI_NOT_EVALUATED 0  /* absent person, or a frame_set entry outside the camera table */
#define FVP_TRI_OUTSIDE (-1)     /* the joint is not finite, behind the camera, or its window holds no cell of the map */
#define FVP_TRI_PEAK_LOW (-2)    /* the window's maximum is below min_peak (or every candidate is a NaN) */
#define FVP_TRI_NOT_ENCLOSED (-3) /* the maximum lies on the window's border: the true peak may be outside */
#define FVP_TRI_OCCLUDED (-4)    /* a peak was taken, but occluder says the view does not see the joint */
#define FVP_TRI_REJECTED (-5)    /* dropped by the rejection round */
#define FVP_TRI_UNSOLVED (-6)    /* usable, but the joint was not triangulated: too few usable views, or degenerate */
#define FVP_CAL_ACC 32           /* fvp_camera_refit_*: doubles of accumulator state per camera */
/* fvp_camera_refit_solve: cal_state */
#define FVP_CAL_OK 1             /* the step was solved and applied */
#define FVP_CAL_CLAMPED 2        /* solved, and scaled down to the trust region before it was applied */
#define FVP_CAL_FEW 0            /* fewer than min_obs observations: the record is copied */
#define FVP_CAL_DEGENERATE (-1)  /* the normal matrix is not positive definite enough, or the step is not finite: copied */
/* fvp_anonymise_rois, fvp_anonymise_rois_nv12: shape and mode */
#define FVP_ANON_RECT 0          /* the box itself */
#define FVP_ANON_ELLIPSE 1       /* the ellipse inscribed in the box */
#define FVP_ANON_MOSAIC 0        /* covered pixels take the mean of their frame-anchored cell */
#define FVP_ANON_FILL 1          /* covered pixels take one colour */

#define FVP_EINVAL 10001 /* bad argument (null pointer, unsupported size) */
#define FVP_ELIMIT 10002 /* size beyond a compiled limit (see message) */

typedef void* fvp_stream_t;

/* Per-dataset projection constants (lib/models/project_whole.py:49-60). */
typedef struct FvpGeom {
  float clamp_max; /* max(ORI_IMAGE_SIZE) : pixel clamp [-1, clamp_max]          :51 */
  float rt[6];     /* resize_transform 2x3, row-major                             :52 */
  float hm_w, hm_h;   /* HEATMAP_SIZE as floats                                   :53 */
  float img_w, img_h; /* IMAGE_SIZE as floats                                     :55 */
  int32_t W, H;       /* heatmap width / height                                       */
  int32_t V, J;       /* views, joints                                                */
  int32_t JP;         /* joints padded to a multiple of 4 (channels-last staging)     */
} FvpGeom;

int fvp_version(void);
/* 0 for the shipped library, which reads NO environment variable; 1 for the diagnostics build (-DFVP_DIAG=1,
 * tests/diag/libfvp_hip_diag.so - test / tool infrastructure) in which the kernel-selection, tuning and ablation
 * switches of DESIGN.md section 6 (FVP_* environment variables) are honoured. */
int fvp_diag_build(void);
/* sizeof(FvpGeom) (what = 0) / sizeof(FvpConvOp) (what = 1) as compiled into the library: lets a
 * binding check its struct mirrors before passing them. */
int fvp_sizeof(int what);
const char* fvp_error_string(int code);

/* ---- staging ------------------------------------------------------------------------
 * NCHW heatmaps [B,V,J,H,W] -> channels-last [B,V,H,W,JP] (pad channels = 0), so the four
 * bilinear taps of one (voxel, view) read JP contiguous floats each.  No reference
 * counterpart (F.grid_sample reads NCHW); this is the MI355X layout decision. */
int fvp_heatmaps_to_cl(const float* heat, float* heat_cl, int B, const FvpGeom* g, fvp_stream_t s);

/* ---- a-1/a-2/a-13: sampling grid ------------------------------------------------------
 * grid[v][ix*ny*nz + iy*nz + iz] = normalised (x,y) of voxel centre (ax[ix], ay[iy], az[iz])
 * in view v.  Replaces ProjectLayer.project_grid (project_whole.py:49-60,
 * project_individual.py:60-72) + cameras.project_point (utils/cameras.py:30-56) +
 * transforms.affine_transform_pts_cuda (utils/transforms.py:59-63).  The projection kernels
 * below evaluate the same device function on the fly; this export exists for the
 * drop-in `sample_grid` cache and for parity tests.  cams = [V][FVP_CAM_FLOATS]. */
int fvp_sample_grid(const float* ax, const float* ay, const float* az, int nx, int ny, int nz,
                    const float* cams, const FvpGeom* g, float* grid, fvp_stream_t s);

/* ---- a-3 (+ the z-max of a-4): whole-space back-projection ------------------------------
 * cubes[b][j][x][y][z] = clamp01(mean_v bilinear(heat_cl[b][v], grid(v, voxel)))  and/or
 * zmax[b][j][x][y] = max_z cubes.  Either output may be NULL.  Replaces
 * project_whole.ProjectLayer.forward (project_whole.py:62-88) and torch.max(x, dim=4)
 * (cnns_2d.py:174).  cams = [nsets][V][FVP_CAM_FLOATS]; frame_set[b] picks the camera set
 * (one per sequence, meta['seq'][b]). */
int fvp_project_whole(const float* heat_cl, const float* cams, const int32_t* frame_set,
                      const float* ax, const float* ay, const float* az, int X, int Y, int Z, int B,
                      const FvpGeom* g, float* cubes, float* zmax, fvp_stream_t s);

/* ---- a-8 without materialised cubes: the N proposal z-columns of every frame ------------------------
 * feat1d[b*N + k][j][z] = cubes[b][j][flat[b][k]][z] WITHOUT the cubes: the same device function as
 * fvp_project_whole evaluated on the N columns that human_detection_net.py:92-93 gathers (bit-equal to
 * the gather from materialised cubes; tested).  flat [B][N] int64 from fvp_nms_topk; an index outside
 * [0, X*Y) yields a zero column.  Used by the fused forward (HumanDetectionNet inside
 * FasterVoxelPoseNet.forward), where nothing else of the 4*J*X*Y*Z bytes per frame is ever read. */
int fvp_project_columns(const float* heat_cl, const float* cams, const int32_t* frame_set, const float* ax,
                        const float* ay, const float* az, int X, int Y, int Z, int B, const FvpGeom* g,
                        const int64_t* flat, int N, float* feat1d, fvp_stream_t s);

/* ---- joint evidence (ABI 11): per-view reprojection and heatmap support of every fused joint ----------
 * For frame b, person slot n, joint j, view v, with (x,y,z) = fused_poses[b][n][j][0:3] (fused_poses = [B][N][J][5],
 * the output of fvp_fuse_poses, or any poses in that layout: a tracker's, ground truth):
 *   views[b][v][n][j] = (px, py, depth, s_v)                                        views = [B][V][N][J][4]
 *     (px, py)  the distorted pixel in the ORIGINAL camera image, cameras.project_point (utils/cameras.py:30-56),
 *               BEFORE the [-1, clamp_max] clamp of project_whole.py:51 (it may lie outside the image);
 *     depth     the camera-space z, xcam[2] of cameras.py:43, before the + 1e-5 of :44 (<= 0: behind the camera);
 *     s_v       the bilinear sample of channel j of heat_cl[b][v] at the sampling coordinate of that point
 *               (project_whole.py:49-60: clamp, resize transform, heatmap scale, clamp +-1.1), i.e. what
 *               F.grid_sample(align_corners=True, zero padding) of :83 returns for that channel; 0 when no tap is inside;
 *   joint_conf[b][n][j] = clamp01((s_0 + s_1 + ... + s_{V-1}) / V)                  joint_conf = [B][N][J]
 *     summed in view order, every operation rounded on its own: the value project_whole.py:83,86 would put into
 *     channel j of a voxel centred on the joint.
 * Same device functions as the projection kernels: s_v and joint_conf are bit-equal to what fvp_project_whole writes
 * for a voxel centre at that position.  A slot is valid when fused_poses[b][n][0][3] >= 0 (the flag fvp_fuse_poses
 * copies from proposal_centers[...][3]); every output element of an invalid slot is written as 0.  Every element of
 * both outputs is written.  Either output may be NULL (not both).  cams / frame_set / g as for fvp_project_whole. */
int fvp_joint_evidence(const float* heat_cl, const float* cams, const int32_t* frame_set,
                       const float* fused_poses, int B, int N, const FvpGeom* g,
                       float* views /* [B,V,N,J,4] */, float* joint_conf /* [B,N,J] */, fvp_stream_t s);

/* ---- pose tracker (ABI 12): one identity per person across the frames of a camera sequence -----------------------
 * No reference counterpart: the reference returns a bag of poses per frame, ordered by NMS rank.  This call gives every
 * valid slot of fused_poses [B][N][J][5] a track id that follows the person from frame to frame, on the device, in one
 * launch per batch and without host synchronisation.  Nearest-pose greedy association only: no motion prediction (the
 * poses are smoothed, and tracks coast through gaps, by fvp_track_smooth below, which consumes ids / slots; association
 * itself runs on the raw last pose), no re-identification after max_age, no optimal (Hungarian) assignment.
 * Re-identification of a person who comes back after max_age is fvp_track_reid below, which consumes ids / slots.
 * State per sequence s, in caller-owned DEVICE memory, read and rewritten by every call:
 *   trk_pose [nseq][T][J][3] fp32, trk_id [nseq][T] int32 (-1 = free slot), trk_age [nseq][T] int32, next_id [nseq] int32;
 *   the initial state is all ids -1, all ages 0, next_id 0 (the poses of free slots are never read).
 * frame_set [B] int32 (may be NULL = every frame belongs to sequence 0): the sequence of each frame, the table the
 * projection calls take.  Frames are consumed in batch order; the frames of one sequence are its time line; sequences are
 * independent.  For frame b of sequence s:
 *   1. detections D = slots n with fused_poses[b][n][0][3] >= 0; live tracks A = slots t with trk_id[s][t] >= 0;
 *   2. cost(n,t) = (d_0 + d_1 + ... + d_{J-1}) / J,  d_j = sqrt(dx*dx + dy*dy + dz*dz) between joint j of the detection
 *      and of the track (mm); fp32, every operation rounded on its own, sums left to right as written;
 *   3. a pair is eligible when cost <= gate_mm (a NaN cost never is); greedy: repeatedly the eligible pair of an
 *      unassigned detection and an unassigned track with the smallest (cost, n, t) in lexicographic order;
 *   4. matched (n,t): trk_pose[s][t] = the detection's xyz, trk_age[s][t] = 0;
 *      ids[b][n] = trk_id[s][t], slots[b][n] = t, costs[b][n] = cost(n,t);
 *   5. unmatched live track: trk_age += 1; if it is now > max_age, trk_id = -1 (the slot may be reused in this frame);
 *   6. unmatched detections in ascending n: the lowest free slot, or, when none is free, the live track with the largest
 *      age (lowest slot on a tie; T >= N, so its age is >= 1) is evicted; the slot gets trk_id = next_id[s]
 *      (then next_id[s] += 1), trk_age = 0 and the detection's xyz; ids[b][n] = the new id, slots[b][n] = the slot,
 *      costs[b][n] = -1;
 *   7. invalid slots: ids = slots = -1, costs = -1.
 * ids, slots [B][N] int32 and costs [B][N] fp32: every element is written by every call.  A frame whose frame_set entry
 * is outside [0, nseq) belongs to no sequence: its outputs are written as invalid and no state changes.
 * One workgroup of one wave per sequence walks the batch.  FVP_EINVAL: a null pointer (frame_set excepted), N, J or nseq
 * < 1, T < N, max_age < 0;  FVP_ELIMIT: N > FVP_TRACK_MAX_DETS, T > FVP_TRACK_MAX_TRACKS, J > FVP_MAX_JOINTS.  Nothing is
 * written when an error is returned.  B == 0 returns 0 without a launch. */
int fvp_track_update(const float* fused_poses, const int32_t* frame_set, float* trk_pose, int32_t* trk_id,
                     int32_t* trk_age, int32_t* next_id, int32_t* ids /* [B,N] */, int32_t* slots /* [B,N] */,
                     float* costs /* [B,N] */, int B, int N, int J, int nseq, int T, float gate_mm, int max_age,
                     fvp_stream_t s);

/* ---- track smoother (ABI 13): steady, slot-stable poses per track ---------------------------------------------------
 * fvp_track_smooth is a One-Euro filter (Casiez et al. 2012) per joint, in fp32.  Every operation is rounded on its own;
 * sums and products are evaluated exactly as written below; `/` and sqrtf are the correctly rounded forms.
 * State per sequence s, in caller-owned DEVICE memory, read and rewritten by every call:
 *   flt_pose [nseq][T][J][3] fp32, flt_vel [nseq][T][J][3] fp32 (mm/s), flt_id [nseq][T] int32 (-1 = free; initially all
 *   -1), flt_age [nseq][T] int32 (initially 0).
 * Inputs per call: fused_poses [B][N][J][5]; frame_set [B] (NULL = sequence 0); ids [B][N] and slots [B][N] as
 * fvp_track_update wrote them for the same batch; joint_conf [B][N][J] (fvp_joint_evidence) or NULL.
 * Parameters: rate_hz, min_cutoff, beta, d_cutoff, conf_min, damp (floats), max_age (int).
 * Constants, computed in the kernel: dt = 1.0f / rate_hz;  alpha(fc) = r / (r + 1.0f) with r = (6.2831855f * fc) / rate_hz;
 * a_d = alpha(d_cutoff).
 * Frames are consumed in batch order, sequences are independent.  A frame whose frame_set entry is outside [0, nseq)
 * changes no state, and its outputs are written as invalid.  For frame b of sequence s, every track slot t:
 *   1. n = the lowest detection slot with ids[b][n] >= 0 and slots[b][n] == t, if any (a slot with ids >= 0 whose slots
 *      entry is outside [0, T) is treated like one with ids < 0 everywhere below);
 *   2. n exists and flt_id[s][t] != ids[b][n] - a birth, a reuse, an eviction: the slot is (re)initialised.  For every j:
 *      x^ = fused_poses[b][n][j][0:3], v^ = 0, flag = 1;  flt_id = ids[b][n], flt_age = 0;
 *   3. n exists and the id is the same: flt_age = 0 and every joint j on its own, with x = fused_poses[b][n][j][0:3]:
 *        e_c = x_c - x^_c for c = 0,1,2;
 *        the joint is MEASURED when (joint_conf is NULL or joint_conf[b][n][j] >= conf_min) and fabsf(e_c) <= FLT_MAX
 *        for all three c (a NaN or Inf never counts as measured):
 *          v_c = e_c * rate_hz;  v^_c = v^_c + a_d * (v_c - v^_c);
 *          sp = sqrtf((v^_0*v^_0 + v^_1*v^_1) + v^_2*v^_2);  a = alpha(min_cutoff + beta * sp);
 *          x^_c = x^_c + a * e_c;  flag = 1;
 *        otherwise it is PREDICTED:  v^_c = v^_c * damp;  x^_c = x^_c + v^_c * dt;  flag = 0;
 *   4. no n and flt_id[s][t] >= 0: flt_age += 1; if it is now > max_age, flt_id = -1, flt_age = 0 and the slot is free
 *      (its x^, v^ stay as they are and are never read); otherwise every joint takes the PREDICTED update of 3 (coasting);
 *   5. outputs - each may be NULL, not all of them; every element of a non-NULL output is written by every call:
 *        smooth [B][N][J][5]: for a valid slot, columns 0:3 are the x^ of its track slot after this frame and columns 3:5
 *          are copied from fused_poses; an invalid slot (ids < 0) is copied from fused_poses unchanged (the layout
 *          core/metrics.py, utils/vis.py and fvp_joint_evidence take);
 *        track_poses [B][T][J][4]: (x^_0, x^_1, x^_2, flag) after this frame - person-stable: a person keeps its row t
 *          for the life of the track, coasting frames included; a free slot is four zeros;
 *        track_state [B][T][2] int32: (flt_id, flt_age) after this frame; a free slot is (-1, 0).
 * Consequence (tested): with the tracker's own max_age, flt_id == trk_id after every call, and flt_age == trk_age in every
 * live slot (the tracker leaves max_age + 1 in a slot it has freed; here a freed slot's age is 0).
 * The tracker still associates against the raw last pose: predictions are not fed back into association.
 * One thread per (s, t, j) walks the batch; one launch per batch.  FVP_EINVAL: a null required pointer (frame_set and
 * joint_conf excepted; all three outputs null), N, J or nseq < 1, T < N, max_age < 0, rate_hz, min_cutoff or d_cutoff not
 * > 0, beta not >= 0, damp outside [0, 1] (a NaN fails every one of these comparisons);  FVP_ELIMIT as for
 * fvp_track_update.  Nothing is written when an error is returned.  B == 0 returns 0 without a launch. */
int fvp_track_smooth(const float* fused_poses, const int32_t* frame_set, const int32_t* ids, const int32_t* slots,
                     const float* joint_conf, float* flt_pose, float* flt_vel, int32_t* flt_id, int32_t* flt_age,
                     float* smooth /* [B,N,J,5] */, float* track_poses /* [B,T,J,4] */,
                     int32_t* track_state /* [B,T,2] */, int B, int N, int J, int nseq, int T, float rate_hz,
                     float min_cutoff, float beta, float d_cutoff, float conf_min, float damp, int max_age,
                     fvp_stream_t s);

/* ---- limb model (ABI 22): bone lengths per person, and poses constrained to them -----------------------------------------
 * The tracker, the smoother and re-ID treat every joint on its own; a person is a rigid linkage.  fvp_limb_learn keeps a
 * running, gated estimate of every limb's length per track (from the frames in which both ends are supported);
 * fvp_limb_fit moves a pose, as little as a few Gauss-Seidel sweeps allow, onto those lengths: with both ends supported each
 * takes half of a limb's correction, an unsupported end takes all of it.  Both are fp32 with every operation rounded on
 * its own; sums and products are evaluated exactly as written below; `/` and sqrtf are the correctly rounded forms.
 * limbs is a HOST array [L][2] of joint index pairs (i, k), copied into the launch; any list works (COCO-17 has cycles),
 * no tree is required.
 * SUPPORTED: joint j of slot (b, n) is supported when (joint_conf is NULL or joint_conf[b][n][j] >= conf_min) and
 * fabsf(x_c) <= FLT_MAX for its three coordinates (a NaN or Inf never is).
 * dist(i, k): delta_c = x_k,c - x_i,c;  d = sqrtf((delta_0*delta_0 + delta_1*delta_1) + delta_2*delta_2);  d is VALID when
 * d > 0 && d <= FLT_MAX.
 *
 * fvp_limb_learn.  State per sequence s, in caller-owned DEVICE memory, read and rewritten by every call:
 *   limb_len, limb_var [nseq][T][L] fp32 (mm, mm^2), limb_cnt, limb_out [nseq][T][L] int32 (accepted samples, capped at
 *   window; outliers in a row), all initially 0;  limb_id [nseq][T] int32, initially -1.
 * Inputs per call: fused_poses [B][N][J][5]; frame_set [B] (NULL = sequence 0); ids [B][N] and slots [B][N] as
 * fvp_track_update wrote them for the same batch; joint_conf [B][N][J] or NULL.
 * Frames are consumed in batch order, sequences are independent.  A frame whose frame_set entry is outside [0, nseq)
 * changes no state, and its outputs are written as invalid.  For frame b of sequence s, every track slot t:
 *   1. n = the lowest detection slot with ids[b][n] >= 0 and slots[b][n] == t (a slot with ids >= 0 whose slots entry is
 *      outside [0, T) is treated like one with ids < 0 everywhere below).  No n: the slot's state is untouched - the
 *      lengths survive coasting and the tracker's freeing of the slot; only a new id resets them;
 *   2. n exists and limb_id[s][t] != ids[b][n]: limb_id = ids[b][n], and len = var = 0, cnt = out = 0 for every limb;
 *      step 3 follows in the same frame;
 *   3. every limb l = (i, k) on its own, from fused_poses[b][n]:
 *        either end unsupported, or d = dist(i, k) not VALID: NOT_MEASURED, limb_obs = (-1, 0), statistics unchanged;
 *        else e = d - len, and the gate: when cnt >= min_frames, tol = fmaxf(gate_sigma * sqrtf(var), gate_mm) and the
 *        sample passes when fabsf(e) <= tol; when cnt < min_frames it passes;
 *        failed: out += 1; if out > relearn the limb starts over from this sample - len = d, var = 0, cnt = 1, out = 0,
 *          RELEARNED - otherwise OUTLIER and len, var, cnt are unchanged;
 *        passed: out = 0; c = min(cnt + 1, window); cnt = c; g = 1.0f / (float)c; len = len + g * e;
 *          var = var + g * (e * (d - len) - var) with the NEW len (Welford up to window, exponential forgetting after it;
 *          the first sample gives len = d, var = 0 without a special case); LEARNED when c >= min_frames, else LEARNING;
 *        measured limbs write limb_obs = (d, e);
 *        target[b][n][l] = len after this frame when cnt (after this frame) >= min_frames, else 0 - whatever the state;
 *   4. an invalid slot (ids < 0) gets target = 0, limb_obs = (-1, 0), limb_state = INVALID.  (A further detection in the
 *      same track slot, which fvp_track_update never writes, gets the values of the lowest one.)
 * Outputs, every element written by every call: target [B][N][L] fp32, limb_obs [B][N][L][2] fp32 (d, e), limb_state
 * [B][N][L] int32 (FVP_LIMB_*).  One thread per (s, t, l) walks the batch; one launch per batch.
 *
 * fvp_limb_fit is stateless, per slot (b, n).  The slot is valid when poses[b][n][0][3] >= 0 and (ids is NULL or
 * ids[b][n] >= 0); an invalid slot is copied unchanged and its resid is 0.  Otherwise y = the xyz of poses[b][n], m_j =
 * SUPPORTED decided once from the input pose, and for it = 0..iters-1, for l = 0..L-1 in table order, with l = (i, k):
 *   t = target[b][n][l]; skip unless t > 0 (a NaN skips);  delta = y_k - y_i, d = dist;  skip unless d is VALID (a
 *   non-finite joint constrains nothing and poisons nothing);
 *   s = (stiffness * (d - t)) / d;  (w_i, w_k) = (0.5f, 0.5f) when m_i == m_k, (0, 1) when only i is supported, (1, 0)
 *   when only k is;  y_i,c = y_i,c + (w_i * s) * delta_c;  y_k,c = y_k,c - (w_k * s) * delta_c.
 * fitted [B][N][J][5]: y in columns 0:3, columns 3:5 copied (fitted may be poses itself);  resid [B][N][L] or NULL: d - t
 * recomputed after the last sweep for the limbs with t > 0 and a VALID d, else 0.  poses may be any poses of the layout
 * (fvp_track_smooth's smooth).  One lane per slot; one launch.
 *
 * Not built: carrying a person's lengths across re-identification, lengths as a re-ID or association cue, joint-angle
 * limits, left/right symmetry, a fit coupled into the One-Euro state.
 * FVP_EINVAL: a null required pointer (frame_set, joint_conf, fvp_limb_fit's ids and resid excepted); N, J, L or nseq < 1;
 * T < N; a limb index outside [0, J) or i == k; min_frames < 1; window < min_frames; relearn < 0; gate_sigma or gate_mm not
 * >= 0; stiffness outside [0, 1]; iters outside [1, 32] (a NaN fails every one of these comparisons).  FVP_ELIMIT: L >
 * FVP_LIMB_MAX, J > FVP_MAX_JOINTS, N > FVP_TRACK_MAX_DETS, T > FVP_TRACK_MAX_TRACKS.  Nothing is written when an error is
 * returned.  B == 0 returns 0 without a launch. */
int fvp_limb_learn(const float* fused_poses /* [B][N][J][5] */, const int32_t* frame_set /* [B] or NULL */,
                   const int32_t* ids, const int32_t* slots /* [B][N], fvp_track_update's */,
                   const float* joint_conf /* [B][N][J] or NULL */, const int32_t* limbs /* HOST [L][2] */, int L,
                   float* limb_len, float* limb_var, int32_t* limb_cnt, int32_t* limb_out /* state [nseq][T][L] */,
                   int32_t* limb_id /* state [nseq][T], initially -1; the others 0 */,
                   float* target /* [B][N][L] */, float* limb_obs /* [B][N][L][2] */, int32_t* limb_state /* [B][N][L] */,
                   int B, int N, int J, int nseq, int T, float conf_min, int min_frames, int window,
                   float gate_sigma, float gate_mm, int relearn, fvp_stream_t s);
int fvp_limb_fit(const float* poses /* [B][N][J][5] */, const int32_t* ids /* [B][N] or NULL */,
                 const float* joint_conf /* [B][N][J] or NULL */, const float* target /* [B][N][L] */,
                 const int32_t* limbs /* HOST [L][2] */, int L, float* fitted /* [B][N][J][5] */,
                 float* resid /* [B][N][L] or NULL */, int B, int N, int J, float conf_min, float stiffness, int iters,
                 fvp_stream_t s);

/* ---- person re-identification (ABI 20): old identities back after a gap -------------------------------------------------
 * fvp_track_update forgets a track after max_age frames: a person who leaves the capture volume, stays hidden for longer, or
 * re-appears further than gate_mm from where they vanished comes back under a new track id.  The two calls below give every
 * track a PERSON id that survives such gaps: fvp_person_signature reads a colour signature of every person from the camera
 * frames, fvp_track_reid keeps the signatures of retired tracks in a gallery per sequence and hands an old person id to a new
 * track that looks the same.  A person id is the track id of the first track that person ever had: there is no second
 * counter.  One launch each, on the device, no host synchronisation.  Everything below is integer arithmetic except where
 * fp32 / fp64 is named, so no result depends on the order of accumulation or on scheduling.
 *
 * fvp_person_signature.  frames [B*V][Hs][Ws][3] uint8: the contiguous HWC layout of fvp_ingest_frames; the three bytes of a
 * pixel are taken in memory order (c0, c1, c2), there is no channel flag.  views [B][V][N][J][4], ids [B][N] or NULL, joint_conf
 * [B][N][J] or NULL and conf_min are those of fvp_draw_poses; occluder [B][V][N][J] int32 of fvp_joint_visibility, or NULL.
 * Body model, HOST memory, passed to the kernel by value: limbs [L][2] int32 joint index pairs, limb_part [L] int32 with values in
 * [0, P): the body part (for example 0 = upper body, 1 = legs) a limb's samples are counted in; K samples per limb.
 * Usable joint-view (b,v,n,j): the joint is drawable by fvp_draw_poses' rule - depth > 0, |px| <= 32768 and |py| <= 32768 (fp32
 *   compares: a NaN or an Inf fails them), joint_conf NULL or joint_conf[b][n][j] >= conf_min (a NaN confidence is not usable) -
 *   and occluder is NULL or occluder[b][v][n][j] == -1.
 * Selected person: ids is NULL or ids[b][n] >= 0.
 * Samples of a selected person (b,n): for every view v, every limb l = (i,k) whose two joints are usable in view v, and m = 0 ..
 *   K-1, in fp32, every operation rounded on its own (no contraction), IEEE division:
 *     t = (float(m) + 0.5f) / float(K)
 *     x = px_i + t * (px_k - px_i)            y = py_i + t * (py_k - py_i)
 *     xi = (int)rintf(x)                      yi = (int)rintf(y)               round-half-even
 *   The sample COUNTS iff 0 <= xi < Ws and 0 <= yi < Hs.  Its bin is (c0 >> 6) * 16 + (c1 >> 6) * 4 + (c2 >> 6) of the three
 *   bytes of pixel (xi, yi) of frame b*V + v.  No byte of a sample that does not count is read, and no byte outside the frames.
 *   A limb whose two ends coincide puts its K samples on one pixel; they count K times.
 * Outputs, every element of a non-NULL output written by every call; either may be NULL, not both:
 *     sig       [B][N][P][FVP_SIG_BINS] int32: the number of counting samples of part limb_part[l] with that bin, over all views
 *                                              and limbs;
 *     sig_count [B][N][P]               int32: their sum over the bins (<= FVP_SIG_MAX_SAMPLES over the parts of one person).
 *   A person that is not selected writes zeros, and so does an invalid slot: fvp_joint_evidence writes its depth as 0.
 * FVP_EINVAL: null frames, views, limbs or limb_part; both outputs null; B or V < 0; N, J, Hs, Ws, L or P < 1; K outside [1, 32];
 * a limb index outside [0, J); a part outside [0, P); NaN conf_min.  FVP_ELIMIT: N > 32, J > FVP_MAX_JOINTS, V > FVP_MAX_VIEWS,
 * L > 64, P > FVP_SIG_MAX_PARTS, Hs or Ws > 16384.  Nothing is written when an error is returned.  B * V == 0 returns 0 without a
 * launch.  One workgroup per (b, n): the V * L * K samples are strided over its threads, the histogram is built in LDS with
 * integer atomics and written out coalesced.  Not built: NV12 surfaces, pitched frames, a channel-order flag, learned embeddings. */
int fvp_person_signature(const uint8_t* frames /* [B*V][Hs][Ws][3] */, int B, int V, int Hs, int Ws,
                         const float* views /* [B][V][N][J][4] of fvp_joint_evidence */,
                         const int32_t* ids /* [B][N] or NULL */, const float* joint_conf /* [B][N][J] or NULL */,
                         const int32_t* occluder /* [B][V][N][J] of fvp_joint_visibility, or NULL */, int N, int J,
                         const int32_t* limbs /* HOST [L][2] */, const int32_t* limb_part /* HOST [L] */, int L, int P, int K,
                         float conf_min, int32_t* sig /* [B][N][P][FVP_SIG_BINS] */, int32_t* sig_count /* [B][N][P] */,
                         fvp_stream_t s);

/* fvp_track_reid.  State per sequence s, in caller-owned DEVICE memory, read and rewritten by every call:
 *   slot_sig [nseq][T][P][FVP_SIG_BINS] int32: the signature a track has accumulated;
 *   slot_tid [nseq][T] int32: the track id the slot's accumulation belongs to, -1 = free;
 *   slot_pid [nseq][T] int32: the decided person id, -1 = pending;
 *   slot_frames [nseq][T] int32: frames accumulated;   slot_age [nseq][T] int32: frames since the track was last seen;
 *   slot_sim [nseq][T] fp32: sim(best) of the slot's decision, -1 before it and when the gallery was empty;
 *   gal_sig [nseq][G][P][FVP_SIG_BINS] int32, gal_pid [nseq][G] int32 (-1 = free), gal_age [nseq][G] int32: the gallery.
 *   The initial state is all ids -1, slot_sim -1 and everything else 0.  A free slot and a free gallery entry are always in that
 *   state: whatever frees one CLEARS it (ids -1, slot_sim -1, every other value and every counter 0).
 * Inputs per call: ids [B][N] and slots [B][N] as fvp_track_update wrote them for the same batch; sig [B][N][P][FVP_SIG_BINS] and
 * sig_count [B][N][P] as fvp_person_signature wrote them (counters >= 0, at most FVP_SIG_MAX_SAMPLES per person and frame: with
 * other values the integer arithmetic below wraps); frame_set [B] (NULL = sequence 0).
 * Parameters: max_age (the tracker's own), min_samples, min_frames >= 1, window >= min_frames, sim_min, margin (fp32),
 * gallery_max_age (0 = never forget).  With window <= FVP_REID_MAX_WINDOW no counter passes (window + 1) * FVP_SIG_MAX_SAMPLES
 * < 2^25, far below 2^30, and every product below is < 2^50: exact in int64 and in fp64.
 * Frames are consumed in batch order, sequences are independent.  A frame whose frame_set entry is outside [0, nseq) changes
 * no state and its outputs are written as invalid.  For frame b of sequence s, in this order:
 *   1. Gallery ageing: every occupied entry (gal_pid >= 0) gets gal_age += 1; with gallery_max_age > 0 an entry whose age is now
 *      > gallery_max_age is freed.
 *   2. Every track slot t in ascending t.  n = the lowest detection slot with ids[b][n] >= 0 and slots[b][n] == t, if any
 *      (fvp_track_smooth's rule: a detection whose slots entry is outside [0, T) is treated like one with ids < 0 everywhere).
 *      a. RETIRE iff slot_tid[t] >= 0 and either (n exists and ids[b][n] != slot_tid[t]) or (no n and slot_age[t] + 1 > max_age).
 *         If slot_frames[t] >= min_frames, the pair (slot_pid[t] if it is >= 0, else slot_tid[t]; slot_sig[t]) is stored with
 *         gal_age = 0 in the lowest free gallery entry or, when none is free, in the entry with the largest gal_age (lowest
 *         index on a tie), whose former content is lost.  A track with fewer frames is forgotten.  The slot is then cleared.
 *      b. COAST iff no n and slot_tid[t] >= 0 (still live): slot_age += 1.
 *      c. BIRTH iff n exists and slot_tid[t] != ids[b][n]: slot_tid = ids[b][n]; the rest of the slot is in the cleared state.
 *      d. ACCUMULATE iff n exists: slot_age = 0; and if sig_count[b][n][0] + ... + sig_count[b][n][P-1] >= min_samples (int32):
 *         if slot_frames == window, every counter of slot_sig[t] is first halved (>> 1) and slot_frames = window >> 1 (this bounds
 *         the counters and lets a signature follow slow lighting changes); then slot_sig[t] += sig[b][n], slot_frames += 1.
 *      e. DECIDE iff slot_tid[t] >= 0, slot_pid[t] == -1 and slot_frames[t] >= min_frames.  For every occupied gallery entry g:
 *           for every part p: Ca, Cg = the sum of the slot's, the entry's counters of part p over the bins; the part COUNTS iff
 *           Ca > 0 and Cg > 0; inter_p = the sum over the bins of min(a_bin * Cg, g_bin * Ca), in int64 (exact);
 *           sim(g) = float((q_0 + q_1 + ...) / double(parts that count)), q_p = double(inter_p) / (double(Ca) * double(Cg)) over
 *           the parts that count in ascending p, in fp64, every operation rounded on its own, one rounding to fp32 at the end;
 *           sim(g) = 0.0f when no part counts.  It is the histogram intersection of the two normalised signatures, in [0, 1].
 *         best = the occupied entry with the largest sim (lowest g on a tie); second = the largest sim among the other occupied
 *         entries, 0.0f when there is none.  ADOPT iff a best exists and sim(best) >= sim_min and sim(best) - second >= margin
 *         (fp32 subtraction and compares: a NaN fails): slot_pid = gal_pid[best] and the entry is freed.  Otherwise slot_pid =
 *         slot_tid: a new person.  slot_sim = sim(best), or -1.0f when the gallery was empty.
 *         Slots decide in ascending t, so two pending tracks cannot adopt the same entry: the lower slot takes it.
 *   3. Outputs, every element written by every call.  Detection n is VALID iff ids[b][n] >= 0 and t = slots[b][n] is in [0, T):
 *        pids [B][N] int32:       slot_pid[t], or slot_tid[t] while the slot is pending;
 *        reid_state [B][N] int32: 0 pending, 1 a new person (slot_pid == slot_tid), 2 re-identified (slot_pid != slot_tid);
 *        reid_sim [B][N] fp32:    slot_sim[t];
 *      all after step 2 of this frame.  An invalid detection writes -1, -1, -1.0f.
 * Consequences (tested): with the tracker's own max_age, slot_tid == trk_id in every live slot after every call; a person id is
 * held by at most one live slot or gallery entry of a sequence at any time; splitting a batch into chunks changes nothing.
 * The defaults the host class suggests (min_samples, min_frames, window, sim_min, margin) are guesses: nothing was tuned on
 * real footage.  pids are not fed back into the tracker's association.
 * FVP_EINVAL: a null pointer (frame_set excepted); B < 0; N, nseq, G or P < 1; T < N; max_age, min_samples or gallery_max_age
 * < 0; min_frames < 1; window < min_frames; NaN sim_min or margin.  FVP_ELIMIT: N > FVP_TRACK_MAX_DETS, T >
 * FVP_TRACK_MAX_TRACKS, G > FVP_REID_MAX_GALLERY, P > FVP_SIG_MAX_PARTS, window > FVP_REID_MAX_WINDOW.  Nothing is written when
 * an error is returned.  B == 0 returns 0 without a launch.  One workgroup per sequence walks the batch: thread (p, bin) owns that
 * counter of every slot and gallery entry, a wave sums a part.  Not built: re-identification across sequences, learned
 * embeddings, NV12 surfaces, merging a returning track's gallery signature into its new accumulation. */
int fvp_track_reid(const int32_t* ids /* [B][N] */, const int32_t* slots /* [B][N] */,
                   const int32_t* sig /* [B][N][P][FVP_SIG_BINS] */, const int32_t* sig_count /* [B][N][P] */,
                   const int32_t* frame_set /* [B] or NULL */, int32_t* slot_sig, int32_t* slot_tid, int32_t* slot_pid,
                   int32_t* slot_frames, int32_t* slot_age, float* slot_sim, int32_t* gal_sig, int32_t* gal_pid,
                   int32_t* gal_age, int32_t* pids /* [B][N] */, int32_t* reid_state /* [B][N] */,
                   float* reid_sim /* [B][N] */, int B, int N, int nseq, int T, int G, int P, int max_age, int min_samples,
                   int min_frames, int window, float sim_min, float margin, int gallery_max_age, fvp_stream_t s);

/* z-max of already materialised cubes [n][Z] -> [n] (n = B*J*X*Y): the first statement of
 * CenterNet.forward (cnns_2d.py:174) when it is called on its own. */
int fvp_zmax(const float* cubes, float* zmax, long n, int Z, fvp_stream_t s);

/* ---- a-14 integer part: per-person fine-grid windows ------------------------------------
 * For each of n proposals ([n][7] rows of proposal_centers): tl = round_half_even(c*scale+bias)
 * (int32), offset (mm), margin from the bbox, start/end clipped to the fine grid.  boxes =
 * [n][9] int32 = tl[3], start[3], end[3]; offset = [n][3].  Bit-exact with
 * project_individual.ProjectLayer.forward :110-121.  consts = scale[3], bias[3], whole[3],
 * ind[3] (12 floats, device memory: host-side values of project_individual.py:22-30 uploaded once);
 * fine_cube = fine[3], cube[3]: six int32 in HOST memory, read at call time and passed to the
 * kernel by value (the only host-memory pointer argument of this ABI besides FvpGeom / op lists). */
int fvp_person_boxes(const float* centers, int n, const float* consts, const int32_t* fine_cube,
                     int32_t* boxes, float* offset, fvp_stream_t s);

/* The rows of each person's three orthographic planes that the individual projection can write (ABI 21).  The cube is
 * masked by the box (project_individual.py:113-121): outside [start, end) every voxel stays zero, so in the x-y and x-z
 * planes (rows = x) the rows outside [start0 - tl0, end0 - tl0) and in the y-z plane (rows = y) the rows outside
 * [start1 - tl1, end1 - tl1) are +0.0 in every channel.  boxes = [nP][9] of fvp_person_boxes; live_rows = [nP*3][2]
 * int32 = {r0, r1} per plane, clamped to [0, C]; an empty window in any axis gives {0, 0} for all three planes.
 * The array is what fvp_conv_stack_run_rows takes for P2PNet's input.  One launch, no host synchronisation. */
int fvp_plane_live_rows(const int32_t* boxes, int nP, int C, int32_t* live_rows, fvp_stream_t s);

/* ---- a-14 sampling part (drop-in, materialises the cube) ---------------------------------
 * cubes[p][j][C][C][C]; person p lives in frame person_frame[p]; fine-grid axis tables
 * fx/fy/fz of lengths fine[0..2].  Windows outside [start,end) stay 0; persons with
 * person_valid[p]==0 (may be NULL = all valid) are zero-filled.  Replaces
 * project_individual.ProjectLayer.forward :124-134. */
int fvp_project_individual(const float* heat_cl, const float* cams, const int32_t* frame_set,
                           const int32_t* person_frame, const uint8_t* person_valid, const int32_t* boxes,
                           const float* fx, const float* fy, const float* fz, const int32_t* fine, int C,
                           int nP, const FvpGeom* g, float* cubes, fvp_stream_t s);

/* ---- a-15 (drop-in on a materialised cube): orthographic max projections -------------------
 * planes[p][0]=max_z -> [J][x][y], [p][1]=max_y -> [J][x][z], [p][2]=max_x -> [J][y][z];
 * planes = [nP][3][J][C][C].  Replaces joint_localization_net.py:80-81. */
int fvp_triplane_max(const float* cubes, float* planes, int nP, int J, int C, fvp_stream_t s);

/* ---- a-14 + a-15 fused (fast path): never materialises the cube ----------------------------
 * Same result as fvp_project_individual followed by fvp_triplane_max, bit for bit
 * (max is order-independent).  planes must be zero-filled by the caller beforehand
 * (hipMemsetAsync); cross-workgroup maxima use integer atomicMax on the non-negative floats.
 * persons_per_frame > 0 promises person_frame[p] == p / persons_per_frame (placement hint: the
 * workgroups of one frame are numbered onto one XCD); pass 0 if unknown.
 * A workgroup owns a compact 4 x 4 x 16 voxel block; its taps are 16-byte global loads served by the CU's L1 (no LDS
 * staging of the heatmap: DESIGN.md 4.1), LDS holds the block's plane maxima only.
 * fine_grid (may be NULL): the per-sequence cache of sampling coordinates the reference keeps
 * (project_individual.py:82-94), [nsets][V][fine0*fine1*fine2][2] as written by fvp_sample_grid on the fine
 * axes; when given, `fine` must point to the three fine-grid sizes in HOST memory and the kernel loads the
 * 8-byte coordinate of a (voxel, view) instead of recomputing the projection (same bits either way). */
int fvp_project_individual_triplane(const float* heat_cl, const float* cams, const int32_t* frame_set,
                                    const int32_t* person_frame, const uint8_t* person_valid,
                                    const int32_t* boxes, const float* fx, const float* fy, const float* fz,
                                    const int32_t* fine, int C, int nP, const FvpGeom* g, float* planes,
                                    int persons_per_frame, const float* fine_grid, fvp_stream_t s);

/* ---- a-4/a-5/a-9/a-16: conv stacks ----------------------------------------------------------
 * A stack is a list of FvpConvOp over numbered activation buffers (all NCHW fp32,
 * [planes][C][H][W]; 1-D nets use H = 1).  The same interpreter runs CenterNet
 * (cnns_2d.py:147-178), C2CNet (cnns_1d.py:112-132) and P2PNet (cnns_2d.py:115-135).
 * Convs run on the fp32 matrix cores, the kernel chosen from the layer SHAPE alone (never the batch): 3x3 layers on
 * power-of-two maps and on rows of >= 40 columns (masked tiles: CenterNet's 80- / 40-wide levels, ABI 8) as Winograd
 * F(2x2,3x3) on v_mfma_f32_16x16x4_f32 (k_conv_wino), P2PNet's 7x7 front conv on
 * 16x16x4 tiles (k_conv7), 1x1 / transposed convs register-direct (k_conv_reg), everything else as implicit GEMMs on
 * v_mfma_f32_32x32x2_f32 (k_conv_dma); the whole 1-D stack in one kernel (fvp_conv_stack_run_fused_1d).
 * BatchNorm (eval) is applied in the epilogue as  y = (acc + bias) * bn_scale + bn_shift  (no weight folding, to stay
 * close to the reference's rounding), followed by the optional residual add / ReLU. */
enum {
  FVP_OP_CONV = 0,     /* stride-1 'same' conv, KH x KW                                     */
  FVP_OP_POOL2 = 1,    /* max_pool(2,2) (2-D) or max_pool1d(2) when H == 1                  */
  FVP_OP_CONVT2 = 2    /* ConvTranspose(k2,s2) as 4 (2-D) / 2 (1-D) interleaved 1x1 GEMMs   */
};
enum {
  FVP_EPI_RELU = 1,          /* ReLU after BN (and after the residual unless RES_AFTER)     */
  FVP_EPI_RES = 2,           /* add buffer `res`                                            */
  FVP_EPI_RES_AFTER_RELU = 4 /* upsample blocks: relu(bn(x)) + skip  (cnns_2d.py:106,110)   */
};
typedef struct FvpConvOp {
  int32_t kind;
  int32_t src, dst, res;      /* activation buffer ids; res = -1 if unused                  */
  int32_t cin, cout;          /* true channel counts                                        */
  int32_t kh, kw;
  int32_t h, w;               /* INPUT spatial size                                         */
  int32_t flags;              /* FVP_EPI_*                                                  */
  int32_t w_off;              /* float offset of packed weights in `params`                 */
  int32_t e_off;              /* float offset of epilogue vectors bias|scale|shift, 3*coutp */
  int32_t cinp, coutp;        /* padded counts used by the packed layout                    */
  int32_t wino_off;           /* 0, or float offset of the Winograd-domain copy of a 3x3    */
                              /* conv's weights ([cinp][coutp][16]); when set the conv runs  */
                              /* as F(2x2,3x3) (requires even H, W a power of two)           */
  int32_t pair_off;           /* 0, or float offset of the pixel-pair copy of the weights:    */
                              /* 7x7 conv with cout <= 16 -> [cinp][7][8][32], followed by the */
                              /* k-grouped copy [max(4,ceil(cin/4))][13][4][16][4] (ABI 7,     */
                              /* fvp_conv7.h); 2-D ConvTranspose(k2,s2) ->                     */
                              /* [dy][cinp][dx*coutp+co] (fvp_conv.hip)                        */
} FvpConvOp;

/* bufs[i] = device pointer of activation buffer i (caller sized: planes*C*H*W floats).
 * plane_valid (may be NULL): planes with plane_valid[n / valid_div] == 0 are skipped. */
int fvp_conv_stack_run(const FvpConvOp* ops, int nops, const float* params, float* const* bufs, int nbufs,
                       int planes, const uint8_t* plane_valid, int valid_div, fvp_stream_t s);

/* fvp_conv_stack_run with a promise about the stack's input (ABI 21; P2PNet on the masked tri-planes,
 * joint_localization_net.py:75-80 on the cubes of project_individual.py:113-121).  live_rows (device memory, may be
 * NULL: then this IS fvp_conv_stack_run) = [planes][2] int32 = {r0, r1}: the caller promises that in plane p of
 * bufs[ops[0].src] every channel of every row outside [r0, r1) is +0.0.  The range is clamped to [0, H]; r0 >= r1 says
 * the whole plane is zero.  The 7x7 front conv (k_conv7) then multiplies no row of zeros and fetches none; every other
 * kernel, and every op but ops[0], ignores the array.  The result has the same bits as without the array.  A promise
 * that does not hold gives a wrong result (the rows are treated as zero), never an out-of-bounds access.
 * fvp_conv_stack_reads_live_rows (host only, no launch): 1 if some kernel of the stack would read the array at this plane
 * count - ops[0] takes k_conv7 (7x7, cout <= 16, maps 64 or 128 wide, cin <= 20) -, else 0: a caller need not compute an
 * array that nothing reads (a miniature cube, CenterNet's stack). */
int fvp_conv_stack_reads_live_rows(const FvpConvOp* ops, int nops, int planes);
int fvp_conv_stack_run_rows(const FvpConvOp* ops, int nops, const float* params, float* const* bufs, int nbufs,
                            int planes, const uint8_t* plane_valid, int valid_div, const int32_t* live_rows,
                            fvp_stream_t s);

/* The same interpreter for a 1-D stack (H = 1, W <= 24, cout <= 128: C2CNet) fused into ONE
 * kernel, one workgroup per plane, activations resident in LDS.  in = [planes][cin][W] (buffer
 * ops[0].src), out = [planes][cout][W'] of the last op.  Deterministic; equal to fvp_conv_stack_run
 * up to rounding (each op's reduction is split into four K slices added in a fixed order).
 * The last op must be a conv or a transposed conv (its epilogue is what stores to `out`; its
 * residual, if any, is kept like any other op's): a stack that ends in a max-pool is refused with
 * FVP_EINVAL, and so is a pool of an odd length, exactly as fvp_conv_stack_run refuses it.
 * FVP_ELIMIT: nops > 32, more than 40 buffers, W or W' > 24, coutp > 128, a conv that is not
 * 1 x {1, 3, 7}, a stack whose activations and weight ring exceed 160 KB of LDS.  Nothing is
 * written when an error is returned. */
int fvp_conv_stack_run_fused_1d(const FvpConvOp* ops, int nops, const float* params, const float* in,
                                float* out, int planes, fvp_stream_t s);

/* Pack one conv's parameters from the reference's state_dict tensors (device copies):
 * weight [cout][cin][kh][kw] (or [cin][cout][kh][kw] when transposed) -> [tap][cinp][coutp];
 * bias / BN vectors -> bias|scale|shift with scale = gamma/sqrt(var+eps), shift = beta - mean*scale
 * (scale = 1, shift = 0 when bn_* are NULL). */
int fvp_pack_conv(const float* weight, const float* bias, const float* bn_gamma, const float* bn_beta,
                  const float* bn_mean, const float* bn_var, float eps, int transposed, const FvpConvOp* op,
                  float* params, fvp_stream_t s);

/* ---- a-6/a-7: NMS + top-k (bit-exact indices) -------------------------------------------------
 * hm2d [B][X][Y].  keep = (x == maxpool3x3(x)) ? x : 0 ; top-N by (value desc, flat index asc).
 * vals [B][N] fp32, idx [B][N][2] int64 = (flat / X, flat % X) -- the reference divides by
 * shape[1] = X (core/proposal.py:16-17), flat [B][N] int64.  Replaces core/proposal.py:13-33.
 * One workgroup per frame with the map in LDS: FVP_ELIMIT when X * Y * 4 + 128 bytes exceed the CU's 160 KB
 * (X * Y > 40 928, e.g. beyond 200 x 200); maps up to 128 x 128 take the register-resident fast path. */
int fvp_nms_topk(const float* hm2d, int B, int X, int Y, int N, float* vals, int64_t* idx, int64_t* flat,
                 fvp_stream_t s);

/* ---- a-8: gathers at the top-k cells ------------------------------------------------------------
 * bbox_map [B][2][X][Y] -> bbox_flat [B][X*Y][2] (the 4th output of HumanDetectionNet.forward,
 * may be NULL) and match_bbox [B][N][2]; cubes [B][J][X][Y][Z] -> feat1d [B*N][J][Z]
 * (cubes and feat1d may both be NULL: the columns then come from fvp_project_columns).
 * Replaces human_detection_net.py:88-93. */
int fvp_gather_proposals(const float* bbox_map, const float* cubes, const int64_t* flat, int B, int J, int X,
                         int Y, int Z, int N, float* bbox_flat, float* match_bbox, float* feat1d,
                         fvp_stream_t s);

/* ---- a-10/a-11: z arg-max, confidence product, proposal packing ---------------------------------
 * hm1d [B*N][Z]; idx2d from fvp_nms_topk.  topk_index [B][N][3] int64 (may be NULL);
 * centers [B][N][7] = (x,y,z mm = idx*scale + bias as fp32 mul then add, no FMA), valid-1,
 * conf, bbox_w, bbox_h.  sb = scale[3], bias[3].  valid [B][N] uint8 (may be NULL) = centers[...,3] >= 0,
 * the `mask` faster_voxelpose.py:45 hands to the joint localisation net (ABI 8: written here instead of by a
 * separate comparison launch).  Replaces human_detection_net.py:95-102 and ProposalLayer.forward :44-65
 * (eval branch). */
int fvp_proposals(const float* hm1d, const float* conf2d, const int64_t* idx2d, const float* match_bbox,
                  const float* sb, float min_score, int B, int N, int Z, int64_t* topk_index, float* centers,
                  uint8_t* valid, fvp_stream_t s);

/* ---- a-11 standalone: ProposalLayer.forward, eval branch (human_detection_net.py:44-65) -----------
 * topk_index [B][N][3] int64 (voxel indices x, y, z), topk_confs [B][N], match_bbox [B][N][2];
 * centers [B][N][7] = (idx.float() * scale + bias as fp32 mul then add, no FMA), (conf > min_score) - 1,
 * conf, bbox_w, bbox_h.  sb = scale[3], bias[3].  The forward path uses the fused fvp_proposals; this is
 * the module-level drop-in for callers that invoke the layer on its own. */
int fvp_proposal_layer(const int64_t* topk_index, const float* topk_confs, const float* match_bbox, const float* sb,
                       float min_score, int B, int N, float* centers, fvp_stream_t s);

/* ---- a-17/a-18 first half: soft-argmax + WeightNet per (person, plane, joint) map ----------------
 * feat [nP][3][J][C][C] (P2PNet output).  For each map: softmax(beta*x) over C*C cells,
 * expectation of center_grid[plane] ([3][C*C][2]) accumulated in fp64, max probability;
 * WeightNet (conv 1->F k3 + BN + maxpool2 + ReLU + global avg + MLP F->Hd->1 + sigmoid,
 * lib/models/weight_net.py:69-80) from wn = packed WeightNet parameters (see fvp_pack_weightnet).
 * pose2d [nP][3][J][2] (offset NOT yet added), pmax [nP][3][J], wgt [nP][3][J]. */
int fvp_softargmax_weightnet(const float* feat, const float* center_grid, const float* wn, float beta,
                             int nP, int J, int C, int F, int Hd, const uint8_t* person_valid, float* pose2d,
                             float* pmax, float* wgt, fvp_stream_t s);
int fvp_pack_weightnet(const float* conv_w, const float* conv_b, const float* bn_gamma, const float* bn_beta,
                       const float* bn_mean, const float* bn_var, float eps, const float* fc1_w,
                       const float* fc1_b, const float* fc2_w, const float* fc2_b, int F, int Hd, float* wn,
                       fvp_stream_t s);

/* ---- a-18 second half / a-19: offsets, fusion, scatter-back ---------------------------------------
 * Adds offset per plane (joint_localization_net.py:87-90), normalises the weight pairs and
 * blends (:44-62), conf = mean over (plane, joint) of pmax (:27-28); writes rows of
 * fused_poses [B*N][J][5] (x,y,z, valid flag, conf), plane_poses [3][B*N][J][2] and
 * proposal_centers[..][4] = conf for valid persons (:96-98, faster_voxelpose.py:102-103).
 * Invalid persons get xyz = 0 and keep their HDN confidence. */
int fvp_fuse_poses(const float* pose2d, const float* pmax, const float* wgt, const float* offset,
                   const uint8_t* person_valid, int nP, int J, float* centers, float* fused_poses,
                   float* plane_poses, fvp_stream_t s);

/* ---- "next" row f-2: input heatmaps rasterised from 2-D detections ------------------------------------
 * joints [nimg][P][J][2] float64 in NETWORK-image pixels (already through the resize affine, as
 * JointsDataset.py:149-151 leaves them), num_people [nimg] <= P.  Writes Gaussian heatmaps
 * [nimg][J][H][W] (heat_nchw, the reference layout) and / or the channels-last staging copy
 * [nimg][H*W][JP] the projection kernels read (heat_cl; either may be NULL).  Replaces
 * JointsDataset.generate_input_heatmap (lib/dataset/JointsDataset.py:271-338, eval branch) and
 * compute_human_scale (:197-203); float64 scalar arithmetic like numpy, one rounding to fp32.
 * Counts: image i stamps its first min(max(num_people[i], 0), P) people; a count above P is clamped, a negative one is an
 * empty image.  Every requested output element is written (+0.0 where nothing is stamped, and in the channels J..JP-1).
 * Non-finite joints: a joint with a coordinate that is not finite (fabs(x) <= DBL_MAX fails for the coordinate or for its
 * quotient by the stride: NaN, +-Inf) stamps nothing and is left out of its person's extent in compute_human_scale; a
 * person with no finite joint stamps nothing.  (The reference raises in int(nan).)  Finite coordinates of any magnitude
 * behave as the reference's Python integers do: a window beyond the image is skipped.
 * FVP_EINVAL: null joints or num_people; both outputs null; nimg or P < 0; J, W or H < 1; a stride or sigma that is not
 * > 0 or not finite; JP < J with heat_cl set.  nimg == 0 returns 0 before any limit check and writes nothing.
 * FVP_ELIMIT: J * W * 4 > 32 KB (one row of all joints in LDS), P > 64, P * J > 1024.  Nothing is written when an error is
 * returned. */
int fvp_rasterise_heatmaps(const double* joints, const int32_t* num_people, int nimg, int P, int J, int W, int H,
                           double feat_stride_x, double feat_stride_y, double sigma, float* heat_nchw,
                           float* heat_cl, int JP, fvp_stream_t s);

/* ---- "next" row f-3: camera frames -> backbone input ---------------------------------------------------
 * frames [N][Hs][Ws][3] uint8 HWC at the camera's resolution (contiguous) -> the network image of H x W:
 * bilinear warp + channel swap + / 255 + mean / std in one pass.  Replaces the reference's offline resize
 * (preprocess.py: cv2.warpAffine(image, trans, image_size, flags=INTER_LINEAR) with the matrix of
 * get_resize_transform) and its loader (lib/dataset/JointsDataset.py:129-133 imread / BGR->RGB / transform,
 * run/validate.py:44-52 ToTensor + Normalize).
 *   inv  [6]  HOST memory, passed to the kernel by value: destination pixel -> source pixel, row-major 2x3 (the
 *             inverse of resize_transform);
 *   mean, stdv [3]  HOST memory, by value, in OUTPUT channel order;
 *   flags     FVP_INGEST_SWAP_RB: output channel c reads source channel 2 - c (COLOR_BGR2RGB);
 *             FVP_INGEST_GENERAL: accepted, no effect - the general (gather) form is the only one shipped; an
 *             LDS-staged form for axis-aligned matrices computed the same bits and was not faster;
 *   nhwc8     (may be NULL) [N][H][W/2] pixel pairs of 8 bf16 = fvp_bb_input's layout, channel 3 = 0;
 *   nchw      (may be NULL) [N][3][H][W] fp32 (torch backbones, tests).  W even.
 * Arithmetic, fp32, every operation rounded on its own (no fma, IEEE divisions), x, y = destination pixel:
 *   sx = inv[0]*x + inv[1]*y + inv[2],  sy = inv[3]*x + inv[4]*y + inv[5]          (left to right)
 *   x0 = floor(sx), y0 = floor(sy), fx = sx - x0, fy = sy - y0
 *   p00..p11 = the four source bytes of the channel; a tap outside [0,Ws) x [0,Hs) is 0 (BORDER_CONSTANT 0)
 *   v   = (1-fy)*((1-fx)*p00 + fx*p01) + fy*((1-fx)*p10 + fx*p11)
 *   out = ((v / 255) - mean[c]) / stdv[c];   bf16 = round-to-nearest-even of out (as fvp_bb_input)
 * With the identity matrix and Hs, Ws == H, W this is ToTensor + Normalize in fp32.  Not bit-compatible with
 * OpenCV's fixed-point INTER_LINEAR.  N == 0 returns 0 without a launch. */
enum { FVP_INGEST_SWAP_RB = 1, FVP_INGEST_GENERAL = 2 };
int fvp_ingest_frames(const uint8_t* frames, int N, int Hs, int Ws, const float inv[6], const float mean[3],
                      const float stdv[3], int H, int W, int flags, uint16_t* nhwc8, float* nchw, fvp_stream_t s);

/* ---- NV12 camera frames -> backbone input (ABI 10) ------------------------------------------------------
 * The surface a hardware decoder or a capture card leaves in device memory, read directly: colour conversion +
 * bilinear warp + / 255 + mean / std in one pass, no RGB frame in between.  An NV12 frame of Hs x Ws (both even):
 *   y   Hs rows of Ws luma bytes, y_pitch bytes from row to row, y_frame_stride bytes from frame to frame;
 *   uv  Hs/2 rows of Ws/2 interleaved (U, V) byte pairs, uv_pitch bytes from row to row, uv_frame_stride bytes
 *       from frame to frame.  y and uv are separate DEVICE pointers: uv = y + Hs * pitch for a contiguous NV12
 *       buffer, or a plane of its own.  A (U, V) pair is read as one 2-byte load: uv, uv_pitch and
 *       uv_frame_stride must be even.
 * The SOURCE RGB PIXEL at integer (xi, yi) is defined in int32 arithmetic; chroma is replicated, not
 * interpolated (the sample at (xi >> 1, yi >> 1) serves its 2 x 2 luma quad):
 *   c = max(0, Y[yi][xi] - yoff)      d = U[yi>>1][xi>>1] - 128      e = V[yi>>1][xi>>1] - 128
 *   R = clip(0, 255, (CY*c + CRV*e          + (1 << 19)) >> 20)          (>> is arithmetic: floor)
 *   G = clip(0, 255, (CY*c + CGU*d + CGV*e  + (1 << 19)) >> 20)
 *   B = clip(0, 255, (CY*c + CBU*d          + (1 << 19)) >> 20)
 * with the constants of the colour standard below: round(k * 2^20) of the standard's float64 coefficients
 * (limited range: yoff 16, luma gain 255/219, chroma gain g = 255/224; full range: yoff 0, gains 1;
 * CRV = 2(1-Kr)g, CBU = 2(1-Kb)g, CGU = -CBU*Kb/Kg, CGV = -CRV*Kr/Kg; BT.601 Kr 0.299 Kb 0.114, BT.709 Kr 0.2126
 * Kb 0.0722).  Every intermediate stays below 5.8e8 in magnitude.  No bit-compatibility with any particular
 * library's converter is claimed.
 * From the source RGB pixel on, the arithmetic is exactly that of fvp_ingest_frames with flags = 0 (output channel 0
 * is R): coordinates through inv, floor, four taps with a zero border (a tap outside [0,Ws) x [0,Hs) is 0 and is
 * not converted), the same fp32 bilinear expression, / 255, - mean, / stdv, bf16 round-to-nearest-even.  Hence:
 * THE OUTPUTS OF fvp_ingest_nv12 EQUAL, BIT FOR BIT, fvp_ingest_frames APPLIED TO THE RGB uint8 FRAME OBTAINED BY
 * CONVERTING EVERY SOURCE PIXEL WITH THE FORMULA ABOVE.
 * inv, mean, stdv: HOST memory, by value, as for fvp_ingest_frames; nhwc8 / nchw as there (either may be NULL).
 * FVP_EINVAL: a null pointer or both outputs null; odd Hs, Ws or W; y_pitch < Ws or uv_pitch < Ws; odd uv_pitch,
 * uv address or uv_frame_stride; unknown standard; non-finite inv / mean / stdv or stdv == 0.  FVP_ELIMIT as
 * fvp_ingest_frames.  N == 0 returns 0 without a launch. */
enum { FVP_YUV_BT601_LIMITED = 0, FVP_YUV_BT709_LIMITED = 1, FVP_YUV_BT601_FULL = 2, FVP_YUV_BT709_FULL = 3 };
/*                                      yoff  CY       CRV      CGU      CGV      CBU */
#define FVP_YUV_BT601_LIMITED_COEFFS { 16, 1220945, 1673555, -410793, -852458, 2115221 }
#define FVP_YUV_BT709_LIMITED_COEFFS { 16, 1220945, 1879825, -223607, -558796, 2215014 }
#define FVP_YUV_BT601_FULL_COEFFS { 0, 1048576, 1470104, -360853, -748826, 1858077 }
#define FVP_YUV_BT709_FULL_COEFFS { 0, 1048576, 1651297, -196424, -490864, 1945738 }
int fvp_ingest_nv12(const uint8_t* y, const uint8_t* uv, int N, int Hs, int Ws, long y_pitch, long uv_pitch,
                    long y_frame_stride, long uv_frame_stride, /* bytes */
                    int standard, const float inv[6], const float mean[3], const float stdv[3], int H, int W,
                    uint16_t* nhwc8, float* nchw, fvp_stream_t s);

/* ---- Bayer raw camera frames (ABI 24): fvp_demosaic_bayer, fvp_ingest_bayer ---------------------------------------------
 * What a machine-vision camera delivers: the sensor's 8-bit Bayer mosaic (BayerRG8 / GR8 / GB8 / BG8), one byte per pixel.
 * fvp_ingest_bayer takes it to the backbone input in one pass, with no RGB frame in between; fvp_demosaic_bayer writes the
 * RGB frame for the stages that work on one.  Everything up to the source RGB pixel is exact integer arithmetic; no
 * bit-compatibility with any library's demosaic is claimed.
 * Frame: raw is a DEVICE pointer to N frames of Hs rows of Ws bytes, Hs and Ws both even and >= 4, pitch >= Ws bytes from
 * row to row, frame_stride bytes from frame to frame.  Pitch, stride and the address may be odd: no alignment is required.
 * pattern names the 2 x 2 cell at the frame's top-left corner by where its red sample (rx, ry) lies:
 *   FVP_BAYER_RGGB 0: (0, 0)    FVP_BAYER_GRBG 1: (1, 0)    FVP_BAYER_GBRG 2: (0, 1)    FVP_BAYER_BGGR 3: (1, 1)
 * The site (x, y) is red if (x&1) == rx and (y&1) == ry, blue if both differ, green otherwise; a green site is "in a red
 * row" if (y&1) == ry, else "in a blue row".
 * Border: a neighbour index outside the frame is reflected about the edge sample without repeating it (i < 0 -> -i,
 * i >= n -> 2(n-1) - i).  Offsets are at most 2 and n >= 4, so the result is inside; reflection keeps the parity, so a
 * reflected neighbour has the colour the formula expects.
 * Neighbour sums at (x, y), int32, raw(dy, dx) the reflected neighbour:
 *   c  = raw(0,0)               H1 = raw(0,-1) + raw(0,1)      V1 = raw(-1,0) + raw(1,0)
 *   D  = raw(-1,-1) + raw(-1,1) + raw(1,-1) + raw(1,1)         H2 = raw(0,-2) + raw(0,2)      V2 = raw(-2,0) + raw(2,0)
 * Sixteenths of the three colours - the Malvar-He-Cutler 5 x 5 linear filter with its coefficients doubled so that all are
 * integers; "third colour" is the non-green colour the site does not carry:
 *   the site's own colour                                          16c
 *   green at a red or blue site                                    8c + 4(H1 + V1) - 2(H2 + V2)
 *   the third colour at a red or blue site                         12c + 4D - 3(H2 + V2)
 *   at a green site, the colour of its row neighbours
 *   (red in a red row, blue in a blue row)                         10c + 8 H1 - 2D - 2 H2 + V2
 *   at a green site, the colour of its column neighbours           10c + 8 V1 - 2D - 2 V2 + H2
 * value = clip(0, 255, (X16 + 8) >> 4), >> arithmetic; every X16 lies in [-3060, 7140].
 * tone: a DEVICE pointer to uint8 [3][256], or NULL (the identity).  After the clip R = tone[0][R], G = tone[1][G],
 * B = tone[2][B]: one table carries black level, white-balance gains and gamma for sensors that deliver linear data.
 * The triple is the SOURCE RGB PIXEL at integer (xi, yi).
 * fvp_demosaic_bayer writes every source RGB pixel to rgb [N][Hs][Ws][3] in R, G, B order: the contiguous HWC layout that
 * fvp_ingest_frames, fvp_draw_poses, fvp_crop_rois, fvp_person_signature and fvp_anonymise_rois take.  flags must be 0.
 * fvp_ingest_bayer: from the source RGB pixel on, the arithmetic is exactly that of fvp_ingest_frames with flags = 0 (output
 * channel 0 is R): coordinates through inv, floor, four taps with a zero border (a tap outside [0,Ws) x [0,Hs) is 0 and is
 * not demosaiced), the same fp32 bilinear expression, / 255, - mean, / stdv, bf16 round-to-nearest-even.  Hence:
 * THE OUTPUTS OF fvp_ingest_bayer EQUAL, BIT FOR BIT, fvp_ingest_frames (flags = 0) APPLIED TO THE OUTPUT OF
 * fvp_demosaic_bayer.  inv, mean, stdv: HOST memory, by value; nhwc8 / nchw as for fvp_ingest_frames (either may be NULL).
 * Which of its two kernels runs (the source rectangle of a 64 x 8 destination tile demosaiced once in LDS, or a gather that
 * demosaics per tap when that rectangle does not fit) is a function of inv, H, W, Hs, Ws only and changes no bit.
 * FVP_EINVAL: a null raw, inv, mean or stdv; a null rgb (demosaic); both outputs null (ingest); N < 0; Hs or Ws odd or < 4;
 * pitch < Ws; pattern outside 0..3; non-zero flags; odd W, or H or W < 1; non-finite inv, mean or stdv, or stdv == 0.
 * FVP_ELIMIT: the ingest as fvp_ingest_frames; the demosaic Hs or Ws > 16384, or a grid of 2^31 or more workgroups (one per
 * 256 x 8 pixels).  Nothing is written when an error is returned.  N == 0 returns 0 without a launch.
 * Not built: 10-, 12- or 16-bit and packed raw formats; gains applied to the mosaic before interpolation (the tone table
 * acts after it); edge-directed demosaics; a pitched RGB output; Bayer input for the overlay, the crops or the anonymiser
 * directly - they take the demosaiced frame. */
enum { FVP_BAYER_RGGB = 0, FVP_BAYER_GRBG = 1, FVP_BAYER_GBRG = 2, FVP_BAYER_BGGR = 3 };
int fvp_demosaic_bayer(const uint8_t* raw, int N, int Hs, int Ws, long pitch, long frame_stride, /* bytes */
                       int pattern, const uint8_t* tone, int flags, uint8_t* rgb /* [N][Hs][Ws][3] */, fvp_stream_t s);
int fvp_ingest_bayer(const uint8_t* raw, int N, int Hs, int Ws, long pitch, long frame_stride, /* bytes */
                     int pattern, const uint8_t* tone, const float inv[6], const float mean[3], const float stdv[3], int H,
                     int W, uint16_t* nhwc8, float* nchw, fvp_stream_t s);

/* ---- skeleton overlay (ABI 14): the poses drawn onto the camera frames they were computed from ------------------------
 * Counterpart of the reference's host-side lib/utils/vis.py::save_image_with_poses (cv2.circle / cv2.line per view), on the
 * device and in place.  frames [B*V][Hs][Ws][3] uint8 is the contiguous HWC layout of fvp_ingest_frames: frame b*V + v
 * belongs to views[b][v].  views [B][V][N][J][4] = (px, py, depth, s) as fvp_joint_evidence writes them (pixels of the
 * ORIGINAL frame); ids [B][N] int32 (fvp_track_update) or NULL; joint_conf [B][N][J] or NULL.  limbs [L][2] int32 (joint
 * index pairs) and palette [P][3] uint8 are HOST memory and go to the kernel by value, as inv / mean do.
 * Geometry: integers, in sixteenths of a pixel ("Q4"); the centre of pixel (x, y) is (16x, 16y).
 * Drawable joint (b,v,n,j): depth > 0, and |px| <= 32768 and |py| <= 32768 (fp32 compares: a NaN or an Inf fails them),
 *   and joint_conf is NULL or joint_conf[b][n][j] >= conf_min (a NaN confidence is not drawable).  Its Q4 position is
 *   q = (rint(px * 16), rint(py * 16)), round-half-even; the product by 16 is exact.
 * Drawn person: n of frame b is drawn iff ids is NULL or ids[b][n] >= 0; its colour is palette[key % P] with
 *   key = ids ? ids[b][n] : n.  Invalid slots need no flag: fvp_joint_evidence writes them as zeros, so their depth is 0.
 * Primitives of person n in view v: a disc of radius joint_radius_q4 around every drawable joint; for every limb (i, k)
 *   whose two joints are both drawable, the capsule of half-width limb_half_q4 around the segment a = q_i, b = q_k.
 * Coverage of a pixel centre p, all comparisons in exact integers:
 *   disc:     |p-q|^2 <= R^2;
 *   capsule:  with d = b-a, w = p-a, t = w.d, dd = d.d:   t <= 0 (this includes dd == 0): |w|^2 <= W^2;
 *             t >= dd: |p-b|^2 <= W^2;   otherwise: (w_x d_y - w_y d_x)^2 <= W^2 * dd.
 * Paint: for every pixel of the frame, for n = 0 .. N-1 in ascending order: if any primitive of person n covers the pixel,
 *   then ONCE per person and per channel   dst = (colour * alpha + dst * (256 - alpha) + 128) >> 8.
 *   Overlapping primitives of one person blend once; persons blend one over the other in slot order.  Pixels that nothing
 *   covers are neither read nor written.
 * One workgroup per 64 x 16 pixel tile of one frame collects the primitives whose bounding box meets the tile and its
 * pixels evaluate them: no two workgroups write the same byte, the result does not depend on scheduling.
 * FVP_EINVAL: null frames, views or palette; limbs null with L > 0; B or V < 0; N, J, Hs, Ws or P < 1; L < 0; a limb index
 * outside [0, J); alpha outside [1, 256]; joint_radius_q4 or limb_half_q4 outside [0, 1024]; NaN conf_min.
 * FVP_ELIMIT: N > 32, J > FVP_MAX_JOINTS, V > FVP_MAX_VIEWS, L > 64, P > 64, Hs or Ws > 16384, B * V > 65535 (one grid
 * plane per frame).  Nothing is written when an error is returned.  B * V == 0 returns 0 without a launch.
 * No bit-compatibility with OpenCV's rasteriser is claimed.  NV12 surfaces: fvp_draw_poses_nv12 below.  Not built: text
 * labels, anti-aliasing, pitched RGB frames. */
int fvp_draw_poses(uint8_t* frames /* [B*V][Hs][Ws][3], in place */, int B, int V, int Hs, int Ws,
                   const float* views /* [B][V][N][J][4] of fvp_joint_evidence */,
                   const int32_t* ids /* [B][N] or NULL */, const float* joint_conf /* [B][N][J] or NULL */,
                   int N, int J, const int32_t* limbs /* HOST [L][2], may be NULL when L == 0 */, int L,
                   const uint8_t* palette /* HOST [P][3] */, int P,
                   int joint_radius_q4, int limb_half_q4, int alpha, float conf_min, fvp_stream_t s);

/* ---- skeleton overlay on NV12 surfaces (ABI 15) -------------------------------------------------------------------------
 * fvp_draw_poses for the surface fvp_ingest_nv12 reads, in place, with no RGB frame in between.  y, uv, y_pitch, uv_pitch,
 * y_frame_stride, uv_frame_stride (bytes) and standard are those of fvp_ingest_nv12: Hs x Ws luma bytes and Hs/2 x Ws/2
 * interleaved (U, V) pairs per frame, Hs and Ws even, uv at an even address; frame b*V + v belongs to views[b][v].  views,
 * ids, joint_conf, limbs, joint_radius_q4, limb_half_q4, alpha and conf_min are those of fvp_draw_poses.  THE CALLER
 * GUARANTEES THAT THE TWO PLANES DO NOT OVERLAP (any frame of one with any frame of the other, padding aside).
 * Coverage: drawable joints, drawn persons, Q4 geometry, the disc and the capsule test are exactly those of fvp_draw_poses;
 *   person n covers luma pixel (x, y) iff one of its primitives covers the pixel centre (16x, 16y).  No new geometry.
 * Colour: palette [P][3] is R, G, B in HOST memory.  Each entry is converted once, on the host, in int32:
 *     Yc = clip(0, 255, YOFF + ((CYR*R + CYG*G + CYB*B + 32768) >> 16))          (>> is arithmetic: floor)
 *     Uc = clip(0, 255, UOFF + ((CUR*R + CUG*G + CUB*B + 32768) >> 16))
 *     Vc = clip(0, 255, VOFF + ((CVR*R + CVG*G + CVB*B + 32768) >> 16))
 *   with the twelve constants of the standard below: the offsets, and round(k * 2^16) of the float64 values
 *     luma (Kr, Kg, Kb) * sy;   U (-Kr, -Kg, 1-Kb) / (2 (1-Kb)) * sc;   V (1-Kr, -Kg, -Kb) / (2 (1-Kr)) * sc
 *   (Kg = 1 - Kr - Kb; limited range: sy = 219/255, sc = 224/255, YOFF 16; full range: sy = sc = 1, YOFF 0; UOFF = VOFF =
 *   128; Kr, Kb as for fvp_ingest_nv12).  Over all 2^24 colours limited range gives Y in 16..235 and U, V in 16..240
 *   without the clip; full range reaches 256 on U (pure blue) and V (pure red): there the clip is part of the definition.
 * Luma paint: for n = 0 .. N-1 ascending: if person n covers the pixel, ONCE per person
 *     Y = (Yc * alpha + Y * (256 - alpha) + 128) >> 8.
 * Chroma paint: the sample (cx, cy) serves the luma quad (2cx .. 2cx+1, 2cy .. 2cy+1).  With k_n in 0..4 the number of the
 *   quad's pixels person n covers: for n ascending with k_n > 0, ONCE per person, a = alpha * k_n (1..1024):
 *     U = (Uc * a + U * (1024 - a) + 512) >> 10        V = (Vc * a + V * (1024 - a) + 512) >> 10.
 *   A partly covered quad takes the colour in proportion (a box filter); alpha = 256 and k = 4 write Uc, Vc exactly.
 * Never read and never written: a luma byte nothing covers; a (U, V) pair whose quad has every k_n = 0; every byte of pitch
 *   padding and between frames.
 * One workgroup per 64 x 16 luma tile (32 x 8 chroma samples) of one frame, one thread per quad: tiles start at even
 * coordinates, no two workgroups touch the same byte, the result does not depend on scheduling.  A (U, V) pair is one
 * 2-byte load and one 2-byte store; luma goes byte by byte, nothing is required of y's alignment.
 * FVP_EINVAL: as fvp_draw_poses (null y or uv for null frames), and: odd Hs or Ws; y_pitch < Ws or uv_pitch < Ws; odd uv
 * address, uv_pitch or uv_frame_stride; unknown standard; with B * V > 1, y_frame_stride < (Hs-1) * y_pitch + Ws or
 * uv_frame_stride < (Hs/2-1) * uv_pitch + Ws.  FVP_ELIMIT as fvp_draw_poses.  Nothing is written when an error is
 * returned.  B * V == 0 returns 0 without a launch.  Not built: text labels, anti-aliasing, planar (I420) or 10-bit (P010)
 * surfaces. */
/*                                          YOFF  CYR    CYG    CYB  UOFF   CUR     CUG    CUB  VOFF   CVR    CVG    CVB */
#define FVP_RGB2YUV_BT601_LIMITED_COEFFS { 16, 16829, 33039, 6416, 128, -9714, -19071, 28784, 128, 28784, -24103, -4681 }
#define FVP_RGB2YUV_BT709_LIMITED_COEFFS { 16, 11966, 40254, 4064, 128, -6596, -22189, 28784, 128, 28784, -26145, -2639 }
#define FVP_RGB2YUV_BT601_FULL_COEFFS { 0, 19595, 38470, 7471, 128, -11058, -21710, 32768, 128, 32768, -27439, -5329 }
#define FVP_RGB2YUV_BT709_FULL_COEFFS { 0, 13933, 46871, 4732, 128, -7509, -25259, 32768, 128, 32768, -29763, -3005 }
int fvp_draw_poses_nv12(uint8_t* y, uint8_t* uv /* in place */, int B, int V, int Hs, int Ws, long y_pitch, long uv_pitch,
                        long y_frame_stride, long uv_frame_stride, /* bytes */
                        int standard /* FVP_YUV_* */, const float* views /* [B][V][N][J][4] */,
                        const int32_t* ids /* [B][N] or NULL */, const float* joint_conf /* [B][N][J] or NULL */,
                        int N, int J, const int32_t* limbs /* HOST [L][2], may be NULL when L == 0 */, int L,
                        const uint8_t* palette /* HOST [P][3], R G B */, int P,
                        int joint_radius_q4, int limb_half_q4, int alpha, float conf_min, fvp_stream_t s);

/* ---- person crops out (ABI 16): per-view person boxes, and crop + resize + normalise in one pass ------------------------
 * What a rig does with a person after the pose - appearance features, a top-down 2-D refiner, face blurring, an action
 * classifier - starts from a fixed-size, normalised image patch of that person in the view that sees them best.
 * fvp_person_rois turns the per-view pixels of fvp_joint_evidence into one box per (frame, view, person);
 * fvp_crop_rois / fvp_crop_rois_nv12 cut any list of boxes out of the camera frames with the ingest's arithmetic.
 *
 * fvp_person_rois.  views [B][V][N][J][4], ids [B][N] or NULL, joint_conf [B][N][J] or NULL and conf_min are those of
 * fvp_draw_poses.  joint_mask: bit j selects joint j (bits >= J are ignored).
 * Usable joint (b,v,n,j): bit j of joint_mask is set and the joint is drawable by fvp_draw_poses' rule: depth > 0, |px| <=
 *   32768 and |py| <= 32768 (fp32 compares: a NaN or an Inf fails them), and joint_conf is NULL or joint_conf[b][n][j] >=
 *   conf_min (a NaN confidence is not usable).
 * Selected person: ids is NULL or ids[b][n] >= 0.   k = the number of usable joints of (b,v,n).
 * The box is VALID iff the person is selected and k >= min_joints.  For a valid box, with xmin, xmax, ymin, ymax the exact
 * minimum / maximum of px, py over the usable joints (taken in ascending j: the first usable value, replaced by a later one
 * iff that compares < resp. >), in fp32, every operation rounded on its own, IEEE division:
 *     cx = (xmin + xmax) * 0.5f                          cy = (ymin + ymax) * 0.5f
 *     hw = ((xmax - xmin) * 0.5f) * scale + pad_px       hh = ((ymax - ymin) * 0.5f) * scale + pad_px
 *     if (hw < hh * aspect) hw = hh * aspect; else hh = hw / aspect;              (aspect = width / height of the crop)
 *     roi = (cx - hw, cy - hh, cx + hw, cy + hh)         pixels of the ORIGINAL frame, NOT clipped to the frame
 * A single usable joint with pad_px = 0 gives a degenerate box (x1 == x0), which fvp_crop_rois answers with zeros.
 * Outputs, every element written by every call; each may be NULL, not all three:
 *     rois      [B][V][N][4] fp32 (x0, y0, x1, y1);
 *     roi_count [B][V][N]    int32 = k;
 *     roi_score [B][V][N]    fp32 = (s summed over the usable joints in ascending j, from 0) / float(k), s = views[...][3]:
 *                            the mean heatmap support of the box's joints in that view - argmax over V picks the best view.
 * An invalid box writes zeros to all three.
 * FVP_EINVAL: null views or all three outputs null; B or V < 0; N, J or min_joints < 1; scale not > 0, pad_px not >= 0,
 * aspect not > 0, any of them not finite; NaN conf_min.  FVP_ELIMIT: N > 32, J > FVP_MAX_JOINTS, V > FVP_MAX_VIEWS.  Nothing
 * is written when an error is returned.  B * V == 0 returns 0 without a launch.  One thread per box. */
int fvp_person_rois(const float* views /* [B][V][N][J][4] of fvp_joint_evidence */, const int32_t* ids /* [B][N] or NULL */,
                    const float* joint_conf /* [B][N][J] or NULL */, int B, int V, int N, int J, uint32_t joint_mask,
                    int min_joints, float scale, float pad_px, float aspect, float conf_min,
                    float* rois /* [B][V][N][4] */, int32_t* roi_count /* [B][V][N] */, float* roi_score /* [B][V][N] */,
                    fvp_stream_t s);

/* fvp_crop_rois / fvp_crop_rois_nv12: a generic crop-and-resize, any caller-made boxes.  The frames are those of
 * fvp_ingest_frames ([F][Hs][Ws][3] uint8, flags = 0 or FVP_INGEST_SWAP_RB) resp. fvp_ingest_nv12 (y, uv, pitches, frame
 * strides, standard).  rois [R][4] fp32 (x0, y0, x1, y1) in DEVICE memory, in pixels of the frame; ROI r reads frame
 * r / rois_per_frame, and R == F * rois_per_frame.  mean, stdv [3]: HOST memory, by value, OUTPUT channel order.  The crop is
 * h rows of w pixels, w even.  Outputs as the ingest's, one image per ROI (either may be NULL, not both):
 *     nhwc8 [R][h][w/2] pixel pairs of 8 bf16, channel 3 = 0;      nchw [R][3][h][w] fp32.
 * ROI r is CROPPABLE iff its four values are finite (fabsf <= FLT_MAX) and x1 > x0 and y1 > y0.  For a croppable ROI, in the
 * kernel, fp32, every operation rounded on its own, IEEE division:
 *     ax = (x1 - x0) / float(w)      bx = (x0 + 0.5f * ax) - 0.5f          (pixel centres map to pixel centres)
 *     ay = (y1 - y0) / float(h)      by = (y0 + 0.5f * ay) - 0.5f
 *     inv = { ax, 0, bx,   0, ay, by }
 * and from there on the arithmetic is that of fvp_ingest_frames (resp. fvp_ingest_nv12) exactly: sx = inv[0]*x + inv[1]*y +
 * inv[2], sy likewise, floor, four taps with a zero border (a tap outside the frame is 0 and, for NV12, is not converted),
 * the same bilinear expression, / 255, - mean, / stdv, bf16 round-to-nearest-even.  Hence:
 * CROP r EQUALS, BIT FOR BIT, fvp_ingest_frames (RESP. fvp_ingest_nv12) ON FRAME r / rois_per_frame WITH THAT inv, H = h, W = w.
 * A non-croppable ROI writes an all-zero image (fp32 0, bf16 0) and loads no frame byte.  No byte outside a frame's pixels -
 * pitch padding, the gap between frames - is ever read.  A crop that shrinks by more than 2 x aliases as the ingest does.
 * One workgroup handles 256 pixel pairs of ONE ROI (the ROI is a grid dimension): the four floats and inv are wave-uniform.
 * FVP_EINVAL: as fvp_ingest_frames / fvp_ingest_nv12 (inv aside), and: null rois; F or R < 0; rois_per_frame < 1; R != F *
 * rois_per_frame; a flag other than FVP_INGEST_SWAP_RB.  FVP_ELIMIT: as the ingest calls; more than 65535 * 256 pixel pairs
 * per crop.  Nothing is written when an error is returned.  R == 0 returns 0 without a launch.  Not built: rotated boxes,
 * anti-aliased down-scaling, I420 / P010 surfaces, compaction of the valid crops. */
int fvp_crop_rois(const uint8_t* frames /* [F][Hs][Ws][3] */, int F, int Hs, int Ws, const float* rois /* DEVICE [R][4] */,
                  int R, int rois_per_frame, const float mean[3], const float stdv[3], int h, int w, int flags,
                  uint16_t* nhwc8 /* [R][h][w/2][8] */, float* nchw /* [R][3][h][w] */, fvp_stream_t s);
int fvp_crop_rois_nv12(const uint8_t* y, const uint8_t* uv, int F, int Hs, int Ws, long y_pitch, long uv_pitch,
                       long y_frame_stride, long uv_frame_stride, /* bytes */
                       int standard /* FVP_YUV_* */, const float* rois /* DEVICE [R][4] */, int R, int rois_per_frame,
                       const float mean[3], const float stdv[3], int h, int w, uint16_t* nhwc8, float* nchw,
                       fvp_stream_t s);

/* ---- faces out of the camera frames (ABI 23): fvp_anonymise_rois, fvp_anonymise_rois_nv12 ---------------------------------
 * A rig that records or shows its camera streams usually has to hide who is in them before a frame leaves the machine.
 * fvp_person_rois makes a box from any joint subset, the head's included; fvp_crop_rois only cuts a copy out.  These two
 * calls WRITE BACK: the pixels a list of boxes covers are replaced in place, by a mosaic or by one colour.
 * fvp_anonymise_rois: frames [F][Hs][Ws][3] uint8, the contiguous HWC layout of fvp_ingest_frames / fvp_draw_poses.
 * fvp_anonymise_rois_nv12: the surface of fvp_draw_poses_nv12 - y, uv, y_pitch, uv_pitch, y_frame_stride, uv_frame_stride
 * (bytes) and standard with the same rules (Hs and Ws even, uv at an even address, even uv_pitch and uv_frame_stride), and
 * THE CALLER GUARANTEES THAT THE TWO PLANES DO NOT OVERLAP, as there.
 * rois [R][4] fp32 (x0, y0, x1, y1) in DEVICE memory, in pixels of the frame; R == F * rois_per_frame and ROI r belongs to
 * frame r / rois_per_frame, as for fvp_crop_rois.  cell: 2, 4, 8, 16 or 32.  shape: FVP_ANON_RECT or FVP_ANON_ELLIPSE.  mode:
 * FVP_ANON_MOSAIC or FVP_ANON_FILL.  colour [3] uint8 R, G, B: HOST memory, goes to the kernel by value, used by FILL only
 * (it may be NULL for MOSAIC).
 * Active ROI: all four values v satisfy fabsf(v) <= 65536.0f (an fp32 compare: a NaN or an Inf fails it), and x1 > x0 and
 *   y1 > y0.  Any other ROI is inactive and covers nothing - the all-zero invalid box of fvp_person_rois is one.
 * Coverage: pixel (x, y) has the centre xc = float(x) + 0.5f, yc = float(y) + 0.5f (both exact).  An active ROI covers it
 *   RECT:     iff x0 <= xc && xc < x1 && y0 <= yc && yc < y1;
 *   ELLIPSE:  with cx = (x0 + x1) * 0.5f, hw = (x1 - x0) * 0.5f, dx = xc - cx and cy = (y0 + y1) * 0.5f, hh = (y1 - y0) * 0.5f,
 *             dy = yc - cy:   iff (dx*dx)*(hh*hh) + (dy*dy)*(hw*hw) <= (hw*hw)*(hh*hh)
 *             in fp32, every operation rounded on its own (no fused multiply-add), evaluated as written.  There is no
 *             division, and the bound of 65536 keeps every term finite (below 2^70).  The expression is taken literally
 *             also where it underflows: a box thinner than about 1e-22 pixels both ways has hw*hw == hh*hh == 0 and covers
 *             every pixel of its frame (0 <= 0); no box made from pixel coordinates is that thin.
 *   A pixel is COVERED iff an active ROI of its frame covers it: a union - the order of the ROIs never matters.
 * Cells: anchored at the frame's origin, not at a box.  Cell (i, j) is the pixels [i*cell, min((i+1)*cell, Ws)) x [j*cell,
 *   min((j+1)*cell, Hs)); the last cells of a row / column may be narrower.  A frame-anchored mosaic does not shimmer when
 *   a box moves by a pixel, and overlapping boxes agree on it.  A cell is TOUCHED iff one of its pixels is covered.
 * MOSAIC, RGB: for a touched cell and each channel, S = the sum of the ORIGINAL bytes of ALL n in-frame pixels of the cell,
 *   covered or not;  m = (2*S + n) / (2*n)  in int32 with truncating division (the mean, half up).  Every covered pixel of
 *   the cell becomes m.  Uncovered pixels are not written; untouched cells are neither read nor written.
 * MOSAIC, NV12: luma as above, one channel.  The chroma cell of luma cell (i, j) is its (cell/2) x (cell/2) block of (U, V)
 *   pairs, clipped to (Ws/2) x (Hs/2).  A pair is covered iff any of the four luma pixels of its quad is covered; U and V of
 *   a covered pair become the chroma cell's means, by the same formula over the original in-frame pairs of the cell.  A
 *   chroma cell is read iff its luma cell is touched.
 * FILL: covered pixels become colour; for NV12 colour is converted once, on the host, to (Yc, Uc, Vc) with the
 *   FVP_RGB2YUV_* constants exactly as fvp_draw_poses_nv12 converts a palette entry; covered luma becomes Yc, covered pairs
 *   (Uc, Vc).  No frame byte is read.
 * Never read and never written: pitch padding, the bytes between frames, the bytes of other frames' cells.
 * One workgroup owns a 64 x 32 pixel tile of one frame - whole cells for every permitted cell size.  It reads the frame's
 * ROIs (at most 64) and leaves if none can cover a pixel of the tile; otherwise: coverage, the touched cells marked in LDS,
 * barrier, integer sums of the touched cells in LDS (integer adds commute: the result does not depend on scheduling),
 * barrier, write.  Every read of a cell precedes the barrier and every write follows it, in the one workgroup that owns the
 * cell: that is what makes in place safe.  An NV12 (U, V) pair is one 2-byte load and one 2-byte store, luma goes byte by
 * byte.
 * FVP_EINVAL: null frames (y, uv) or rois; F or R < 0; rois_per_frame < 1; R != F * rois_per_frame; cell not in {2, 4, 8,
 * 16, 32}; unknown shape or mode; FILL with a null colour; Hs or Ws < 1; NV12: every surface rule of fvp_draw_poses_nv12
 * (odd Hs or Ws; y_pitch < Ws or uv_pitch < Ws; odd uv address, uv_pitch or uv_frame_stride; unknown standard; with F > 1,
 * y_frame_stride < (Hs-1) * y_pitch + Ws or uv_frame_stride < (Hs/2-1) * uv_pitch + Ws).  FVP_ELIMIT: rois_per_frame > 64;
 * Hs or Ws > 16384; F > 65535 (one grid plane per frame).  Nothing is written when an error is returned.  R == 0 (hence
 * also F == 0) returns 0 without a launch.  Not built: Gaussian blur, rotated boxes, a face detector, I420 / P010 surfaces,
 * pitched RGB frames. */
int fvp_anonymise_rois(uint8_t* frames /* [F][Hs][Ws][3], in place */, int F, int Hs, int Ws,
                       const float* rois /* DEVICE [R][4] */, int R, int rois_per_frame, int cell,
                       int shape /* FVP_ANON_RECT, _ELLIPSE */, int mode /* FVP_ANON_MOSAIC, _FILL */,
                       const uint8_t* colour /* HOST [3], R G B */, fvp_stream_t s);
int fvp_anonymise_rois_nv12(uint8_t* y, uint8_t* uv /* in place */, int F, int Hs, int Ws, long y_pitch, long uv_pitch,
                            long y_frame_stride, long uv_frame_stride, /* bytes */
                            int standard /* FVP_YUV_* */, const float* rois /* DEVICE [R][4] */, int R, int rois_per_frame,
                            int cell, int shape, int mode, const uint8_t* colour /* HOST [3], R G B */, fvp_stream_t s);

/* ---- joint visibility per view (ABI 17): a device-side occlusion test ---------------------------------------------------
 * fvp_joint_evidence says where a joint lands in every view and what the heatmap holds there, not whether the camera can see
 * it: a joint behind another person's torso still projects into the frame.  With every person's 3-D skeleton and every
 * camera centre in hand the answer is geometry: the ray from the camera centre to the joint is tested against a capsule model
 * of every present person of the frame.
 *
 * fused_poses [B][N][J][5], cams [nsets][V][FVP_CAM_FLOATS] and frame_set [B] are those of fvp_joint_evidence; ids [B][N] int32
 * (fvp_track_update) or NULL; views [B][V][N][J][4] of fvp_joint_evidence, or NULL.  Body model, HOST memory, passed to the
 * kernel by value: prims [L][2] int32 joint index pairs, radius_mm [L].  Primitive (i, k, r) of a person is the capsule of radius r
 * around the 3-D segment from joint i to joint k; i == k is a sphere (a head).
 *
 * fp32, every operation rounded on its own (no contraction), IEEE division and square root:
 *   dot(p,q) = (p0*q0 + p1*q1) + p2*q2          clamp(x,lo,hi) = fminf(fmaxf(x,lo),hi)
 *   person m of frame b is PRESENT iff fused_poses[b][m][0][3] >= 0 and (ids is NULL or ids[b][m] >= 0);
 *   a point is FINITE iff fabsf(c) <= FLT_MAX for its three coordinates;
 *   C = cams[frame_set[b]][v].T (floats 9..11 of the record): the camera centre, as in the projection, d = w - T.
 * For joint (b,v,n,j), P = fused_poses[b][n][j][0:3]:
 *   1. d1 = P - C, a = dot(d1,d1), len = sqrtf(a).  The joint is EVALUATED iff person n is present, P is finite and
 *      len > guard_mm (a NaN fails); otherwise occluder = -2.  smax = 1.0f - guard_mm / len: the last guard_mm of the ray before
 *      the joint are never tested, so the joint's own flesh does not hide it.
 *   2. Candidates: the primitives (i,k,r) of every present person m, A = pose[m][i], B = pose[m][k].  A primitive is skipped
 *      if A or B is not finite, or if m == n and (i == j or k == j): the limbs that end in the joint itself.
 *   3. Closest points of the segments C + s*d1, s in [0,smax], and A + t*d2, t in [0,1] (Ericson, Real-Time Collision
 *      Detection, 5.1.9): d2 = B - A, r0 = C - A, e = dot(d2,d2), f = dot(d2,r0), c = dot(d1,r0).
 *        if e == 0:  t = 0, s = clamp(-c / a, 0, smax)
 *        else:       bb = dot(d1,d2), den = a*e - bb*bb, s = den > 0 ? clamp((bb*f - c*e) / den, 0, smax) : 0,
 *                    t = (bb*s + f) / e;
 *                    if t < 0:       t = 0, s = clamp(-c / a, 0, smax)
 *                    else if t > 1:  t = 1, s = clamp((bb - c) / a, 0, smax)
 *      w = (C + d1*s) - (A + d2*t) per component.  HIT iff dot(w,w) <= r*r (a NaN fails).
 *   4. No hit: occluder = -1, a free line of sight.  Otherwise occluder = m of the hit with the smallest (s, m) in
 *      lexicographic order: the body nearest the camera.  m == n is self-occlusion.
 *   5. With views: view v SEES joint (b,n,j) iff occluder == -1, depth > 0, 0 <= px <= Ws-1 and 0 <= py <= Hs-1 (fp32
 *      compares against float(Ws-1), float(Hs-1); a NaN fails).  vis_count = the number of seeing views; vis_conf =
 *      clamp((s_v summed over the seeing views in ascending v, from 0) / float(vis_count), 0, 1), 0 when the count is 0.  The
 *      summation order is fixed: the result does not depend on scheduling.
 * Outputs, every element of a non-NULL output written by every call; any may be NULL, not all three; vis_conf and vis_count
 * need views:
 *     occluder  [B][V][N][J] int32: -2 not evaluated, -1 visible, else the occluding person's slot;
 *     vis_conf  [B][N][J]    fp32;        vis_count [B][N][J] int32.
 * FVP_EINVAL: null fused_poses, cams or frame_set; prims or radius_mm null with L > 0; all outputs null; vis_conf or vis_count
 * without views; B < 0; V, N, J, Hs or Ws < 1; L < 0; a primitive index outside [0,J); a radius not > 0 or not finite;
 * guard_mm not >= 0 or not finite.  FVP_ELIMIT: N > FVP_VIS_MAX_PEOPLE, J > FVP_MAX_JOINTS, V > FVP_MAX_VIEWS, L >
 * FVP_VIS_MAX_PRIMS.  Nothing is written when an error is returned.  B == 0 returns 0 without a launch.
 * One launch, no host synchronisation, no atomics: one workgroup per (b, n) with the frame's joints in LDS, one thread per
 * (v, j); the per-view results go through LDS and one thread per j sums the views in order.  Not built: occlusion by scene
 * objects, soft visibility, a per-view mask inside fvp_draw_poses / fvp_person_rois. */
int fvp_joint_visibility(const float* fused_poses /* [B][N][J][5] */, const float* cams /* [nsets][V][FVP_CAM_FLOATS] */,
                         const int32_t* frame_set /* [B] */, const int32_t* ids /* [B][N] or NULL */,
                         const float* views /* [B][V][N][J][4] of fvp_joint_evidence, or NULL */,
                         int B, int V, int N, int J,
                         const int32_t* prims /* HOST [L][2] */, const float* radius_mm /* HOST [L] */, int L,
                         float guard_mm, int Hs, int Ws,
                         int32_t* occluder /* [B][V][N][J] */, float* vis_conf /* [B][N][J] */,
                         int32_t* vis_count /* [B][N][J] */, fvp_stream_t s);

/* ---- triangulated joints from the views (ABI 18): a geometric second opinion per joint -------------------------------------
 * Everything behind fvp_fuse_poses takes the voxel network's 3-D joints as given.  This call answers, for every fused joint,
 * where the rays through the 2-D heat-map peaks of the usable views meet (independent of the fine grid's resolution, the
 * soft-argmax and WeightNet), how far each view's peak lies from the reprojection of that point (pixels of the original
 * image) and what that residual is per camera and frame - a camera that has been bumped stands apart from the others.
 *
 * heat_cl [B][V][H][W][JP], cams [nsets][V][FVP_CAM_FLOATS], frame_set [B] and g as for fvp_joint_evidence (V, J, JP, W, H
 * are g's); nsets is the number of camera sets in cams; fused_poses [B][N][J][5]; ids [B][N] int32 (fvp_track_update) or NULL;
 * occluder [B][V][N][J] int32 of fvp_joint_visibility or NULL.
 *
 * fp32 unless stated, every operation rounded on its own (no contraction) except the fmaf chains written as fma(); IEEE
 * division and square root;  dot(p,q) = (p0*q0 + p1*q1) + p2*q2;  clamp(x,lo,hi) = fminf(fmaxf(x,lo),hi);
 * a value is FINITE iff fabsf(x) <= FLT_MAX.  Person n of frame b is PRESENT iff fused_poses[b][n][0][3] >= 0 and (ids is
 * NULL or ids[b][n] >= 0).  Frame b is EVALUATED iff 0 <= frame_set[b] < nsets (the camera table is not read otherwise);
 * joint (b,n,j) is EVALUATED iff its frame is and its person is present.  Joints that are not evaluated: tri_count = -2,
 * view_state = 0, tri_poses = fused_poses, tri_stats = 0, obs = (0,0,0,-1).
 * On the host, once per call, in double from the fp32 fields of g, each result rounded to fp32 once (inv, passed by value):
 *     det = rt0*rt4 - rt1*rt3,  sx = img_w / hm_w,  sy = img_h / hm_h,
 *     inv0 = rt4/det*sx   inv1 = -rt1/det*sy   inv2 = (rt1*rt5 - rt4*rt2)/det
 *     inv3 = -rt3/det*sx  inv4 = rt0/det*sy    inv5 = (rt3*rt2 - rt0*rt5)/det            (left to right)
 * For an evaluated joint, P = fused_poses[b][n][j][0:3], and view v with camera record cm = cams[frame_set[b]][v]
 * (R row-major, T, f, c, k, p), r = radius:
 *   1. Window centre.  If P is not finite: state OUTSIDE.  (px, py, depth) = the camera model of fvp_joint_evidence
 *      (project_pixel, csrc/fvp_geom.h: d = P - T, xc = R d as fma chains, y = xc.xy / (xc.z + 1e-5f), the radial and
 *      tangential polynomial, px = f*u + c); depth = xc.z.  If not depth > 0: OUTSIDE.
 *        ax = fma(rt2, 1, fma(rt1, py, rt0*px)),  ay = fma(rt5, 1, fma(rt4, py, rt3*px)),
 *        hx = (ax*hm_w)/img_w,  hy = (ay*hm_h)/img_h                        (the heat-map cell coordinate, no clamp)
 *      If hx or hy is not finite: OUTSIDE.  cxf = floorf(hx + 0.5f), cyf likewise.  If not (-r <= cxf <= W-1+r and
 *      -r <= cyf <= H-1+r), compared as floats: OUTSIDE - the window holds no cell of the map.  Only then cx = int(cxf),
 *      cy = int(cyf).  A view that is OUTSIDE costs no load from heat_cl.
 *   2. Peak.  Candidates: the cells (x, y), |x-cx| <= r, |y-cy| <= r, 0 <= x < W, 0 <= y < H, of channel j, walked in
 *      ascending (y, x).  A NaN is no candidate; a candidate replaces the winner iff it is strictly larger: a tie stays with
 *      the smallest (y, x).  No candidate: PEAK_LOW, peak = 0.  Otherwise peak = the winner's value; if not peak >=
 *      min_peak: PEAK_LOW; else if x == cx-r or x == cx+r or y == cy-r or y == cy+r (the border of the unclipped window):
 *      NOT_ENCLOSED.
 *   3. Sub-cell refinement, per axis with the neighbours m (at -1), c = peak, p (at +1) along that axis, a neighbour
 *      outside the map being 0:  den = (2*c - m) - p,  delta = den > 0 ? clamp((0.5*(p - m))/den, -0.5, 0.5) : 0.
 *      qx = float(x) + delta_x,  qy = float(y) + delta_y.
 *   4. Back to the original image:  ox = fma(inv2, 1, fma(inv1, qy, inv0*qx)),  oy = fma(inv5, 1, fma(inv4, qy, inv3*qx)).
 *   5. Undistort.  u0 = (ox - c0)/f0, u1 = (oy - c1)/f1, y = u; then undistort_iters rounds, both components from the old y:
 *        rr = y0*y0 + y1*y1,  d = ((1 + k0*rr) + (k1*rr)*rr) + ((k2*rr)*rr)*rr,
 *        t0 = ((2*p0)*y0)*y1 + p1*(rr + (2*y0)*y0),  t1 = ((2*p1)*y0)*y1 + p0*(rr + (2*y1)*y1),
 *        y0 = (u0 - t0)/d,  y1 = (u1 - t1)/d.
 *      The fixed point reached from y = u is the small-radius root of the polynomial, the physical one where it folds.
 *   6. Ray.  g_k = (R[k]*y0 + R[3+k]*y1) + R[6+k], k = 0..2 (R transposed times (y0, y1, 1));  d = g / sqrtf(dot(g,g));
 *      origin C = T;  w = clamp(peak, 0, 1).  The view's state is USED - or OCCLUDED, if occluder is given and
 *      occluder[b][v][n][j] != -1.
 *   7. The usable views are those in state USED.  Fewer than min_views: tri_count = their number, not triangulated.  The
 *      usable views of a joint that is not triangulated (here or in step 8) end in state UNSOLVED.
 *   8. Solve, in fp64 (every fp32 input converted exactly, every operation rounded on its own), over the usable views in
 *      ascending v, all sums from 0:
 *        m00 = 1 - dx*dx, m11 = 1 - dy*dy, m22 = 1 - dz*dz, m01 = -(dx*dy), m02 = -(dx*dz), m12 = -(dy*dz)
 *        Aik = Aik + w*mik (six sums),  b0 = b0 + w*((m00*C0 + m01*C1) + m02*C2), b1 and b2 with rows (m01, m11, m12),
 *        (m02, m12, m22).
 *        k00 = A11*A22 - A12*A12   k01 = A02*A12 - A01*A22   k02 = A01*A12 - A02*A11
 *        k11 = A00*A22 - A02*A02   k12 = A01*A02 - A00*A12   k22 = A00*A11 - A01*A01
 *        det = (A00*k00 + A01*k01) + A02*k02,  t3 = ((A00 + A11) + A22)/3
 *      DEGENERATE iff not det > double(min_det)*((t3*t3)*t3) (a NaN fails): tri_count = -1, not triangulated.  Otherwise
 *        X0 = ((k00*b0 + k01*b1) + k02*b2)/det, X1 = ((k01*b0 + k11*b1) + k12*b2)/det, X2 = ((k02*b0 + k12*b1) + k22*b2)/det,
 *      each rounded to fp32 once.
 *   9. Residual of every view of the solve:  (qx, qy, .) = the camera model at X;  ex = qx - ox, ey = qy - oy,
 *      e_v = sqrtf(ex*ex + ey*ey).
 *  10. One rejection round, iff reject_px > 0: keep = the views of the solve with not e_v > reject_px.  Iff keep differs from
 *      the solve's views, holds at least min_views views and step 8 over keep is not degenerate, its X replaces the first,
 *      the dropped views get state REJECTED and e_v = -1, and step 9 is repeated over keep.  Otherwise the first solution,
 *      its residuals and states stand.  The round is not iterated.
 * Outputs; every element of a non-NULL output is written by every call; any may be NULL, not all of them; cam_resid and
 * cam_count are reduced from obs and view_state and need both:
 *     tri_poses  [B][N][J][5]    xyz = X where triangulated, else P; elements 3 and 4 copied from fused_poses: the tensor
 *                                drops in wherever fused_poses goes (tracker, smoother, overlay, evidence);
 *     tri_count  [B][N][J] int32 the views of the final solve (>= min_views); 0..min_views-1: that many usable views, not
 *                                triangulated; -1 degenerate; -2 not evaluated;
 *     tri_stats  [B][N][J][2]    shift_mm = sqrtf(dot(X - P, X - P)),  rms_px = sqrtf(num/den) with num = num + w*(e_v*e_v),
 *                                den = den + w over the views of the final solve in ascending v; (0, 0) when not triangulated;
 *     obs        [B][V][N][J][4] (ox, oy, peak, e_v); e_v = -1 unless the state is USED; ox = oy = 0 in the states
 *                                NOT_EVALUATED, OUTSIDE, PEAK_LOW and NOT_ENCLOSED, peak = 0 in the first two (and where
 *                                every candidate is a NaN);
 *     view_state [B][V][N][J] int32  FVP_TRI_USED ... FVP_TRI_UNSOLVED above;
 *     cam_resid  [B][V] fp32, cam_count [B][V] int32: the mean e_v and the number of USED joint-views of view v in frame b.
 *                                With q = n*J + j: thread t of 256 adds the used entries q = t, t+256, ... in ascending
 *                                order from 0, then the 256 partial sums fold as s[t] = s[t] + s[t+h] for h = 128, 64, ..., 1;
 *                                cam_resid = s[0]/float(count), 0 when the count is 0.  No dependence on scheduling.
 * FVP_EINVAL: a null heat_cl, cams, frame_set, fused_poses or g; all outputs null; cam_resid or cam_count without obs and
 * view_state; B < 0; N or nsets < 1; radius < 1; min_views < 2; undistort_iters < 0; min_peak, min_det or reject_px not finite;
 * g's JP, W or H invalid; an rt that cannot be inverted.  FVP_ELIMIT: J > FVP_MAX_JOINTS, V > FVP_MAX_VIEWS, radius >
 * FVP_TRI_MAX_RADIUS, undistort_iters > 16.  Nothing is written when an error is returned.  B == 0 returns 0 without a launch.
 * One launch (two with cam_resid / cam_count), no host synchronisation, no atomics: one workgroup per (b, n), the camera
 * records in LDS, one thread per (v, j) for steps 1-6, one thread per j for steps 7-10.
 * Suggested parameters - guesses, not tuned on real data: radius 3, min_peak 0.3, undistort_iters 8, min_views 2,
 * min_det 1e-3, reject_px 0 (off).  Re-calibration: fvp_camera_refit_* below.  Not built: an iterated rejection, triangulated
 * poses fed into tracker or smoother by default. */
int fvp_triangulate_joints(const float* heat_cl /* [B][V][H][W][JP] */, const float* cams /* [nsets][V][FVP_CAM_FLOATS] */,
                           int nsets, const int32_t* frame_set /* [B] */, const float* fused_poses /* [B][N][J][5] */,
                           const int32_t* ids /* [B][N] or NULL */, const int32_t* occluder /* [B][V][N][J] or NULL */,
                           int B, int N, const FvpGeom* g,
                           int radius, float min_peak, int undistort_iters, int min_views, float min_det, float reject_px,
                           float* tri_poses /* [B][N][J][5] */, int32_t* tri_count /* [B][N][J] */,
                           float* tri_stats /* [B][N][J][2] */, float* obs /* [B][V][N][J][4] */,
                           int32_t* view_state /* [B][V][N][J] */, float* cam_resid /* [B][V] */,
                           int32_t* cam_count /* [B][V] */, fvp_stream_t s);

/* ---- bumped cameras re-fitted on the device (ABI 19): fvp_camera_refit_accumulate + fvp_camera_refit_solve ------------------
 * fvp_triangulate_joints shows that a camera has moved (cam_resid); these two calls correct it.  A robust RESECTION of every
 * camera against the 3-D joints: one Gauss-Newton step on the camera's six extrinsic parameters, the observations
 * accumulated over as many batches as the caller likes, the step solved on the device, the result a camera record in the
 * layout every projection call reads.  The 3-D points are held fixed - that is what pulls one bumped camera back to the
 * consensus of the others; this is not bundle adjustment, and when every camera is re-fitted at once nothing fixes the gauge.
 *
 * ALL ARITHMETIC IS fp64 unless stated; every fp32 input is converted exactly; every operation is rounded on its own (no
 * contraction); division and sqrt are IEEE; no transcendental function is used anywhere (a numpy restatement reproduces every
 * output bit for bit: tests/recalibrate_cases.py).  dot(p,q) = (p0*q0 + p1*q1) + p2*q2.
 *
 * 1. fvp_camera_refit_accumulate.  points [B][N][J][5] is fused_poses or tri_poses, the caller's choice (elements 0..2 are
 * read); obs [B][V][N][J][4] and view_state [B][V][N][J] as fvp_triangulate_joints wrote them for the same batch; cams
 * [nsets][V][FVP_CAM_FLOATS]; frame_set [B].  acc [nsets][V][FVP_CAL_ACC] doubles is caller-owned state (as the tracker's);
 * its initial state is all zeros:
 *     0..20  the upper triangle of H, row-major (00, 01, ..., 05, 11, ..., 55)      21..26  g
 *     27  sum of ww      28  sum of ww*e2      29  the number of observations (an exact integer in a double)
 *     30  the number of observations with h < 1      31  0
 * Observation (b,v,n,j) COUNTS for camera (s, v), s = frame_set[b], iff 0 <= s < nsets, view_state == FVP_TRI_USED,
 * X = points[b][n][j][0:3] is finite (fabsf(x) <= FLT_MAX), ox, oy = obs[..][0:2] are finite, wf = fminf(fmaxf(obs[..][2],
 * 0), 1) > 0 (fp32), and z > 1.0 below (the point lies more than 1 mm in front of the camera).  A NaN fails every one.
 * For a counting observation, cm = cams[s][v] (R row-major, T, f, c, k, p):
 *     (y0, y1) = step 5 of fvp_triangulate_joints at (ox, oy) with undistort_iters rounds, in fp32 (the same device function);
 *     d = X - T;  xc_k = (R[3k]*d0 + R[3k+1]*d1) + R[3k+2]*d2;  z = xc_2;  iz = 1/z;  u = xc_0/z;  v = xc_1/z;
 *     r0 = (y0 - u)*f0;  r1 = (y1 - v)*f1                         (pixels of the undistorted image)
 *     the Jacobian of the prediction by (w, t) of the perturbation xc' = C(w) xc + t, at zero:
 *     Ju = (f0*(-(u*v)), f0*(1 + u*u), f0*(-v), f0*iz, 0, f0*(-(u*iz)))
 *     Jv = (f1*(-(1 + v*v)), f1*(u*v), f1*u, 0, f1*iz, f1*(-(v*iz)))
 *     e2 = r0*r0 + r1*r1;  e = sqrt(e2);  h = (huber_px > 0 and e > huber_px) ? huber_px/e : 1;  ww = wf*h;
 *     H_ik = H_ik + ww*((Ju_i*Ju_k) + (Jv_i*Jv_k)), i <= k;  g_i = g_i + ww*((Ju_i*r0) + (Jv_i*r1));
 *     elements 27..30 = themselves + ww, + ww*e2, + 1, + (h < 1 ? 1 : 0).
 * The reduction is fixed and independent of scheduling: one workgroup of 256 threads per (s, v); with q = (b*N + n)*J + j
 * over the whole batch, thread t adds its counting entries q = t, t+256, ... in ascending order, all 31 sums from 0; the 256
 * partial vectors fold as p[t] = p[t] + p[t+h] for h = 128, 64, ..., 1; then acc[s][v][i] = acc[s][v][i]*double(decay) +
 * p[0][i] for i < 31, and element 31 is written as 0.  decay = 1 accumulates, 0 < decay < 1 forgets, 0 replaces (the old
 * content must be finite: NaN*0 is NaN).  Every camera of the table is updated by every call (a camera without a counting
 * observation decays).  The accumulators are a linearisation AT cams: after a camera's record changes, its row of acc must
 * be zeroed by the caller before the next accumulation.
 * FVP_EINVAL: a null pointer; B < 0; V, N, J or nsets < 1; undistort_iters < 0; huber_px not finite; decay not in [0, 1].
 * FVP_ELIMIT: V > FVP_MAX_VIEWS, J > FVP_MAX_JOINTS, undistort_iters > 16, B*N*J > INT_MAX.  B == 0 returns 0 without a
 * launch (acc does not decay).  One launch, no atomics.
 *
 * 2. fvp_camera_refit_solve, one thread per camera (s, v), a = acc[s][v], cm = cams_in[s][v]; lambda, min_pivot,
 * max_angle_rad and max_shift_mm converted to double:
 *     count = a[29].  Not count >= min_obs: state FVP_CAL_FEW.
 *     D_i = sqrt(H_ii).  Any H_ii not > 0: FVP_CAL_DEGENERATE.
 *     A_ik = H_ik/(D_i*D_k), and A_ii = H_ii/(D_i*D_i) + lambda         (Jacobi scaling: radians against millimetres put
 *     the unscaled matrix at a condition of ~1e9).
 *     Cholesky A = L L^T column by column, j = 0..5, every sum left to right in ascending k:
 *         piv_j = A_jj - L_j0*L_j0 - ... - L_j,j-1*L_j,j-1;  L_jj = sqrt(piv_j);
 *         L_ij = (A_ij - L_i0*L_j0 - ... - L_i,j-1*L_j,j-1)/L_jj, i = j+1..5.
 *     Any piv_j not > min_pivot (a NaN fails): DEGENERATE.  The threshold is unit-free because of the scaling.
 *     minpiv: from piv_0, replaced by piv_j iff piv_j < minpiv, j ascending.
 *     Forward  y_i = (g_i/D_i - L_i0*y_0 - ... - L_i,i-1*y_i-1)/L_ii, i = 0..5;
 *     back     zeta_i = (y_i - L_i+1,i*zeta_i+1 - ... - L_5,i*zeta_5)/L_ii, i = 5..0;   delta_i = zeta_i/D_i;
 *     w = delta[0:3] (radians), t = delta[3:6] (mm);  theta = sqrt(dot(w,w)), sigma = sqrt(dot(t,t)).
 *     theta or sigma not finite (not <= DBL_MAX): DEGENERATE.
 *     gd = ((((g0*delta0 + g1*delta1) + g2*delta2) + g3*delta3) + g4*delta4) + g5*delta5      (before the clamp)
 *     Trust region: kappa = 1;  if theta > max_angle_rad: kappa = max_angle_rad/theta;  if sigma > max_shift_mm and
 *     max_shift_mm/sigma < kappa: kappa = max_shift_mm/sigma.  If kappa < 1: delta_i = delta_i*kappa, theta and sigma are
 *     computed again from it, state FVP_CAL_CLAMPED; else FVP_CAL_OK.
 *     Cayley retraction: h = 0.5*w;  n = sqrt(1 + dot(h,h));  qw = 1/n, qx = h0/n, qy = h1/n, qz = h2/n;
 *         C00 = 1 - 2*(qy*qy + qz*qz)   C01 = 2*(qx*qy - qz*qw)       C02 = 2*(qx*qz + qy*qw)
 *         C10 = 2*(qx*qy + qz*qw)       C11 = 1 - 2*(qx*qx + qz*qz)   C12 = 2*(qy*qz - qx*qw)
 *         C20 = 2*(qx*qz - qy*qw)       C21 = 2*(qy*qz + qx*qw)       C22 = 1 - 2*(qx*qx + qy*qy)
 *     R'_ik = (C_i0*R_0k + C_i1*R_1k) + C_i2*R_2k;   T'_k = T_k - ((R'_0k*t0 + R'_1k*t1) + R'_2k*t2)   (R' before its rounding);
 *     R' and T' are each rounded to fp32 once; the other 12 floats of the record are copied.
 * cams_out [nsets][V][FVP_CAM_FLOATS] (must not be cams_in): in the states FEW and DEGENERATE a copy of the cams_in record.
 * cal_stats [nsets][V][6] fp32 or NULL: (theta, sigma - after the clamp -, rms_before = sqrt(a[28]/a[27]), rms_pred =
 * sqrt(max(0, a[28] - gd)/a[27]), count, minpiv), each rounded to fp32 once; max(0, x) = x > 0 ? x : 0.  In the states FEW and
 * DEGENERATE: (0, 0, rms_before, 0, count, 0); rms_before and rms_pred are 0 unless a[27] > 0.  rms_pred is the residual the
 * linear model expects after the step; it is exact only for lambda = 0 and kappa = 1.
 * cal_state [nsets][V] int32 or NULL: FVP_CAL_OK, FVP_CAL_CLAMPED, FVP_CAL_FEW, FVP_CAL_DEGENERATE.
 * FVP_EINVAL: a null acc, cams_in or cams_out; cams_out == cams_in; nsets or V < 1; min_obs < 6; lambda not >= 0 or not
 * finite; min_pivot, max_angle_rad or max_shift_mm not > 0 or not finite.  FVP_ELIMIT: V > FVP_MAX_VIEWS.
 * Both calls: every pointer is a device pointer, nothing is allocated, no host synchronisation, capturable; nothing is
 * written when an error is returned.  One Gauss-Newton round is accumulate + solve; for another round zero acc and
 * accumulate against cams_out (obs are pixels and do not depend on the camera table).
 * Suggested parameters - guesses, not tuned on real data: undistort_iters 8, huber_px 0 (off), decay 1, min_obs 60,
 * lambda 0, min_pivot 1e-9, max_angle_rad 0.087 (5 degrees), max_shift_mm 200.  Not built: intrinsics or lens re-fit, joint
 * refinement of points and cameras (bundle adjustment), gauge fixing when every camera is re-fitted at once, automatic
 * adoption of the corrected cameras into an engine. */
int fvp_camera_refit_accumulate(const float* points /* [B][N][J][5] */, const float* obs /* [B][V][N][J][4] */,
                                const int32_t* view_state /* [B][V][N][J] */,
                                const float* cams /* [nsets][V][FVP_CAM_FLOATS] */, int nsets,
                                const int32_t* frame_set /* [B] */, int B, int V, int N, int J, int undistort_iters,
                                float huber_px, float decay, double* acc /* [nsets][V][FVP_CAL_ACC] in/out */,
                                fvp_stream_t s);
int fvp_camera_refit_solve(const double* acc /* [nsets][V][FVP_CAL_ACC] */,
                           const float* cams_in /* [nsets][V][FVP_CAM_FLOATS] */, int nsets, int V, int min_obs,
                           float lambda, float min_pivot, float max_angle_rad, float max_shift_mm,
                           float* cams_out /* [nsets][V][FVP_CAM_FLOATS], not cams_in */,
                           float* cal_stats /* [nsets][V][6] or NULL */, int32_t* cal_state /* [nsets][V] or NULL */,
                           fvp_stream_t s);

/* ---- "next" row f-1: Pose-ResNet backbone in bf16 (lib/models/resnet.py:98-215) ------------------------
 * Activations are NHWC bf16 (uint16 storage; the image input is padded to 8 channels), every conv /
 * ConvTranspose(k4,s2,p1) is an implicit GEMM on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, eval
 * BatchNorm folded into a per-cout scale / shift, residual add and ReLU in the epilogue.  The op flagged
 * FVP_BB_OUT_HEAT (final_layer) writes fp32 heatmaps: channels-last [N][H*W][heat_jp] (what the projection
 * kernels read) and / or NCHW [N][J][H][W] (the reference's layout). */
enum { FVP_BB_CONV = 0, FVP_BB_MAXPOOL = 1, FVP_BB_DECONV = 2 };
enum { FVP_BB_OUT_HEAT = 8,      /* with FVP_EPI_RELU = 1 in `flags` */
       FVP_BB_STEM = 16,         /* the 7x7 / stride-2 stem on a <= 4-channel image: pixel-pair form (fvp_backbone.hip) */
       FVP_BB_CFG_SHIFT = 8 };   /* flags bits 8-9: tile configuration chosen by fvp_bb_tune (0 = built-in heuristic) */
typedef struct FvpBbOp {
  int32_t kind;
  int32_t src, dst, res;      /* activation buffer ids (dst = -1 for the heatmap op, res = -1 if unused) */
  int32_t cin, cinp;          /* true / stored input channels (cinp: power of two >= 8)                 */
  int32_t cout, coutp, cbuf;  /* true couts, couts of the packed weights (multiple of 64), channels of dst */
  int32_t kh, kw, stride, pad;
  int32_t h, w, oh, ow;       /* input and output spatial size                                          */
  int32_t flags;
  int32_t w_off;              /* bf16 element offset of the packed weights in wblob                     */
  int32_t e_off;              /* float offset of scale | shift (2 * coutp) in eblob                      */
} FvpBbOp;
/* images [N][C<=4][H][W] fp32 (W even) -> NHWC bf16 with 4 channels per pixel = [N][H][W/2][8] pixel pairs */
int fvp_bb_input(const float* images, uint16_t* nhwc8, int N, int C, int H, int W, fvp_stream_t s);
/* state_dict tensors of one conv (+ its BatchNorm, may be NULL) -> packed bf16 weights [cls][coutp][taps*cinp]
 * and fp32 scale | shift (resnet.py conv / bn / deconv / final_layer modules) */
int fvp_bb_pack(const float* weight, const float* bias, const float* bn_gamma, const float* bn_beta,
                const float* bn_mean, const float* bn_var, float eps, const FvpBbOp* op, uint16_t* wblob,
                float* eblob, fvp_stream_t s);
/* run the op list on N images; bufs[i] = NHWC bf16 activation buffer i.  The first 64 floats of eblob must be
 * zero (e_off >= 64): the LDS-DMA of the large-tile kernel reads them for padding.
 * Op patterns the list holds in sequence run as ONE kernel each, with the bits of the op-by-op launches (ABI 8):
 * stem conv (+ bn, ReLU) followed by its max-pool (resnet.py:103-106, :185-188), and a 64-plane bottleneck
 * [1x1 downsample,] 1x1 -> 3x3 -> 1x1 + residual (resnet.py:57-95) on one map - provided nothing else in the list
 * reads the intermediate buffers, which then stay unwritten.  The 1x1 heatmap layer behind the last transposed
 * conv is applied in that conv's epilogue. */
int fvp_bb_run(const FvpBbOp* ops, int nops, const uint16_t* wblob, const float* eblob, void* const* bufs, int nbufs,
               int N, float* heat_cl, int heat_jp, float* heat_nchw, fvp_stream_t s);
/* optional, once per (op list, N): times every conv op with each tile configuration of the large-tile kernel and
 * records the fastest in its flags (the configurations compute identical bits).  Synchronises `s`; the activation
 * buffers are used as scratch. */
int fvp_bb_tune(FvpBbOp* ops, int nops, const uint16_t* wblob, const float* eblob, void* const* bufs, int nbufs, int N,
                fvp_stream_t s);

/* ---- measurement hooks (bench.py roofline leg) -----------------------------------------------------
 * fvp_prof_enable(1): kernel classes are bracketed by hipEvents on the stream they are launched
 * on -- per launch for the projection / soft-argmax / small kernels, one pair per
 * fvp_conv_stack_run for the conv class (launches = convs in the stack), so that a ~100-launch
 * step is not perturbed.  fvp_prof_enable(2): one pair per conv LAUNCH instead, the Winograd 3x3
 * launches (the dominant kernel) in their own class FVP_K_CONV_WINO, all others in FVP_K_CONV.  Winograd launches with
 * fewer work units than the chip has workgroup slots (CenterNet's levels since round 6, everything at B = 1) are
 * launch-latency-bound, not matrix-core-bound: they go to FVP_K_CONV_WINO_SMALL so that the roofline of the
 * chip-filling launches stays what it describes.
 * fvp_prof_read synchronises the events and returns accumulated milliseconds, launch count and
 * algorithmic FLOPs since the last reset. */
enum { FVP_K_PROJECT_WHOLE = 0, FVP_K_PROJECT_TRIPLANE = 1, FVP_K_CONV = 2, FVP_K_SOFTARGMAX = 3,
       FVP_K_OTHER = 4, FVP_K_CONV_WINO = 5, FVP_K_BACKBONE = 6, FVP_K_CONV_WINO_SMALL = 7, FVP_K_COUNT = 8 };
int fvp_prof_enable(int on);
int fvp_prof_read(int cls, double* ms, int64_t* launches, double* flops);
int fvp_prof_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* FVP_H_ */
