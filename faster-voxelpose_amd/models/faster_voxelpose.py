"""Top module -- drop-in for the reference's ``lib/models/faster_voxelpose.py``
(``FasterVoxelPoseNet`` :18-105, ``get`` :108), inference branch.

``forward(backbone=None, views=None, meta=None, targets=None, input_heatmaps=None,
cameras=None, resize_transform=None)`` returns
``(fused_poses [B,N,J,5], plane_poses [3,B,N,J,2], proposal_centers [B,N,7], input_heatmaps, None)``.

Beyond the reference: ``model.evidence = True`` makes ``forward`` also leave ``model.last_evidence = (views [B,V,N,J,4],
joint_conf [B,N,J])`` - every fused joint reprojected into every camera image with its heatmap support there, and the
per-joint confidence the model itself defines (``FasterVoxelPoseNet.joint_evidence``) - and a stage object assigned to one of
the attributes of ``STAGES`` makes it also run that stage behind its own poses.  Every stage is static-shape and free of host
synchronisation like the rest of the forward, so under ``GraphedForward`` / ``GraphedPipeline`` its launches are part of the
captured graph and its ``last_*`` holds static tensors, overwritten by the next replay; the returned tuple is the same with
and without it, and unset (None) the forward issues exactly the launches it issues without the feature.
"""
import collections
import time

import torch
import torch.nn as nn

from .. import _capi as capi
from ..dataset.images import BayerFrames, Nv12Frames, demosaic_bayer, ingest_bayer, ingest_frames, ingest_nv12
from ..engine import HotPath
from .human_detection_net import HumanDetectionNet
from .joint_localization_net import JointLocalizationNet

# One row per optional stage of the forward, in the order in which PipelinedForward refuses them.  ``attr``: the model
# attribute that holds the stage object; ``last``: the attribute the forward leaves its result in; ``needs``: what else has
# to be set, each with the reason the error message gives - "evidence" (model.evidence = True), "tracker", "triangulator",
# "frames" (camera frames as ``views``: uint8 [B,V,Hs,Ws,3] or Nv12Frames); ``about``: what the forward does with it;
# ``recipe``: what to do instead on the consumer stream of a pipeline, which takes no stage.  The calls themselves are
# FasterVoxelPoseNet._run_stages.
Stage = collections.namedtuple("Stage", "attr last needs about recipe")
STAGES = (
    Stage("tracker", "last_tracks", {},
          "a core.tracking.PoseTracker: tracker.update() on the fused poses (one more launch, frames in batch order, the "
          "frames' sequence rows are the engine's own) leaves (ids [B,N], slots [B,N], costs [B,N]): one identity per person "
          "across the frames of a camera sequence.  The track state lives in device memory and carries from call to call, "
          "and from replay to replay of a captured graph.",
          "call tracker.update(outputs[0], meta) on the consumer stream in submit order"),
    Stage("smoother", "last_smooth", {"tracker": "filters the tracks of model.tracker"},
          "a core.smoothing.PoseSmoother: smoother.update() behind the tracker's, on last_tracks and the stages' joint_conf "
          "(one more launch), leaves (smooth [B,N,J,5], track_poses [B,T,J,4], track_state [B,T,2]): the One-Euro-filtered "
          "pose of every track, slot-stable, unsupported joints and dropped-out tracks bridged by prediction.",
          "call smoother.update(outputs[0], ids, slots, meta=meta) behind tracker.update on the consumer stream in submit "
          "order"),
    Stage("overlay", "last_overlay_views", {"evidence": "draws the pixels of model.last_evidence",
                                            "frames": "draws into the camera frames"},
          "a utils.overlay.PoseOverlay: draws the skeletons into the caller's frames, in place, behind tracker, smoother and "
          "crops (one more launch) - from last_evidence[0], or, with a smoother, from one more joint_evidence() of "
          "last_smooth[0] kept in last_overlay_views (issued once for crops and overlay) - coloured by last_tracks[0], gated "
          "by the stages' joint_conf.  Nv12Frames views are drawn on, in the surface itself, only by an overlay built with "
          "nv12=True: the surface is the decoder's own memory.",
          "call overlay.draw(frames, views, ids) on the consumer stream"),
    Stage("crops", "last_crops", {"evidence": "cuts around the pixels of model.last_evidence",
                                  "frames": "cuts the patches out of the camera frames"},
          "a utils.crops.PersonCrops: cuts a normalised, fixed-size patch per (frame, view, person) out of the caller's "
          "frames before the overlay paints them (two more launches) - boxes around the pixels the overlay would draw, "
          "last_tracks[0] as ids, the stages' joint_conf - and leaves (patches [B,V,N,3,h,w], rois [B,V,N,4], count [B,V,N], "
          "score [B,V,N]).",
          "call crops(frames, views, ids) on the consumer stream, with views from model.joint_evidence(outputs[0], ...)[0], "
          "before any overlay.draw"),
    Stage("visibility", "last_visibility", {"evidence": "judges the pixels of model.last_evidence"},
          "a utils.visibility.JointVisibility: tests every fused joint's line of sight to every camera against the other "
          "people's bodies, right behind the evidence launch (one more launch, on last_evidence[0] and the engine's camera "
          "tables), and leaves (occluder [B,V,N,J], vis_conf [B,N,J], vis_count [B,N,J]).  Built with feeds_conf=True (the "
          "default), vis_conf takes the place of last_evidence[1] as the joint_conf of smoother, overlay and crops.",
          "call visibility(outputs[0], cameras, meta, views=views) on the consumer stream, with views from "
          "model.joint_evidence(outputs[0], ...)[0]"),
    Stage("recalibrator", None, {"triangulator": "reads the triangulation's obs and view_state"},
          "a utils.recalibrate.CameraRefiner: adds this batch's observations to recalibrator.acc, one launch right behind "
          "the triangulation's, on last_triangulation and the engine's camera tables; model.recalibrator_points: 'fused' "
          "(the forward's joints) or 'tri' (the triangulated ones) as the 3-D points.  Solving and adopting stay with the "
          "caller (recalibrator.solve(model.engine.geo.cams), camera_dicts): the engine's tables are never swapped here.",
          "call recalibrator.accumulate(outputs[0], obs, view_state, cams, frame_set) behind the triangulator on the "
          "consumer stream"),
    Stage("triangulator", "last_triangulation", {},
          "a utils.triangulate.JointTriangulator: triangulates every fused joint from the heat-map peaks of the views, "
          "behind the evidence and visibility launches (one or two more launches, on the staging copy of this forward and "
          "the engine's camera tables, last_visibility[0] as the occluder table), and leaves (tri_poses [B,N,J,5], tri_count "
          "[B,N,J], tri_stats [B,N,J,2], obs [B,V,N,J,4], view_state [B,V,N,J], cam_resid [B,V], cam_count [B,V]).  The poses "
          "handed to tracker, smoother, overlay and crops stay the fused ones.",
          "call triangulator(outputs[0], cameras, meta, heat_cl) on the consumer stream, with heat_cl from "
          "model.engine.heat_cl(outputs[3], geom)"),
)
_STAGE = {s.attr: s for s in STAGES}
_CHECKED_FIRST = ("smoother", "visibility", "overlay", "crops")    # forward() checks their needs before any launch, in this order
_REMEDY = {"tracker": "set model.tracker (a PoseTracker) too", "evidence": "set model.evidence = True too",
           "triangulator": "set model.triangulator = JointTriangulator(cfg) as well",
           "frames": "pass them as views, uint8 [B,V,Hs,Ws,3] or Nv12Frames (float images and input_heatmaps alone leave "
                     "nothing to work on; an overlay takes Nv12Frames only when built with nv12=True)",
           "bayer_rgb": "set model.bayer_rgb = True (BayerFrames views hold no RGB frame: with it the forward demosaics "
                        "them once into model.last_frames, uint8 [B,V,Hs,Ws,3] in R, G, B order, and works on that)"}


class FasterVoxelPoseNet(nn.Module):
    def __init__(self, cfg, _lib=None):
        super().__init__()
        self.cfg = cfg
        self.max_people = cfg.CAPTURE_SPEC.MAX_PEOPLE
        self.num_joints = cfg.DATASET.NUM_JOINTS
        self.device = torch.device(cfg.DEVICE)
        self.engine = HotPath(cfg, _lib=_lib)
        self.pose_net = HumanDetectionNet(cfg, _engine=self.engine)
        self.joint_net = JointLocalizationNet(cfg, _engine=self.engine)
        self.lambda_loss_2d = cfg.TRAIN.LAMBDA_LOSS_2D
        self.lambda_loss_1d = cfg.TRAIN.LAMBDA_LOSS_1D
        self.lambda_loss_bbox = cfg.TRAIN.LAMBDA_LOSS_BBOX
        self.lambda_loss_fused = cfg.TRAIN.LAMBDA_LOSS_FUSED
        # True: forward() also evaluates joint_evidence() on its own poses (one more launch) and keeps the pair in
        # `last_evidence`; the returned tuple is the same either way
        self.evidence = False
        self.last_evidence = None
        # BayerFrames views (dataset/images.py).  False: fvp_ingest_bayer feeds the backbone and no RGB frame exists, so a
        # stage that needs frames is refused.  True: the forward demosaics once into `last_frames` (uint8 [B,V,Hs,Ws,3], R, G,
        # B), ingests that - the same bits - and hands it to overlay and crops; PersonReId, LimbModel and FaceAnonymiser take
        # it from there
        self.bayer_rgb = False
        self.last_frames = None
        for stage in STAGES:                             # every optional stage unset (STAGES says what each does when set)
            setattr(self, stage.attr, None)
            if stage.last is not None:
                setattr(self, stage.last, None)
        self.recalibrator_points = "fused"
        self.eval()

    def joint_evidence(self, fused_poses, input_heatmaps, meta, cameras, resize_transform):
        """Per-joint, per-view evidence for ANY poses in the layout of ``fused_poses`` [B,N,J,5] (the model's own, a
        tracker's smoothed ones, ground truth) against ``input_heatmaps`` [B,V,J,H,W]:

        ``views`` [B,V,N,J,4] = (px, py, depth, s): the joint's distorted pixel in the original image of camera v (before
        any clamp; it may lie outside the image), its camera-space depth (<= 0: behind the camera), and the bilinear
        sample s of the joint's own heatmap of that view at the position the projection layers sample;
        ``joint_conf`` [B,N,J] = clamp(mean over views of s, 0, 1): the value the reference's whole-space projection
        (project_whole.py:83,86) puts into a voxel centred on the joint, bit for bit.

        Slots with ``fused_poses[b,n,0,3] < 0`` are all zero.  One static-shape launch on the current stream, no host
        synchronisation."""
        return self.engine.joint_evidence(fused_poses, input_heatmaps, meta, cameras, resize_transform)

    def _check_needs(self, stage, views):
        """FvpError unless everything ``stage`` (a row of STAGES, set on this model) needs is there as well."""
        for need, why in stage.needs.items():
            if need == "evidence":
                ok = self.evidence
            elif need == "frames":
                # an NV12 surface is the decoder's own memory: drawn on only by an overlay built with nv12=True
                if isinstance(views, BayerFrames):        # a sensor's mosaic: the stage works on the demosaiced frames
                    if not self.bayer_rgb:
                        raise capi.FvpError(f"model.{stage.attr} {why}: {_REMEDY['bayer_rgb']}")
                    continue
                ok = getattr(getattr(self, stage.attr), "nv12", True) if isinstance(views, Nv12Frames) \
                    else torch.is_tensor(views) and views.dtype == torch.uint8
            else:
                ok = getattr(self, need) is not None
            if not ok:
                raise capi.FvpError(f"model.{stage.attr} {why}: {_REMEDY[need]}")

    def _heatmaps_from_views(self, backbone, views, resize_transform, swap_rb=None):
        """``views`` - fp32 images [B,V,3,H,W], uint8 camera frames [B,V,Hs,Ws,3] (BGR unless ``swap_rb`` is False), or an
        ``Nv12Frames`` / ``BayerFrames`` with leading dimensions [B,V] (dataset/images.py) - through ``backbone`` ->
        ``input_heatmaps`` [B,V,J,H/4,W/4]."""
        nv12 = isinstance(views, Nv12Frames)              # a decoder's NV12 surface
        bayer = isinstance(views, BayerFrames)            # a sensor's Bayer mosaic (model.bayer_rgb False: no RGB frame)
        frames = not (nv12 or bayer) and views.dtype == torch.uint8  # raw camera frames
        if nv12:
            if len(views.lead) != 2:
                raise capi.FvpError(f"NV12 views must have leading dimensions [B,V], got {views.lead}")
            if resize_transform is None:
                raise capi.FvpError("NV12 views need resize_transform (camera -> network pixels) to be resized")
            B, V = views.lead
        elif bayer:
            B, V = views.lead
        else:
            if frames:
                if views.dim() != 5 or views.shape[-1] != 3:
                    raise capi.FvpError(f"uint8 views must be camera frames [B,V,Hs,Ws,3] (HWC), got {tuple(views.shape)}")
                if resize_transform is None:
                    raise capi.FvpError("uint8 views need resize_transform (camera -> network pixels) to be resized")
            B, V = views.shape[:2]
        if hasattr(backbone, "_run"):
            # bf16 HIP backbone (models/resnet.py): all B*V views in one pass - frames and surfaces through the ingest kernel
            # straight into its bf16 input, no RGB frame and no fp32 image in between; it writes the heatmaps as NCHW
            # (returned, like the reference) and in the channels-last layout the projection reads
            if frames and swap_rb is not None:
                nchw, cl = backbone._run(views.flatten(0, 1), True, True, resize_transform=resize_transform, swap_rb=swap_rb)
            else:
                nchw, cl = backbone._run(views if nv12 or bayer else views.flatten(0, 1), True, True,
                                         resize_transform=resize_transform if nv12 or bayer or frames else None)
            input_heatmaps = nchw.view(B, V, *nchw.shape[1:])
            if cl.shape[-1] == self.engine.JP:
                self.engine.adopt_staging(input_heatmaps, cl)
            return input_heatmaps
        # any torch module: the fp32 tensor the reference's loader would have produced, then per-view passes (:36-38)
        if nv12:
            views = ingest_nv12(views, resize_transform, self.cfg.DATASET.IMAGE_SIZE, _lib=self.engine.lib)
        elif bayer:
            views = ingest_bayer(views, resize_transform, self.cfg.DATASET.IMAGE_SIZE, _lib=self.engine.lib)
        elif frames:
            views = ingest_frames(views, resize_transform, self.cfg.DATASET.IMAGE_SIZE, swap_rb=swap_rb is None or swap_rb,
                                  _lib=self.engine.lib)
        return torch.stack([backbone(views[:, c]) for c in range(V)], dim=1)

    def forward(self, backbone=None, views=None, meta=None, targets=None, input_heatmaps=None, cameras=None,
                resize_transform=None):
        if self.training:
            raise NotImplementedError("only the inference branch of FasterVoxelPoseNet.forward is implemented "
                                      "(call model.eval()); training losses are outside the hot path")
        for attr in _CHECKED_FIRST:
            if getattr(self, attr) is not None:
                self._check_needs(_STAGE[attr], views)
        if isinstance(views, BayerFrames):
            if len(views.lead) != 2:
                raise capi.FvpError(f"Bayer views must have leading dimensions [B,V], got {views.lead}")
            if resize_transform is None:
                raise capi.FvpError("Bayer views need resize_transform (camera -> network pixels) to be resized")
        if isinstance(views, BayerFrames) and self.bayer_rgb:
            # one demosaic into last_frames; from here on the views ARE that RGB frame (include/fvp.h: ingesting it gives the
            # bits fvp_ingest_bayer gives), for the ingest and for overlay and crops
            views = self.last_frames = demosaic_bayer(views, _lib=self.engine.lib)
            input_heatmaps = self._heatmaps_from_views(backbone, views, resize_transform, swap_rb=False)
        elif views is not None:
            input_heatmaps = self._heatmaps_from_views(backbone, views, resize_transform)
        _, _, proposal_centers, _ = self.pose_net(input_heatmaps, meta, cameras, resize_transform)
        mask = self.engine.last["valid"]              # uint8 [B,N] = proposal_centers[:, :, 3] >= 0 (:45), written by fvp_proposals
        fused_poses, plane_poses = self.joint_net.forward5(meta, input_heatmaps, proposal_centers, mask, cameras,
                                                           resize_transform, _reuse_staging=True)
        self._run_stages(views, fused_poses, input_heatmaps, meta, cameras, resize_transform)
        # the channels-last staging copy is valid for this call only: a later tensor may reuse the
        # same address / version / shape once the caching allocator recycles the block
        self.engine.invalidate_staging()
        return fused_poses, plane_poses, proposal_centers, input_heatmaps, None

    def _run_stages(self, views, fused_poses, input_heatmaps, meta, cameras, resize_transform):
        """Evidence and the optional stages (STAGES) behind the fused poses, each one only when set: evidence, visibility,
        triangulator, recalibrator, tracker, smoother, the evidence of the smoothed poses, crops, overlay."""
        eng, V = self.engine, input_heatmaps.shape[1]
        rows = []

        def frame_set():
            # the frames' camera-set rows, the engine's own table (cached, no upload here): fetched by the first stage that
            # needs them, once
            if not rows:
                rows.append(eng.frame_sets(meta, cameras, V))
            return rows[0]

        conf = None
        if self.evidence:
            self.last_evidence = eng.joint_evidence(fused_poses, input_heatmaps, meta, cameras, resize_transform,
                                                    reuse_staging=True)
            conf = self.last_evidence[1]
        if self.visibility is not None:
            vis = self.visibility                         # the body model travels by value, the camera tables are the engine's
            ws, hs = self.cfg.DATASET.ORI_IMAGE_SIZE
            self.last_visibility = vis(fused_poses, eng.geo.cams, frame_set(), views=self.last_evidence[0],
                                       frame_size=vis.frame_size or (hs, ws))
            if vis.feeds_conf:
                conf = self.last_visibility[1]
        if self.triangulator is not None:
            g = eng.geom(resize_transform)                # the parameters travel by value, the outputs are the triangulator's own
            g.V = V
            fs = frame_set()
            hcl = eng.heat_cl(input_heatmaps, g, reuse=True)
            occ = self.last_visibility[0] if self.visibility is not None else None
            self.last_triangulation = self.triangulator(fused_poses, eng.geo.cams, fs, hcl, occluder=occ, geom=g)
        if self.recalibrator is not None:
            self._check_needs(_STAGE["recalibrator"], views)
            if self.recalibrator_points not in ("fused", "tri"):
                raise capi.FvpError(f"model.recalibrator_points must be 'fused' or 'tri', got {self.recalibrator_points!r}")
            tri = self.last_triangulation
            pts = fused_poses if self.recalibrator_points == "fused" else tri[0]
            self.recalibrator.accumulate(pts, tri[3], tri[4], eng.geo.cams, frame_set())
        if self.tracker is not None:
            if len(eng.geo.seq_ids) > self.tracker.nseq:
                raise capi.FvpError(f"the engine has seen {len(eng.geo.seq_ids)} sequences, model.tracker was "
                                    f"built for nseq = {self.tracker.nseq}")
            self.last_tracks = self.tracker.update(fused_poses, sequences=frame_set())
            if self.smoother is not None:
                if self.smoother.nseq < self.tracker.nseq:
                    raise capi.FvpError(f"model.smoother was built for nseq = {self.smoother.nseq}, model.tracker for "
                                        f"{self.tracker.nseq}")
                self.last_smooth = self.smoother.update(fused_poses, self.last_tracks[0], self.last_tracks[1],
                                                        joint_conf=conf, sequences=frame_set())
        if self.crops is not None or self.overlay is not None:
            # ingest has read the frames on this stream already.  With a smoother the picture shows the steady poses:
            # their pixels are one more evidence launch on the staging copy of this forward, shared by crops and overlay
            px, self.last_overlay_views = self.last_evidence[0], None
            if self.smoother is not None:
                px = eng.joint_evidence(self.last_smooth[0], input_heatmaps, meta, cameras, resize_transform,
                                        reuse_staging=True)[0]
                self.last_overlay_views = px
            ids = self.last_tracks[0] if self.tracker is not None else None
            if self.crops is not None:                    # before the overlay paints: the patches hold clean pixels
                self.last_crops = self.crops(views, px, ids=ids, joint_conf=conf)
            if self.overlay is not None:
                self.overlay.draw(views, px, ids=ids, joint_conf=conf)


class GraphedForward:
    """The whole hot path captured once into a hipGraph and replayed per batch.

    The path has no host synchronisation and only static-shape launches, so one capture covers
    staging, HDN, JLN and fusion (~110 kernels); a replay costs one host call instead of ~110
    ctypes launches.  Inputs are copied into a static buffer; outputs are the graph's static
    tensors (clone them if they must outlive the next replay).

    With ``model.tracker`` set the tracker's launch is part of the graph and ``model.last_tracks`` holds static tensors;
    the track state lives in device memory, so it carries from replay to replay.  The warm-up and capture runs of the
    constructor are forwards like any other and advance that state: call ``model.tracker.reset()`` after construction.
    The same holds for ``model.smoother``: its launch is captured behind the tracker's, ``model.last_smooth`` holds static
    tensors, the filter state carries across replays - call ``model.smoother.reset()`` after construction as well.  A
    ``model.recalibrator``'s accumulate launch is captured behind the triangulation's and its accumulators carry across
    replays likewise: call ``model.recalibrator.reset()`` after construction."""

    def __init__(self, model, meta, input_heatmaps, cameras, resize_transform, warmup=2):
        self.model = model
        self.static_in = input_heatmaps.clone()
        self.args = dict(meta=meta, cameras=cameras, resize_transform=resize_transform)
        side = torch.cuda.Stream(device=input_heatmaps.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):                      # packs weights, fills caches, sizes scratch
                model(input_heatmaps=self.static_in, **self.args)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.current_stream().synchronize()
        geo = model.engine.geo
        geo.pending = [ev for ev in geo.pending if not ev.query()]     # nothing left to query inside the capture
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.out = model(input_heatmaps=self.static_in, **self.args)
        self._pinned = (geo.cams, geo.fine_grid)        # the graph reads these through raw pointers: keep them alive

    def __call__(self, input_heatmaps=None):
        if input_heatmaps is not None and input_heatmaps.data_ptr() != self.static_in.data_ptr():
            self.static_in.copy_(input_heatmaps, non_blocking=True)
        self.graph.replay()
        return self.out


class PipelinedForward:
    """Several batches in flight on one GPU: batch i runs on HIP stream i % depth with its own
    replica of the model (same weights, private scratch buffers).  The detection stage of a batch
    (CenterNet / C2CNet / NMS: small, latency-bound launches) then fills the gaps and tails of the
    previous batch's joint stage (P2PNet: large, matrix-core-bound launches); the forward has no
    host synchronisation, so submitting is just enqueueing.

    ``submit`` returns ``(outputs, event)``; the outputs are valid for a consumer stream after
    ``event.wait()`` (or after ``synchronize()``).  Results are identical to the plain forward:
    every kernel is deterministic and replicas share nothing but read-only inputs.

    Batches run on several streams and replicas, and the optional stages of ``STAGES`` need the frames in time order on
    one stream (tracker, smoother, recalibrator) or read what only one replica holds: the constructor refuses a model with
    any of them set.  Keep the stage objects beside the pipeline and call them on the consumer stream, in submit order,
    after ``event.wait()`` - each row's ``recipe`` says how, and the refusal prints it."""

    def __init__(self, model, depth=2, streams=None, backpressure=True):
        """``streams``: optional list of >= depth ``torch.cuda.Stream`` to run on (a process that builds several pipelines
        should hand them the same streams: the HIP runtime maps streams onto a fixed number of hardware queues -
        GPU_MAX_HW_QUEUES, default 4 - and streams that share a queue serialise).
        ``backpressure`` (round 6): before a slot is reused the HOST waits for the batch that ran in it last, so the host is
        never more than ``depth`` batches ahead of the GPU - nothing changes for the GPU (it always has depth - 1 batches
        queued: 3 235-3 239 frames/s with, 3 238-3 244 without), results can be consumed as they complete
        (``ResultGatherer.poll``) and the outputs of unboundedly many queued batches do not pile up.  ``wait_s`` accumulates
        the host time spent in that wait."""
        assert depth >= 1
        assert streams is None or len(streams) >= depth
        for stage in STAGES:
            if getattr(model, stage.attr) is not None:
                raise capi.FvpError("PipelinedForward runs batches on several streams and replicas: set "
                                    f"model.{stage.attr} = None and {stage.recipe}")
        self.models = [model]
        self.streams = list(streams[:depth]) if streams is not None else [torch.cuda.Stream(device=model.device) for _ in range(depth)]
        for _ in range(1, depth):
            m = FasterVoxelPoseNet(model.cfg).to(model.device)
            m.load_state_dict(model.state_dict())
            m.eval()
            m.evidence = model.evidence
            # camera tables and the per-sequence coordinate cache (164 MB for the Panoptic shape set) are read-only
            # between rebuilds: one copy for all replicas (engine.SharedGeometry orders the streams behind a rebuild)
            m.engine.geo = model.engine.geo
            self.models.append(m)
        self.depth = depth
        self._i = 0
        self.backpressure = bool(backpressure)
        self._last = [None] * depth                      # completion event of the batch that last ran in each slot
        self.wait_s = 0.0

    def submit(self, **forward_kwargs):
        k = self._i % self.depth
        self._i += 1
        st = self.streams[k]
        if self.backpressure and self._last[k] is not None:
            t0 = time.perf_counter()
            self._last[k].synchronize()
            self.wait_s += time.perf_counter() - t0
        st.wait_stream(torch.cuda.current_stream())      # inputs produced on the caller's stream
        # the inputs were allocated on the caller's stream but are read on `st`: tell the caching
        # allocator, or a caller that drops them right after submit() could see the block handed
        # out again (and overwritten on its own stream) while this batch is still queued on `st`
        for v in forward_kwargs.values():
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(st)
        with torch.cuda.stream(st), torch.no_grad():
            out = self.models[k](**forward_kwargs)
            ev = torch.cuda.Event()
            ev.record(st)
        self._last[k] = ev
        return out, ev

    @staticmethod
    def consume(outputs, stream=None):
        """Declare that ``outputs`` (allocated on a pipeline stream) are about to be read on
        ``stream`` (default: the current one) so their memory is not recycled under the reader."""
        stream = stream or torch.cuda.current_stream()
        for t in outputs:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(stream)

    def synchronize(self):
        for st in self.streams:
            st.synchronize()


class GraphedPipeline:
    """``PipelinedForward`` with every slot captured as a hipGraph (round 5): slot k = replica k + HIP stream k + one graph
    of the whole forward on that stream with a static input buffer.  ``submit(input_heatmaps)`` copies the batch into the
    slot's buffer and replays - ONE host call per batch instead of ~85 ctypes launches - and returns ``(outputs, event)``;
    the outputs are the slot's static tensors, overwritten when the slot comes round again (``depth`` submits later): read
    or clone them before that.  Same kernels, same order per slot: results equal ``PipelinedForward`` bit for bit.
    Shapes, cameras and the sequence list are fixed at capture time (the reference's caller loop, function.py:136-148,
    feeds one sequence mix per run); a different shape needs a new pipeline.  As for ``PipelinedForward``, the optional
    stages (``STAGES``) stay outside, on the consumer stream, in submit order, after ``event.wait()`` and before the slot
    comes round again."""

    def __init__(self, model, depth, meta, input_heatmaps, cameras, resize_transform, streams=None, warmup=2):
        self.pipe = PipelinedForward(model, depth=depth, streams=streams)
        self.depth, self._i = depth, 0
        args = dict(meta=meta, cameras=cameras, resize_transform=resize_transform)
        self.static_in, self.graphs, self.outs, self._pinned = [], [], [], []
        cur = torch.cuda.current_stream()
        for k in range(depth):
            st, m = self.pipe.streams[k], self.pipe.models[k]
            buf = input_heatmaps.clone()
            st.wait_stream(cur)
            with torch.cuda.stream(st), torch.no_grad():
                for _ in range(warmup):                  # packs weights, fills the shared caches, sizes the scratch
                    m(input_heatmaps=buf, **args)
            st.synchronize()                             # pending geometry rebuilds have completed ...
            # ... so their events are dropped BEFORE the capture: Event.query() inside a capture is legal on HIP today but
            # not under CUDA's global capture mode - _await_geometry then has nothing to query
            geo = m.engine.geo
            geo.pending = [ev for ev in geo.pending if not ev.query()]
            assert not geo.pending, "a geometry rebuild is still running on another stream: synchronise before capturing"
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st), torch.no_grad():
                out = m(input_heatmaps=buf, **args)
            # the graph holds RAW pointers to the shared camera table / coordinate cache: keep those tensors alive for the
            # graph's lifetime, whatever an eager run with a new sequence retires later
            self._pinned.append((geo.cams, geo.fine_grid))
            self.static_in.append(buf)
            self.graphs.append(g)
            self.outs.append(out)
        torch.cuda.synchronize()

    def submit(self, input_heatmaps):
        k = self._i % self.depth
        self._i += 1
        st = self.pipe.streams[k]
        st.wait_stream(torch.cuda.current_stream())
        input_heatmaps.record_stream(st)
        with torch.cuda.stream(st):
            self.static_in[k].copy_(input_heatmaps, non_blocking=True)
            self.graphs[k].replay()
            ev = torch.cuda.Event()
            ev.record(st)
        return self.outs[k], ev

    def synchronize(self):
        self.pipe.synchronize()


def get(cfg):
    return FasterVoxelPoseNet(cfg)
