"""Data-format helpers either side of the hot path."""
from .heatmaps import generate_input_heatmaps  # noqa: F401
from .images import BayerFrames, Nv12Frames, demosaic_bayer, ingest_bayer, ingest_frames, ingest_nv12  # noqa: F401
