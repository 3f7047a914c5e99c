"""On-device data pipelines: the per-sample work of the reference's ``ClimateDataset`` for a
whole batch of raw tiles, and of its two inference datasets for whole raw grids, in HBM by ``libclimsr_hip.so``."""
from .inference_pipeline import DeviceInferencePipeline  # noqa: F401
from .tile_pipeline import DeviceTilePipeline, TransformsCfg  # noqa: F401
