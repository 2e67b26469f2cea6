from .downscaling_workflow import DownscalingWorkflow  # noqa: F401
from .downscaling import DownscalingLocal, DownscalingSlurm, DownscalingLSF  # noqa: F401
