from .features_workflow import EdgeFeaturesWorkflow, RegionFeaturesWorkflow  # noqa: F401
from .image_filter import ImageFilterLocal, ImageFilterSlurm, ImageFilterLSF  # noqa: F401
