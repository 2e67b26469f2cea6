from .lifted_feature_workflow import LiftedFeaturesFromNodeLabelsWorkflow  # noqa: F401
