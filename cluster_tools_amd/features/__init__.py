from .features_workflow import EdgeFeaturesWorkflow  # noqa: F401
