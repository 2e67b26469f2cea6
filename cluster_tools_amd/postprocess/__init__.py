from .postprocess_workflow import (SizeFilterWorkflow, ConnectedComponentsWorkflow,  # noqa: F401
                                   SizeFilterAndGraphWatershedWorkflow)
