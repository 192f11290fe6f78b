from .collector import Collector  # noqa: F401
from .metrics import (Evaluator, fairness_metrics, group_exposure_metrics, group_gauc, group_topk_metrics,  # noqa: F401
                      group_value_metrics, topk_metrics)
