from .collector import Collector  # noqa: F401
from .metrics import (Evaluator, fairness_metrics, group_gauc, group_topk_metrics, group_value_metrics,  # noqa: F401
                      topk_metrics)
