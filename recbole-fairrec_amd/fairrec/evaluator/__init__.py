from .collector import Collector  # noqa: F401
from .metrics import (Evaluator, bootstrap_fairness, bootstrap_group_sums, bootstrap_intervals, fairness_metrics,  # noqa: F401
                      gauc_user_terms, group_exposure_metrics, group_gauc, group_topk_metrics, group_value_metrics, topk_metrics,
                      topk_user_terms, value_type_rows)
