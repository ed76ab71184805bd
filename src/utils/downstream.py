"""ref src/utils/downstream.py: `count_f1_max` with the reference's name and parameters, computed on the device (oneprot_amd.downstream: a stable sort,
so the order of equal scores is defined; returns a Python float and prints nothing), and `load_data`.  `save_results_to_csv` is not ported."""
from oneprot_amd.downstream import (accuracy, argsort, binary_auc, count_f1_max, evaluate_predictions, load_data, midranks, regression_scores,  # noqa: F401
                                    spearman_rho)
