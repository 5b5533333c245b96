"""Drop-in for the reference's utils/measurement.py (create_score_mat, PRfunc, PR_func); Evaluator is the chunk-wise form."""
from tf2_yolo_amd.measurement import Evaluator, PR_func, PRfunc, create_score_mat  # noqa: F401
