"""`--model_name PRMSequential` finds the class by its own name, beside the reference's spelling `--model_name PRM --model_mode Sequential`
(models/reranker/PRM.py)."""
from models.prm_model import PRMSequential  # noqa: F401
