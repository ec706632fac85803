"""`--model_name PRMGeneral` finds the class by its own name, beside the reference's spelling `--model_name PRM --model_mode General`
(models/reranker/PRM.py)."""
from models.prm_model import PRMGeneral  # noqa: F401
