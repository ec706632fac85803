"""`--model_name SetRankGeneral` finds the class by its own name, beside the reference's spelling `--model_name SetRank --model_mode
General` (models/reranker/SetRank.py)."""
from models.setrank_model import SetRankGeneral  # noqa: F401
