"""`--model_name SetRankSequential` finds the class by its own name, beside the reference's spelling `--model_name SetRank --model_mode
Sequential` (models/reranker/SetRank.py)."""
from models.setrank_model import SetRankSequential  # noqa: F401
