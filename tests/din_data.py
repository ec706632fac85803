"""The tiny synthetic datasets of the DIN reader / Dataset / CLI tests: tests/synth_data.make_context_dataset's layout (the
reference's data/README.md: interactions with c_* situation columns, item_meta.csv, user_meta.csv), one labelled set for the CTR
mode and one top-k set with neg_items, small enough that tests/golden/context_seq_reader.json can list every history."""
from synth_data import make_context_dataset

CTR, TOPK = "din_ctr", "din_topk"


def write(root, n_users=12, n_items=30, per_user=9):
    """-> {mode: dataset name}; the same arguments give the same files"""
    make_context_dataset(root, CTR, n_users=n_users, n_items=n_items, per_user=per_user, ctr=True, seed=11, numeric=True)
    make_context_dataset(root, TOPK, n_users=n_users, n_items=n_items, per_user=per_user, ctr=False, n_neg=5, seed=12)
    return {"CTR": CTR, "TopK": TOPK}


def reader_args(root, dataset, sep="\\t"):
    from types import SimpleNamespace
    return SimpleNamespace(sep="\t", path=root + "/", dataset=dataset, include_item_features=1, include_user_features=1,
                           include_situation_features=1)
