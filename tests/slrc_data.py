"""A synthetic knowledge-aware dataset in the reference's on-disk format: tests/synth_data.py's interactions plus an item_meta.csv
with two item-item relation columns (r_complement, r_substitute: python list literals of tail items) and one attribute column
(i_category, 0 = missing).  The relations are built FROM the interaction sequences -- an item's complements are items that follow
it in some user's history -- so both relations occur in histories, and a few users consume an item twice, so the self relation
(interval entry 0) occurs as well."""
import os

import numpy as np
import pandas as pd

from synth_data import make_dataset


def make_kg_dataset(root, name="synth_kg", n_users=24, n_items=40, per_user=7, n_neg=20, seed=0):
    d = make_dataset(root, name, n_users=n_users, n_items=n_items, per_user=per_user, n_neg=n_neg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    frames = {p: pd.read_csv(os.path.join(d, p + ".csv"), sep="\t") for p in ("train", "dev", "test")}
    # repeat consumption: every third user's dev item becomes an item of their own training history
    train, dev = frames["train"], frames["dev"]
    for u in range(1, n_users + 1, 3):
        own = train.loc[train["user_id"] == u, "item_id"].tolist()
        dev.loc[dev["user_id"] == u, "item_id"] = own[len(own) // 2]
    dev.to_csv(os.path.join(d, "dev.csv"), sep="\t", index=False)
    every = pd.concat([frames["train"], dev, frames["test"]]).sort_values(["user_id", "time"], kind="mergesort")
    follows = {}    # item -> the items that directly follow it in a history
    for _, grp in every.groupby("user_id"):
        seq = grp["item_id"].tolist()
        for a, b in zip(seq[:-1], seq[1:]):
            if a != b:
                follows.setdefault(a, []).append(b)
    complement = {i: [] for i in range(1, n_items + 1)}     # tail lists per HEAD item
    substitute = {i: [] for i in range(1, n_items + 1)}
    for a, nxt in follows.items():
        for k, b in enumerate(dict.fromkeys(nxt)):
            (complement if k % 2 == 0 else substitute)[a].append(int(b))
    category = rng.integers(0, 4, size=n_items)     # 0: no category
    meta = pd.DataFrame({"item_id": np.arange(1, n_items + 1),
                         "i_category": category,
                         "r_complement": [complement[i] for i in range(1, n_items + 1)],
                         "r_substitute": [substitute[i] for i in range(1, n_items + 1)]})
    meta.to_csv(os.path.join(d, "item_meta.csv"), sep="\t", index=False)
    return d
