"""tests/golden/context_seq_reader.json FROM THE REFERENCE ITSELF (helpers/ContextSeqReader.py, models/BaseContextModel.py,
models/context_seq/DIN.py's Datasets), on CPU, on the tiny synthetic datasets tests/din_data.py writes:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_din_reader.py

per mode (CTR, TopK): the `position` column of every phase, `user_his` (item, time, situation values per interaction) and the feed
dicts of a few indices of the train and test Datasets (--history_max 4, --add_historical_situations 1)."""
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import din_data  # noqa: E402

INDICES = [0, 1, 5, 17, -1]


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def main():
    torch, _, _ = make_golden._import_reference()
    from helpers.ContextSeqReader import ContextSeqReader
    from models.context_seq.DIN import DINCTR, DINTopK
    out = {"indices": INDICES, "history_max": 4}
    with tempfile.TemporaryDirectory() as root:
        names = din_data.write(root)
        for mode, cls in (("CTR", DINCTR), ("TopK", DINTopK)):
            a = din_data.reader_args(root, names[mode])
            corpus = ContextSeqReader(a)
            rec = {"position": {ph: plain(corpus.data_df[ph]["position"].to_numpy()) for ph in ("train", "dev", "test")},
                   "user_his": {str(u): [[int(i), int(t), plain(np.asarray(s))] for i, t, s in his] for u, his in corpus.user_his.items()},
                   "situation_feature_names": corpus.situation_feature_names, "feeds": {}}
            model = SimpleNamespace(history_max=4, add_historical_situations=1, buffer=0, test_all=0, num_neg=1)
            for phase in ("train", "test"):
                ds = cls.Dataset(model, corpus, phase)
                if mode == "TopK" and phase == "train":
                    np.random.seed(5)
                    ds.actions_before_epoch()
                feeds = []
                for i in INDICES:
                    f = ds._get_feed_dict(i % len(ds))
                    f.pop("item_id") if (mode == "TopK" and phase == "train") else None      # sampled negatives: not the reader's
                    feeds.append({k: plain(v) for k, v in f.items()})
                rec["feeds"][phase] = feeds
                rec["len_" + phase] = len(ds)
            out[mode] = rec
    path = os.path.join(HERE, "context_seq_reader.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


if __name__ == "__main__":
    main()
