"""CPU: helpers/ContextSeqReader.py and the ContextSeq Datasets against tests/golden/context_seq_reader.json, which
tests/golden/make_golden_din_reader.py recorded from the reference's reader and Datasets on the same synthetic data."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
import din_data

sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "context_seq_reader.json")))


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


@pytest.fixture(scope="module")
def corpora(tmp_path_factory):
    from helpers.ContextSeqReader import ContextSeqReader
    root = str(tmp_path_factory.mktemp("din_reader"))
    names = din_data.write(root)
    return {mode: ContextSeqReader(din_data.reader_args(root, names[mode])) for mode in ("CTR", "TopK")}


@pytest.mark.parametrize("mode", ["CTR", "TopK"])
def test_position_column_and_user_history_are_the_references(mode, corpora):
    corpus, want = corpora[mode], GOLD[mode]
    assert corpus.situation_feature_names == want["situation_feature_names"]
    for phase in ("train", "dev", "test"):
        assert plain(corpus.data_df[phase]["position"].to_numpy()) == want["position"][phase]
    got = {str(u): [[int(i), int(t), plain(np.asarray(s))] for i, t, s in his] for u, his in corpus.user_his.items()}
    assert got == want["user_his"]


@pytest.mark.parametrize("mode", ["CTR", "TopK"])
def test_dataset_feed_dicts_are_the_references(mode, corpora):
    from models.context_seq.DIN import DINCTR, DINTopK
    cls = DINCTR if mode == "CTR" else DINTopK
    corpus, want = corpora[mode], GOLD[mode]
    model = SimpleNamespace(history_max=GOLD["history_max"], add_historical_situations=1, buffer=0, test_all=0, num_neg=1)
    for phase in ("train", "test"):
        ds = cls.Dataset(model, corpus, phase)
        assert len(ds) == want["len_" + phase]
        assert all(p > 0 for p in ds.data["position"])            # instances without history are dropped
        if mode == "TopK" and phase == "train":
            np.random.seed(5)
            ds.actions_before_epoch()
        for i, ref in zip(GOLD["indices"], want["feeds"][phase]):
            f = ds._get_feed_dict(i % len(ds))
            if mode == "TopK" and phase == "train":
                f.pop("item_id")                                   # sampled negatives: not the reader's
            got = {k: plain(v) for k, v in f.items()}
            assert list(got) == list(ref), (mode, phase, i)
            assert got == ref, (mode, phase, i)
            assert len(got["history_item_id"]) == got["lengths"] <= GOLD["history_max"]
            assert "history_c_hour_c" in got and "history_i_category_c" in got
