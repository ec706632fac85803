"""CPU: the DIN model classes against the reference goldens where no GPU is needed -- the init stream (SHA-256 of every tensor of the
state_dict as constructed under the golden's seed), the state_dict's key order, flags, the refusals at construction, and main's
resolution of `--model_name DIN` in both modes."""
import os
import sys

import pytest

from conftest import ROOT, load_golden
import din_model_cases as DC

sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))


@pytest.mark.parametrize("name", DC.CASES)
def test_init_stream_and_state_dict_keys_are_the_references(name):
    g = load_golden(name)
    model, _, _ = DC.build(g)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    for k, v in sd.items():
        assert DC.sha(v) == str(g["I0sha/" + k]), (name, k)
    assert [k for k in sd if k.startswith("embedding_dict.")][0] == "embedding_dict.user_id.weight"
    assert "att_mlp_layers.mlp.0.weight" in sd and "dnn_mlp_layers.mlp.0.weight" in sd


def test_main_resolves_din_in_both_modes_with_the_references_flags():
    import argparse
    import main
    assert "models.context_seq" in main.MODEL_PACKAGES
    for mode, runner in (("CTR", "CTRRunner"), ("TopK", "BaseRunner")):
        cls = main.find_class("model", ("DIN", mode))
        assert cls.__name__ == "DIN" + mode and cls.reader == "ContextSeqReader" and cls.runner == runner
        a, _ = cls.parse_model_args(argparse.ArgumentParser()).parse_known_args([])
        assert (a.emb_size, a.att_layers, a.dnn_layers, a.history_max, a.add_historical_situations) == (64, "[64]", "[64]", 20, 0)
    assert main.find_class("helper", "ContextSeqReader").__name__ == "ContextSeqReader"


@pytest.mark.parametrize("change,flag", [(dict(history_max=65), "--history_max"), (dict(history_max=0), "--history_max"),
                                         (dict(att_layers="[24]"), "--att_layers"), (dict(att_layers="[64,64,64,64]"), "--att_layers"),
                                         (dict(att_layers="[256,16]"), "--att_layers"), (dict(emb_size=258), "--emb_size")])
def test_shapes_outside_the_envelope_are_refused_at_construction(change, flag):
    from models.context_seq.DIN import DINCTR
    g = load_golden("din_ctr_d4_a16_l1_b3")
    _, args, corpus = DC.build(g)
    for k, v in change.items():
        setattr(args, k, v)
    with pytest.raises(ValueError, match=flag):
        DINCTR(args, corpus)
