"""The DIN goldens (tests/golden/din_*.npz, written by tests/golden/make_golden_din.py from the reference) as this project's model
classes see them: the args / corpus stand-ins, the model under the golden's seed, its scaled parameters P0 and the feed dicts.
Test infrastructure shared by tests/test_din_model_cpu.py and tests/test_gpu_din_model.py."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))

CASES = ["din_ctr_d4_a16_l1_b3", "din_ctr_d64_a64x64_l40_b33", "din_topk_d16_a64x64x64_l10_k4_b7_hs", "din_topk_d32_a256_l10_k1_b160"]


def build(g, device="cpu", dropout=0.0):
    """(model as constructed under the golden's seed, args, corpus)"""
    from models.context_seq.DIN import DINCTR, DINTopK
    n_users, n_items, d, L, B, C, seed, ctr, hs = (int(x) for x in g["meta"])
    args = SimpleNamespace(device=torch.device(device), model_path="", buffer=1, num_neg=C - 1, dropout=dropout, test_all=0,
                           emb_size=d, att_layers=str([int(x) for x in g["att_layers"]]), dnn_layers=str([int(x) for x in g["dnn_layers"]]),
                           history_max=L, add_historical_situations=hs, loss_n="BCE" if ctr else "BPR")
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, user_feature_names=[str(x) for x in g["user"]],
                             item_feature_names=[str(x) for x in g["item"]], situation_feature_names=[str(x) for x in g["sit"]],
                             feature_max={str(k): int(v) for k, v in zip(g["fmax_names"], g["fmax"])})
    torch.manual_seed(seed)
    return (DINCTR if ctr else DINTopK)(args, corpus), args, corpus


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def scale_to_p0(model, g):
    """P0 = fl(fl(I0 * 20) * att_scale): every parameter times 20, then the l-th Linear of att_mlp_layers times att_scale[l]"""
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(20.0)
        linears = [m for m in model.att_mlp_layers.mlp if isinstance(m, torch.nn.Linear)]
        assert len(linears) == len(g["att_scale"])
        for lin, s in zip(linears, g["att_scale"]):
            lin.weight.mul_(float(s))
            lin.bias.mul_(float(s))
    return model


def feed(g, n, device):
    pre = "b%d/" % n
    f = {k[len(pre):]: torch.from_numpy(np.asarray(g[k])).to(device) for k in g if k.startswith(pre)}
    f.update(batch_size=int(g["meta"][4]), phase="train")
    return f
