"""The KDA goldens (tests/golden/kda_*.npz, written by tests/golden/make_golden_kda.py from the reference) as this project's model
class sees them: the args / corpus stand-ins, the model under the golden's seed, its scaled parameters P0 and the feed dicts.
Test infrastructure shared by tests/test_kda_model_cpu.py and tests/test_gpu_kda_model.py; the generator imports `scale_to_p0`, the
case list and the stand-ins from here as well, so both sides build the same thing."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: n_users, n_items, n_entities, emb_size, R, n_dft, L, B, num_neg, pooling, include_val, num_layers, num_heads, freq_rand,
#       gamma, (optimizer, lr, l2), seed
CASES = {
    "kda_d16_r1_f2_l1_b1_k1":         (8, 12, 12, 16, 1, 2, 1, 1, 1, "average", 1, 1, 1, 0, 0.5, ("SGD", 0.05, 1e-3), 81),      # the floor
    "kda_d32_r3_f5_l7_b3_k4":         (10, 20, 26, 32, 3, 8, 7, 3, 4, "max", 0, 2, 2, 0, -1, ("Adagrad", 0.01, 1e-4), 82),
    "kda_d64_r5_f33_l20_b33_k7":      (40, 60, 75, 64, 5, 64, 20, 33, 7, "attention", 1, 1, 4, 0, -1, ("Adam", 1e-3, 1e-6), 83),  # the demo line
    "kda_d128_r8_f129_l64_b2_k1":     (8, 30, 40, 128, 8, 256, 64, 2, 1, "average", 1, 1, 1, 1, 0.25, ("SGD", 0.05, 0.0), 84),   # the bounds; --freq_rand 1
}
DATASET_SEED = 11                        # numpy seed of the Dataset recording (tests/golden/kda_kg_dataset.npz)
N_TRIPLETS, N_INTERACTIONS = 50, 200    # len(corpus.relation_df), len(corpus.all_df): gamma -1 resolves to their ratio


def synthetic_freq_x(R, F, seed):
    """complex [R, F]: the stand-in for KDAReader.freq_x (tests/kda_data.py's rule: decays around 0.5 with a spread of 0.7)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kda_data
    re, im = kda_data.freq_tables(np.random.default_rng(seed), R, F)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def stand_ins(name, device="cpu", dropout=0.0):
    (n_users, n_items, n_ent, d, R, n_dft, L, B, K, pooling, include_val, layers, heads, freq_rand, gamma, _, seed) = CASES[name]
    args = SimpleNamespace(device=torch.device(device), model_path="", buffer=1, num_neg=K, dropout=dropout, test_all=0, emb_size=d,
                           history_max=L, neg_head_p=0.5, num_layers=layers, num_heads=heads, gamma=gamma, attention_size=10,
                           pooling=pooling, include_val=include_val, n_dft=n_dft, freq_rand=freq_rand)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, n_relations=R, n_entities=n_ent,
                             freq_x=synthetic_freq_x(R, n_dft // 2 + 1, seed), relation_df=range(N_TRIPLETS), all_df=range(N_INTERACTIONS))
    return args, corpus


def build(name, device="cpu"):
    """(model as constructed under the golden's seed, args, corpus)"""
    sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))
    from models.sequential.KDA import KDA
    args, corpus = stand_ins(name, device)
    torch.manual_seed(CASES[name][-1])
    return KDA(args, corpus), args, corpus


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def scale_to_p0(model, g):
    """P0 from the constructed parameters, in float32: every parameter outside layer_norm and the frequency tables times 20; then entity_embeddings and
    relation_embeddings times emb_scale (chosen by the generator so that the aggregation's logits have a standard deviation of 1.5
    over the valid positions); then, under --freq_rand 1 only, freq_real and freq_imag times freq_scale (raw decays with a standard
    deviation of 1.2)"""
    agg = model.relational_dynamic_aggregation
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "layer_norm" not in k and "freq_" not in k:
                p.mul_(20.0)
        model.entity_embeddings.weight.mul_(float(g["emb_scale"]))
        model.relation_embeddings.weight.mul_(float(g["emb_scale"]))
        if model.freq_rand:
            agg.freq_real.weight.mul_(float(g["freq_scale"]))
            agg.freq_imag.weight.mul_(float(g["freq_scale"]))
    return model


def feed(g, n, device, B):
    pre = "b%d/" % n
    f = {k[len(pre):]: torch.from_numpy(np.asarray(g[k])).to(device) for k in g if k.startswith(pre)}
    f.update(batch_size=B, phase="train")
    return f
