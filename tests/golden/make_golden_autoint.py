"""Golden vectors for AutoInt FROM THE REFERENCE ITSELF (models/context/AutoInt.py, utils/layers.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_autoint.py [--out DIR]

Each autoint_*.npz holds
  meta [n_users, n_items, d, A, H, n_layers, B, C, seed, ctr] + tower widths, fields (names in model order), numeric (names)
  feature_max     the corpus' feature_max of every field, in the order of `fields`
  I0/<key>        the state_dict straight after construction under torch.manual_seed(seed): pins the init stream.  Left out of the one
                  case whose tensors would not fit the size limit a fourth time (store_i0 = False): tests/autoint_np.py:init_from_seed
                  regenerates it from the seed on plain torch modules, this generator asserts that restatement to be bit-equal
                  to the reference's state_dict in EVERY case, and that case stores I0sha/<key>, the SHA-256 of each reference tensor
  qk_scale [L]    the parameters every computation below starts from are P0 = I0 x 20, then, layer by layer on the first batch, that
                  layer's q_linear and k_linear weights multiplied by qk_scale[l] = sqrt(2.5 / std(S)) so that the scaled scores S
                  have standard deviation 2.5.  (x 20 alone leaves every softmax row uniform -- the attention path would go
                  untested; a larger uniform factor saturates the sigmoid and zeroes the gradients.)  P0 itself is not stored: it
                  is fl(fl(I0 * 20) * qk_scale) in float32, which tests/autoint_np.py:scaled_params recomputes and this generator
                  asserts to be bit-equal to the parameters it ran (a second copy of every tensor would not fit the size limit)
  b1/<f>, b2/<f>  two training batches (ids, features, label for CTR)
  Y<l>            every layer's output on the first batch [B, C, F, A];  pmax<l>: the largest probability of every softmax row
  pred, loss, gpred, G/<key>     first batch: prediction, loss, d loss / d prediction, every parameter's gradient
  <opt>/<key>, <opt>_losses, <opt>_hyper     parameters after two optimizer steps from P0, the two losses, (lr, l2)
  <opt>/s1/<key>  the two small TopK cases (store_s1): the parameters after the first step as well.  Their gradients hold elements
                  that are round-off around an exact zero; Adam turns such an element into a step of about lr in a direction the
                  round-off decides; the tests compare the first step, set those elements to the reference's values and compare the second
  state_keys      the state_dict's keys in order
  dev/<key>, dev/pred            categorical-only cases: the reference's own fp32 result against a float64 run of the same modules
                                 driven by the stored gpred, as largest |difference| / largest |float64 entry|
The generator asserts, per case: in every layer at least half of the softmax rows have a largest probability above the
non-uniformity threshold (row_threshold below), and between 25 % and 75 % of the last layer's outputs are positive.
"""
import argparse
import copy
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (numpy alias shim too)
from make_golden_deepfm import ITEM_F, MIND, MIND_FLOAT, SIT_F, USER_F, VOCAB  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import autoint_np  # noqa: E402
from autoint_np import row_threshold  # noqa: E402

# MIND's field names and value types with small vocabularies: the tables are not what these goldens are about, and every stored
# copy of them counts against the size limit
SMALL = {"i_category_c": 6, "i_subcategory_c": 12, "c_hour_c": 8, "c_period_c": 4, "c_weekday_c": 7}
MIND_S, MIND_FLOAT_S = dict(MIND, vocab=SMALL), dict(MIND_FLOAT, vocab=SMALL)
GENERIC = dict(user=USER_F, item=ITEM_F, sit=SIT_F, vocab=VOCAB, numeric={})
ONE_FEATURE = dict(user=[], item=ITEM_F, sit=[], vocab={"i_category_c": 11}, numeric={})
IDS_ONLY = dict(user=[], item=[], sit=[], vocab={}, numeric={})
SCORE_STD = 2.5


def make_case(out_dir, name, mode, d, A, H, n_layers, tower, B, K, spec, opts, seed, n_users, n_items, store_i0=True, store_s1=False):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.context.AutoInt import AutoIntCTR, AutoIntTopK
    torch.set_num_threads(1)   # one summation order for every rerun
    ctr = mode == "CTR"
    cls = AutoIntCTR if ctr else AutoIntTopK
    USER, ITEM, SIT, VOC, NUMERIC = spec["user"], spec["item"], spec["sit"], spec["vocab"], spec["numeric"]
    rng = np.random.default_rng(seed)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=K, dropout=0, test_all=0, emb_size=d,
                           attention_size=A, num_heads=H, num_layers=n_layers, layers=str(tower), loss_n="BCE" if ctr else "BPR")
    fmax = dict(VOC, user_id=n_users, item_id=n_items)
    for f, (_, top) in NUMERIC.items():     # helpers/ContextReader.py:52-53 records max + 1 for every feature; unused for '*_f'
        fmax[f] = top
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items, user_feature_names=USER, item_feature_names=ITEM,
                             situation_feature_names=SIT, feature_max=fmax)
    torch.manual_seed(seed)
    model = cls(args, corpus)
    F = len(model.context_features)
    C = 1 if ctr else 1 + K
    out = {"meta": np.array([n_users, n_items, d, A, H, n_layers, B, C, seed, int(ctr)] + list(tower), dtype=np.int64),
           "fields": np.array(model.context_features), "numeric": np.array(sorted(NUMERIC), dtype=str)}
    out["feature_max"] = np.array([fmax[f] for f in model.context_features], dtype=np.int64)
    out["state_keys"] = np.array(list(model.state_dict().keys()))
    I0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    restated = autoint_np.init_from_seed(out)
    assert list(restated) == list(I0), (name, list(restated), list(I0))
    for k, v in I0.items():
        assert restated[k].tobytes() == v.tobytes(), (name, k)
        if store_i0:
            out["I0/" + k] = v
        else:      # the reference's own bits all the same: SHA-256 of every tensor (autoint_np.initial_params checks against it)
            out["I0sha/" + k] = np.array(hashlib.sha256(v.tobytes()).hexdigest())

    def column(f, size):
        if f not in NUMERIC:
            return rng.integers(0, VOC[f], size=size).astype(np.int64)
        dtype, top = NUMERIC[f]
        if dtype == "int64":
            return rng.integers(0, top, size=size).astype(np.int64)
        return (rng.random(size=size) * (top - 1)).astype(np.float64)

    item_cols = {f: column(f, n_items) for f in ITEM}     # item_meta: one value per item

    def batch():
        b = {"user_id": rng.integers(1, n_users, size=B).astype(np.int64),
             "item_id": rng.integers(1, n_items, size=(B, C)).astype(np.int64)}
        b["item_id"][:, 0] = b["item_id"][:, 0] % 5 + 1  # duplicates
        for f in USER + SIT:
            b[f] = column(f, B)
        for f in ITEM:
            b[f] = item_cols[f][b["item_id"]]
        if ctr:
            b["label"] = rng.integers(0, 2, size=(B, 1)).astype(np.int64)
        return b

    batches = [batch(), batch()]
    for n, b in enumerate(batches, 1):
        for k, v in b.items():
            out["b%d/%s" % (n, k)] = v

    def feed(b):
        f = {k: torch.from_numpy(v) for k, v in b.items()}
        f.update(batch_size=B, phase="train")
        return f

    def layers_of(m, fd):
        """every layer's (scores after the 1 / sqrt(dk), output): AutoInt.py:70-75 spelled out on the reference's own modules"""
        x, _ = m._get_embeddings_FM(fd)
        res = []
        for att, lin in zip(m.autoint_attentions, m.residual_embeddings):
            q, k = att.head_split(att.q_linear(x)), att.head_split(att.k_linear(x))
            S = torch.matmul(q, k.transpose(-2, -1)) / att.d_k ** 0.5
            x = (att(x, x, x) + lin(x)).relu()
            res.append((S, x))
        return res

    with torch.no_grad():
        for p in model.parameters():
            p.mul_(20.0)
        qk_scale = []
        for l in range(n_layers):
            S = layers_of(model, feed(batches[0]))[l][0]
            s = float(np.float32(np.sqrt(SCORE_STD / S.double().std().item())))
            qk_scale.append(s)
            model.autoint_attentions[l].q_linear.weight.mul_(s)
            model.autoint_attentions[l].k_linear.weight.mul_(s)
        per_layer = layers_of(model, feed(batches[0]))
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out["qk_scale"] = np.array(qk_scale, dtype=np.float32)
    derived = autoint_np.scaled_params(out)
    for k, v in P0.items():
        assert derived[k].tobytes() == v.tobytes(), (name, k)
    for l, (S, Y) in enumerate(per_layer):
        pmax = S.softmax(dim=-1).max(dim=-1).values.numpy()
        share = float((pmax > row_threshold(F)).mean())
        assert share >= 0.5, (name, l, share)
        out["Y%d" % l], out["pmax%d" % l] = Y.numpy().copy(), pmax.copy()
        print("  layer %d: std(S) %.3f, rows above %.3f: %.0f %%" % (l, S.std().item(), row_threshold(F), 100 * share))
    active = float((per_layer[-1][1] > 0).float().mean())
    assert 0.25 <= active <= 0.75, (name, active)
    print("  active outputs of the last layer: %.0f %%" % (100 * active))

    model.zero_grad()
    o = model(feed(batches[0]))
    pred = o["prediction"]
    pred.retain_grad()
    loss = model.loss(o)
    loss.backward()
    out["pred"], out["loss"], out["gpred"] = pred.detach().numpy().copy(), np.float32(loss.item()), pred.grad.numpy().copy()
    for k, p in model.named_parameters():
        out["G/" + k] = p.grad.numpy().copy()

    if not NUMERIC:     # the reference's .float() calls stop a double run with numeric fields
        m64 = copy.deepcopy(model).double()
        m64.zero_grad()
        ref_pred = m64(feed(batches[0]))["prediction"]      # CTR: the probability (the sigmoid of :97 in double as well)
        ref_pred.backward(torch.from_numpy(out["gpred"]).double().view_as(ref_pred))
        scale = ref_pred.detach().abs().max().item()
        out["dev/pred"] = np.float64((torch.from_numpy(out["pred"]).double().view(-1) - ref_pred.detach().view(-1)).abs().max().item() / scale)
        for k, p in m64.named_parameters():
            # (a gradient that is exactly zero in exact arithmetic -- the first-order terms of the user-side fields under BPR -- is
            # round-off on both sides: the floor of autoint_np.grad_floor keeps its ratio meaningful)
            g64 = p.grad.numpy()
            out["dev/" + k] = np.float64(autoint_np.rel_err(out["G/" + k], g64, autoint_np.grad_floor(out)))
        print("  fp32 vs float64: pred %.1e, worst gradient %.1e" % (out["dev/pred"], max(out["dev/" + k] for k, _ in m64.named_parameters())))

    for opt_name, lr, l2 in opts:
        m = cls(args, corpus)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in P0.items()})
        runner = BaseRunner(make_golden._runner_args(BaseRunner, opt_name, lr, l2))
        m.optimizer = runner._build_optimizer(m)
        losses = []
        for step, b in enumerate(batches, 1):
            m.optimizer.zero_grad()
            ls = m.loss(m(feed(b)))
            ls.backward()
            m.optimizer.step()
            losses.append(ls.item())
            if store_s1 and step == 1:
                for k, v in m.state_dict().items():
                    out["{}/s1/{}".format(opt_name, k)] = v.detach().numpy().copy()
        for k, v in m.state_dict().items():
            out["{}/{}".format(opt_name, k)] = v.detach().numpy().copy()
        out[opt_name + "_losses"] = np.array(losses, dtype=np.float32)
        out[opt_name + "_hyper"] = np.array([lr, l2], dtype=np.float64)
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


ADAM_SGD = (("Adam", 1e-3, 1e-4), ("SGD", 0.05, 1e-3))
CASES = [
    # name,                             mode,    d,  A,  H, layers, tower,   B, K, fields,       optimizers,                  seed, users, items
    ("autoint_mind_ctr_d64_a32_h1_l1",  "CTR",  64, 32, 1, 1, [64],     48, 0, MIND_S,       ADAM_SGD,                    61,  8, 10),   # the default flags, F = 8
    ("autoint_mindf_ctr_d64_a32_h2_l2", "CTR",  64, 32, 2, 2, [64, 32], 33, 0, MIND_FLOAT_S, ADAM_SGD,                    70,  8, 10, False),   # float c_day_f and i_age_f, F = 9
    ("autoint_topk_d16_a8_h4_l3_k4",    "TopK", 16,  8, 4, 3, [32],     24, 4, GENERIC,      ADAM_SGD,                    63, 40, 60, True, True),   # F = 7
    ("autoint_ctr_d128_a64_h8_l1_b3",   "CTR", 128, 64, 8, 1, [],        3, 0, ONE_FEATURE,  (("Adagrad", 0.01, 1e-4),),  64,  6,  8),   # F = 3
    ("autoint_ids_topk_d8_a4_h4_l1_b1", "TopK",  8,  4, 4, 1, [],        1, 1, IDS_ONLY,     ADAM_SGD,                    65, 40, 60, True, True),   # dk = 1, F = 2
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        print(c[0])
        make_case(a.out, *c)
