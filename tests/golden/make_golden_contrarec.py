"""Golden vectors for ContraRec FROM THE REFERENCE ITSELF (models/sequential/ContraRec.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_contrarec.py [--out DIR]

At the reference's own init (N(0, 0.01)) the attention is uniform and the contrastive loss is rounding noise, so after
construction EVERY parameter is re-drawn from N(0, 0.5) under the case's seed and recorded.

A case is three files, because one copy of the d = 128 encoder's parameters alone is 0.7 MB and no committed file may exceed
1 MiB (tests/contrarec_np.load_case merges them):
  contrarec_<case>.npz
    meta [n_items, d, L, B, C, seed (after the ReLU re-draws, see make_case)], relu_margin [first forward, fit()], hyper [lr, l2, gamma, ctc_temp, ccc_temp], opt (name), state_keys
    P0_<key>                          the parameters (<key> = the state_dict key with '.' written as '__')
    hist, hist_a, hist_b, lengths, item_id   first training batch: the history (right-padded with 0), its two views from the
                                      reference's own Dataset.augment under np.random.seed(seed), candidate column 0 = target = label
    pred, features, ctc, ccc, loss    first batch: training prediction, the normalised features [B, 2, d], the three losses
    hist2, hist2_a, hist2_b, lengths2, item_id2   second batch
    eval_hist, eval_lengths, eval_iid, eval_pred   8 rows x 100 candidates in the test phase (model after the two iterations)
  contrarec_<case>_grads.npz   G_<key>     every parameter gradient of the first batch
  contrarec_<case>_after.npz   P2_<key>, losses   parameters after two fit() iterations (BaseRunner._build_optimizer, the fit call
                                      order, no candidate shuffle) and the two losses
Lengths come from {1, 2, L-1, L}, history ids are Zipf-distributed.

contrarec_augment.npz: 40 sequences of lengths 1..20 (flat `items` + `offsets`), `seed`, `mask_token`, beta [a, b], and the views
`a` / `b` (flat, same offsets) the reference's Dataset.augment makes of them in order a0, b0, a1, b1, ... after np.random.seed(seed).

contraloss_f64*.npz: the reference's ContraLoss in float64 on F.normalize of random features.  The features are int8 / 32 (exact
in fp32 and float64, so every consumer starts from the same numbers; `x_<i>` holds the int8).  Case i: shape_<i> [B, d, distinct
labels or 0 for labels = None], t_<i>, labels_<i> (absent for None), loss_<i> (float64), grad_<i> [B, 2, d]: the float64 gradient
with respect to the un-normalised features, stored rounded to fp32 (the B = 1025 gradients would be 1 MB each in float64; the
rounding is 6e-8 of an entry, the tests' tolerance 2e-5 of the largest).  The two B = 1025 cases are files of their own
(contraloss_f64_b1025_d64.npz, _d32.npz) for the same size limit; each file numbers its cases from 0 (`n`).
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


def _key(k):
    return k.replace(".", "__")


def _dataset(ContraRec, beta_a, beta_b, mask_token):
    """the reference's Dataset without a corpus: augment / mask_op / reorder_op only read self.model"""
    ds = object.__new__(ContraRec.Dataset)
    ds.model = SimpleNamespace(beta_a=beta_a, beta_b=beta_b, mask_token=mask_token)
    return ds


KINK = 2e-7     # smallest |ReLU pre-activation| on a valid row, relative to the largest: ~3 fp32 eps (d = 128, L = 50 has 10^6 units per forward: a wider margin never holds)


class _KinkWatch:
    """forward hooks on every TransformerLayer.linear1: the smallest and the largest |pre-activation| over the valid rows"""

    def __init__(self, model):
        self.lo, self.hi, self.valid = np.inf, 0.0, None
        for blk in model.encoder.transformer_block:
            blk.linear1.register_forward_hook(self._hook)

    def _hook(self, mod, inp, out):
        if self.valid is None:
            return
        v = out.detach().abs().numpy()[self.valid]
        self.lo, self.hi = min(self.lo, float(v.min())), max(self.hi, float(v.max()))

    def watch(self, lengths, width):
        self.valid = np.arange(width)[None, :] < np.asarray(lengths)[:, None]

    def margin(self):
        return self.lo / self.hi


def make_case(out_dir, name, *a, **kw):
    """the ReLU condition: a pre-activation within rounding of 0 has one sign in fp32 and maybe the other in anyone else's
    arithmetic, and with it every gradient below that layer moves by a unit's whole share.  The case is re-drawn (seed + 100,
    + 200, ...) until every valid-row pre-activation of both training forwards is at least KINK of the largest; asserted."""
    seed = a[-1]
    for attempt in range(100):
        if _make_case(out_dir, name, *a[:-1], seed + 100 * attempt, **kw):
            return
    raise SystemExit(name + ": the ReLU re-draw did not terminate")


def _make_case(out_dir, name, n_items, d, L, B, opt, lr, l2, seed, gamma=1.0, ctc_temp=1.0, ccc_temp=0.2, label_pool=None):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.sequential.ContraRec import ContraRec
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    C = 4
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=C - 1, dropout=0, test_all=0, emb_size=d,
                           history_max=L, gamma=gamma, beta_a=3, beta_b=3, ctc_temp=ctc_temp, ccc_temp=ccc_temp, encoder="BERT4Rec")
    corpus = SimpleNamespace(n_users=50, n_items=n_items)
    pz = 1.0 / np.arange(1, n_items)
    pz /= pz.sum()

    def draw_params():
        torch.manual_seed(seed)
        m = ContraRec(args, corpus)
        gen = torch.Generator().manual_seed(seed + 1000)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
        return m

    def zipf(size):
        return rng.choice(np.arange(1, n_items), size=size, p=pz).astype(np.int64)

    ds = _dataset(ContraRec, 3, 3, n_items)
    np.random.seed(seed)

    def batch(rows, n_cand, views=True):
        choices = sorted({1, min(2, L), max(L - 1, 1), L}, reverse=True)
        lengths = np.array([choices[i % len(choices)] for i in range(rows)], dtype=np.int64)
        rng.shuffle(lengths)
        hist = np.zeros((rows, L), dtype=np.int64)
        ha, hb = hist.copy(), hist.copy()
        for b in range(rows):
            hist[b, :lengths[b]] = zipf(lengths[b])
            if views:
                ha[b, :lengths[b]] = ds.augment(hist[b, :lengths[b]])
                hb[b, :lengths[b]] = ds.augment(hist[b, :lengths[b]])
        iid = zipf((rows, n_cand))
        if label_pool:
            iid[:, 0] = rng.choice(np.arange(1, 1 + label_pool), size=rows)
        width = int(lengths.max())     # pad_sequence pads to the longest history of the batch
        return hist[:, :width], ha[:, :width], hb[:, :width], lengths, iid

    def feed(hist, ha, hb, lengths, iid, phase="train"):
        f = {"user_id": torch.zeros(len(lengths), dtype=torch.long), "item_id": torch.from_numpy(iid),
             "history_items": torch.from_numpy(hist), "lengths": torch.from_numpy(lengths), "batch_size": len(lengths), "phase": phase}
        if phase == "train":
            f["history_items_a"], f["history_items_b"] = torch.from_numpy(ha), torch.from_numpy(hb)
        return f

    model = draw_params()
    keys = list(model.state_dict().keys())
    main = {"meta": np.array([n_items, d, L, B, C, seed], dtype=np.int64),
            "hyper": np.array([lr, l2, gamma, ctc_temp, ccc_temp], dtype=np.float64), "opt": np.array(opt), "state_keys": np.array(sorted(keys))}
    for k, v in model.state_dict().items():
        main["P0_" + _key(k)] = v.numpy().copy()

    b1, b2 = batch(B, C), batch(B, C)
    model.train()
    model.zero_grad()
    watch = _KinkWatch(model)
    watch.watch(b1[3], b1[0].shape[1])
    o = model(feed(*b1))
    if watch.margin() < KINK:
        print(name, "seed", seed, "first forward: margin %.2e, re-drawing" % watch.margin())
        return False
    loss = model.loss(o)
    loss.backward()
    with torch.no_grad():
        predictions = o["prediction"] / ctc_temp
        ctc = -ctc_temp * (predictions - predictions.max()).softmax(dim=1)[:, 0].log().mean()
        ccc = model.ccc_loss(o["features"], labels=o["labels"])
    main.update(hist=b1[0], hist_a=b1[1], hist_b=b1[2], lengths=b1[3], item_id=b1[4], pred=o["prediction"].detach().numpy().copy(),
                features=o["features"].detach().numpy().copy(), ctc=np.array(ctc.item(), dtype=np.float32),
                ccc=np.array(ccc.item(), dtype=np.float32), loss=np.array(loss.item(), dtype=np.float32))
    grads = {"G_" + _key(k): p.grad.numpy().copy() for k, p in model.named_parameters()}

    m = draw_params()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    losses = []
    watch2 = _KinkWatch(m)
    for bt in (b1, b2):
        m.train()
        m.optimizer.zero_grad()
        watch2.watch(bt[3], bt[0].shape[1])
        ls = m.loss(m(feed(*bt)))
        if watch2.margin() < KINK:
            print(name, "seed", seed, "fit(): margin %.2e, re-drawing" % watch2.margin())
            return False
        ls.backward()
        m.optimizer.step()
        losses.append(ls.item())
    after = {"P2_" + _key(k): v.numpy().copy() for k, v in m.state_dict().items()}
    after["losses"] = np.array(losses, dtype=np.float32)
    main.update(hist2=b2[0], hist2_a=b2[1], hist2_b=b2[2], lengths2=b2[3], item_id2=b2[4])
    assert watch.margin() >= KINK and watch2.margin() >= KINK
    main["relu_margin"] = np.array([watch.margin(), watch2.margin()], dtype=np.float64)

    m.eval()
    watch2.valid = None      # (the evaluation forward is not part of the condition)
    eh, _, _, en, ei = batch(8, 100, views=False)
    with torch.no_grad():
        ep = m(feed(eh, None, None, en, ei, phase="test"))["prediction"]
    main.update(eval_hist=eh, eval_lengths=en, eval_iid=ei, eval_pred=ep.numpy().copy())

    for suffix, part in (("", main), ("_grads", grads), ("_after", after)):
        path = os.path.join(out_dir, name + suffix + ".npz")
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path) >> 10, "KiB")
    return True


def make_augment(out_dir, seed=20221):
    make_golden._import_reference()
    from models.sequential.ContraRec import ContraRec
    rng = np.random.default_rng(seed)
    mask_token = 500
    ds = _dataset(ContraRec, 3, 3, mask_token)
    lengths = np.array([1 + i % 20 for i in range(40)], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = rng.integers(1, mask_token, size=int(offsets[-1])).astype(np.int64)
    a, b = np.zeros_like(items), np.zeros_like(items)
    np.random.seed(seed)
    for s in range(40):
        seq = items[offsets[s]:offsets[s + 1]]
        a[offsets[s]:offsets[s + 1]] = ds.augment(seq)
        b[offsets[s]:offsets[s + 1]] = ds.augment(seq)
    path = os.path.join(out_dir, "contrarec_augment.npz")
    np.savez_compressed(path, items=items, offsets=offsets, seed=np.int64(seed), mask_token=np.int64(mask_token),
                        beta=np.array([3, 3], dtype=np.int64), a=a, b=b)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


F64_FILES = [
    # file,                          cases (B, d, t, distinct labels | None)
    ("contraloss_f64", [(2, 4, 0.2, 1), (33, 64, 0.2, 7), (300, 128, 0.05, 40), (33, 64, 0.2, None)]),
    ("contraloss_f64_b1025_d64", [(1025, 64, 0.2, 3000)]),
    ("contraloss_f64_b1025_d32", [(1025, 32, 1.0, 2)]),
]


def make_f64(out_dir, seed=20222):
    torch, _, _ = make_golden._import_reference()
    import torch.nn.functional as F
    from models.sequential.ContraRec import ContraLoss
    torch.set_num_threads(1)
    rng = np.random.default_rng(seed)
    for fname, cases in F64_FILES:
        out = {"n": np.int64(len(cases))}
        for i, (B, d, t, distinct) in enumerate(cases):
            xi = rng.integers(-127, 128, size=(B, 2, d)).astype(np.int8)
            x = torch.tensor(xi.astype(np.float64) / 32.0, dtype=torch.float64, requires_grad=True)
            labels = None if distinct is None else rng.integers(1, 1 + distinct, size=B).astype(np.int64)
            loss = ContraLoss(torch.device("cpu"), temperature=t)(F.normalize(x, dim=-1),
                                                                 labels=None if labels is None else torch.from_numpy(labels))
            assert loss.dtype == torch.float64
            loss.backward()
            out.update({"shape_%d" % i: np.array([B, d, distinct or 0], dtype=np.int64), "t_%d" % i: np.float64(t), "x_%d" % i: xi,
                        "loss_%d" % i: np.float64(loss.item()), "grad_%d" % i: x.grad.numpy().astype(np.float32)})
            if labels is not None:
                out["labels_%d" % i] = labels
        path = os.path.join(out_dir, fname + ".npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                            n_items,   d,  L,   B, opt,       lr,   l2,   seed, extras
    ("contrarec_d64_l20_adam_b77",         200,  64, 20,  77, "Adam",    1e-3, 1e-6, 61, {}),                       # the demo flags, B off every tile
    ("contrarec_d32_l7_sgd_b160",          180,  32,  7, 160, "SGD",     0.1,  0.0,  62, dict(label_pool=5)),       # many positives per row
    ("contrarec_d128_l50_adagrad_b33",     120, 128, 50,  33, "Adagrad", 0.01, 1e-4, 63, {}),
    ("contrarec_d4_l1_sgd_b3",              60,   4,  1,   3, "SGD",     0.1,  1e-5, 64, {}),                       # every size at its minimum
    ("contrarec_d64_l20_adam_b1",          200,  64, 20,   1, "Adam",    1e-3, 0.0,  65, {}),                       # one sequence: N = 2
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c[:-1], **c[-1])
    make_augment(a.out)
    make_f64(a.out)
