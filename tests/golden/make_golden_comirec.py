"""Golden vectors for ComiRec FROM THE REFERENCE ITSELF (models/sequential/ComiRec.py, helpers/BaseRunner.py), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_comirec.py [--out DIR]

At the reference's own init (N(0, 0.01)) the K interests of a sequence are nearly identical and the hard selection of
ComiRec.py:84-87 is rounding noise, so after construction EVERY parameter is re-drawn from N(0, 0.5) under the case's seed and
recorded.  Each comirec_*.npz holds
  meta [n_items, d, A, K, L, B, C, add_pos, seed], hyper [lr, l2], opt (name), state_keys
  P0_<key>                       the parameters (<key> = the state_dict key with '.' written as '__')
  hist, lengths, item_id         first training batch (history right-padded with 0; candidate column 0 is the target)
  interests, sel, target_pred, gap   the reference's interest_vectors / idx_select / target_pred of that batch (locals of its
                                 forward) and the top-2 gap of target_pred per row
  pred, loss, G_<key>            first batch: training prediction, BPR loss, every parameter gradient
  keep                           rows of the first batch with a valid position.  The reference's backward is NaN on a batch with an
                                 all-padding row (its NaN softmax row reaches every parameter through attn_score.max()'s backward),
                                 so there G_<key> is the reference's gradient over the rows `keep`, times their share of the batch
                                 mean (the all-padding row's interests are zero and its loss term constant), and the first fit()
                                 iteration runs on the rows `keep`
  hist2, lengths2, item_id2, gap2    second batch (gap2 at the parameters after the first step)
  P1_<key>, P2_<key>, losses     parameters after each of two fit() iterations (BaseRunner._build_optimizer, the fit call order)
  eval_hist, eval_lengths, eval_iid, eval_pred   8 rows x 100 candidates in the test phase (model after the two iterations)
Lengths come from {1, 2, L-1, L}, history ids are Zipf-distributed (items repeat inside a batch and inside a history; a history
of two or more positions holds at least two distinct ids, or its K interests would be one vector whatever the target).
The tie condition: for every row with at least two valid positions the target id of column 0 is re-drawn until the top-2 gap of
target_pred is at least 1e-3 of its largest magnitude in the batch, and that is asserted; rows with one valid position have K
identical interests (gap exactly 0) and no comparable selection.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

GAP = 1e-3


def _key(k):
    return k.replace(".", "__")


def _forward_with_locals(model, feed):
    """the reference's forward plus the locals it ends with (interest_vectors, target_pred, idx_select)"""
    code = type(model).forward.__code__
    got = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is code:
            got.update({k: v for k, v in frame.f_locals.items() if k in ("interest_vectors", "target_pred", "idx_select")})

    sys.setprofile(prof)
    try:
        out = model(feed)
    finally:
        sys.setprofile(None)
    return out, got


def make_case(out_dir, name, n_items, d, A, K, L, B, add_pos, opt, lr, l2, seed, all_padding_row=False, zero_between=False):
    torch, _, BaseRunner = make_golden._import_reference()
    from models.sequential.ComiRec import ComiRec
    torch.set_num_threads(1)   # one summation order for every rerun
    rng = np.random.default_rng(seed)
    C = 4
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=C - 1, dropout=0, test_all=0, emb_size=d,
                           attn_size=A, K=K, add_pos=add_pos, history_max=L)
    corpus = SimpleNamespace(n_users=50, n_items=n_items)
    pz = 1.0 / np.arange(1, n_items)
    pz /= pz.sum()

    def draw_params():
        torch.manual_seed(seed)
        m = ComiRec(args, corpus)
        gen = torch.Generator().manual_seed(seed + 1000)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
        return m

    def zipf(size):
        return rng.choice(np.arange(1, n_items), size=size, p=pz).astype(np.int64)

    def batch(rows, n_cand, special):
        choices = sorted({1, min(2, L), max(L - 1, 1), L}, reverse=True)
        lengths = np.array([choices[i % len(choices)] for i in range(rows)], dtype=np.int64)
        rng.shuffle(lengths)
        hist = np.zeros((rows, L), dtype=np.int64)
        for b in range(rows):
            hist[b, :lengths[b]] = zipf(lengths[b])
            while lengths[b] >= 2 and len(set(hist[b, :lengths[b]].tolist())) < 2:
                hist[b, :lengths[b]] = zipf(lengths[b])   # one id repeated: K identical interests whatever the target
        if special and all_padding_row:
            hist[rows // 2] = 0             # a sequence without a valid position: zero interests, zero gradients
        if special and zero_between:
            b = int(np.argmax(lengths >= 3))
            assert lengths[b] >= 3
            while hist[b, 0] == hist[b, 2]:
                hist[b, 2] = zipf(1)[0]
            hist[b, 1] = 0                  # a padding id between two valid ones: validity is hist > 0, not l < length
        return hist, lengths, zipf((rows, n_cand))

    def feed(hist, lengths, iid, phase="train"):
        return {"user_id": torch.zeros(len(lengths), dtype=torch.long), "item_id": torch.from_numpy(iid),
                "history_items": torch.from_numpy(hist), "lengths": torch.from_numpy(lengths), "batch_size": len(lengths),
                "phase": phase}

    def settle_ties(m, hist, lengths, iid):
        """re-draw the column-0 id of every row with >= 2 valid positions whose top-2 gap is under GAP * max|target_pred|"""
        multi = (hist > 0).sum(1) >= 2
        for _ in range(200):
            with torch.no_grad():
                _, loc = _forward_with_locals(m, feed(hist, lengths, iid))
            tp = loc["target_pred"].numpy()
            if K < 2:
                return np.zeros(len(lengths), dtype=np.float32)
            srt = np.sort(tp, axis=1)
            gap = srt[:, -1] - srt[:, -2]
            bad = multi & (gap < GAP * np.abs(tp).max())
            if not bad.any():
                assert (gap[multi] >= GAP * np.abs(tp).max()).all()
                return gap.astype(np.float32)
            iid[bad, 0] = zipf(int(bad.sum()))
        raise SystemExit(name + ": the tie re-draw did not terminate")

    model = draw_params()
    keys = list(model.state_dict().keys())
    out = {"meta": np.array([n_items, d, A, K, L, B, C, add_pos, seed], dtype=np.int64), "hyper": np.array([lr, l2], dtype=np.float64),
           "opt": np.array(opt), "state_keys": np.array(sorted(keys))}
    for k, v in model.state_dict().items():
        out["P0_" + _key(k)] = v.numpy().copy()

    hist, lengths, iid = batch(B, C, True)
    hist2, lengths2, iid2 = batch(B, C, False)
    out["gap"] = settle_ties(model, hist, lengths, iid)

    model.train()
    model.zero_grad()
    o, loc = _forward_with_locals(model, feed(hist, lengths, iid))
    loss = model.loss(o)
    keep = (hist > 0).any(1)
    if keep.all():
        loss.backward()
    else:
        # the reference's own backward is NaN on a batch with an all-padding row (the NaN softmax row reaches every parameter
        # through the backward of attn_score.max()).  Such a row has zero interests, a constant loss term and so no gradient:
        # the batch gradient is the reference's gradient over the other rows, times their share of the batch mean
        part = model.loss(model(feed(hist[keep], lengths[keep], iid[keep])))
        (part * (float(keep.sum()) / len(keep))).backward()
    out.update(hist=hist, lengths=lengths, item_id=iid, interests=loc["interest_vectors"].detach().numpy().copy(),
               sel=loc["idx_select"].numpy().astype(np.int64), target_pred=loc["target_pred"].detach().numpy().copy(),
               pred=o["prediction"].detach().numpy().copy(), loss=np.array(loss.item(), dtype=np.float32))
    for k, p in model.named_parameters():
        out["G_" + _key(k)] = p.grad.numpy().copy()

    m = draw_params()
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt, lr, l2))
    m.optimizer = runner._build_optimizer(m)
    losses = []
    out["keep"] = keep
    for step, (h, n, i) in enumerate(((hist[keep], lengths[keep], iid[keep]), (hist2, lengths2, iid2)), 1):
        if step == 2:
            out["gap2"] = settle_ties(m, h, n, i)
        m.train()
        m.optimizer.zero_grad()
        ls = m.loss(m(feed(h, n, i)))
        ls.backward()
        m.optimizer.step()
        losses.append(ls.item())
        for k, v in m.state_dict().items():
            out["P%d_" % step + _key(k)] = v.numpy().copy()
    out.update(hist2=hist2, lengths2=lengths2, item_id2=iid2, losses=np.array(losses, dtype=np.float32))

    m.eval()
    eh, en, ei = batch(8, 100, False)
    with torch.no_grad():
        ep = m(feed(eh, en, ei, phase="test"))["prediction"]
    out.update(eval_hist=eh, eval_lengths=en, eval_iid=ei, eval_pred=ep.numpy().copy())

    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB")


CASES = [
    # name,                          n_items,   d,  A, K,  L,   B, add_pos, opt,       lr,   l2,   seed, extras
    ("comirec_d64_a8_k4_l20_adam_b77",    200,  64,  8, 4, 20,  77, 1, "Adam",    1e-3, 1e-6, 51, dict(zero_between=True)),   # the demo flags, B off every tile
    ("comirec_d32_a4_k2_l7_sgd_b160",     180,  32,  4, 2,  7, 160, 0, "SGD",     0.1,  0.0,  52, dict(all_padding_row=True)),  # no position table
    ("comirec_d128_a16_k8_l50_adagrad_b33", 120, 128, 16, 8, 50,  33, 1, "Adagrad", 0.01, 1e-4, 53, {}),
    ("comirec_d4_a1_k1_l1_sgd_b3",         60,   4,  1, 1,  1,   3, 1, "SGD",     0.1,  1e-5, 54, {}),                        # every size at its minimum
    ("comirec_d64_a8_k4_l20_adam_b1",     200,  64,  8, 4, 20,   1, 1, "Adam",    1e-3, 0.0,  55, {}),                        # one sequence
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    for c in CASES:
        make_case(a.out, *c[:-1], **c[-1])
