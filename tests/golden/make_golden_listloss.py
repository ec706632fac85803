"""Golden vectors for all ten list-wise loss names FROM THE REFERENCE, run in float64 AND in fp32 -- build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_listloss.py
writes tests/golden/listloss_f64.npz (data only, < 1 MiB).  The reference's ImpressionModel.loss
(models/BaseImpressionModel.py:44-129) is imported in place and called on seeded inputs; nothing of its text is copied.

Keys:  <set>/pred (fp32), <set>/max_pos, <set>/target/bpr (every row has a negative), <set>/target/h (one row in six has none,
row 0 and the last row among them: what the H-normalised kinds listnet / softmaxCE / attention_rank run on), and per loss name
<set>/<name>/loss64, g64 (the reference on pred.double()), loss32, g32 (on pred itself).  'BPR...simple' stores its rows.
Sets:
  a0 [4, 100+200], a1 [9, 70+3], a2 [33, 3+10]: scores N(0, 1.5), ragged valid counts.  Asserted here: the reference's own
      fp32 run agrees with its float64 run within 1e-5 of the tensor's largest entry (half of what the GPU tests allow).
  c0 [9, 70+3], c1 [33, 3+10], c2 [4, 100+200]: scores N(0, 12) (saturating).
  gap [16, 6+9]: constructed; the top positive of a row lies within 5 of its top negative, every other score 20 ... 120
      below the top of its side, so pair gaps reach +-125: softplus beyond where expf overflows, both sigmoid tails.
  gap1: the same negatives with ONE positive per row, its top one (BPRhard weighs the lowest positive most: on `gap` its Q underflows).
  p1/...: attention_rank rows with two or three valid columns, one of them >= 30 above the rest: in fp32 its p is exactly 1
      and the reference drops the (1 - t) log(1 - p) term.  fp32 only (in float64 p != 1 and the term is kept).
  nf/...: non-finite behaviour as isnan / isinf masks plus the finite entries (others zeroed): a row without negatives under each
      BPR kind, a batch in which no row has a negative under the three H-normalised kinds."""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE_DIR)
sys.path.insert(0, os.path.dirname(HERE_DIR))
from make_golden import HERE, _import_reference  # noqa: E402
from make_golden_impression import lists  # noqa: E402

NAMES = ["BPR", "BPRhard", "BPRafter", "BPRhardafter", "BPRbefore", "BPRhardbefore", "listnet", "softmaxCE", "attention_rank", "BPRsimple"]
H_NORMALISED = ("listnet", "softmaxCE", "attention_rank")


def without_negatives(target, max_pos, rows):
    t = target.copy()
    t[rows, max_pos:] = -1
    return t


def one_in_six(B):
    return sorted(set(range(0, B, 6)) | {B - 1})


def gap_batch(rng, B=16, mp=6, mn=9):
    pred = np.zeros((B, mp + mn), dtype=np.float32)
    target = np.full((B, mp + mn), -1, dtype=np.int64)
    for b in range(B):
        n_pos, n_neg = rng.integers(2, mp + 1), rng.integers(2, mn + 1)
        top = rng.uniform(-10, 10)
        top_neg = top + rng.uniform(-5, 5)
        pos = top - rng.uniform(20, 120, size=n_pos)
        neg = top_neg - rng.uniform(20, 120, size=n_neg)
        pos[rng.integers(n_pos)] = top
        neg[rng.integers(n_neg)] = top_neg
        pred[b, :n_pos], pred[b, mp:mp + n_neg] = pos, neg
        target[b, :n_pos], target[b, mp:mp + n_neg] = 1, 0
    pred[0], target[0] = 0, -1   # row 0 by hand: gaps beyond 90 in both directions, whatever was drawn
    pred[0, :3], pred[0, mp:mp + 3] = (3.0, -115.0, -42.0), (1.0, -120.0, -59.0)
    target[0, :3], target[0, mp:mp + 3] = 1, 0
    return pred, target


def main():
    torch, _, _ = _import_reference()
    from models.BaseImpressionModel import ImpressionModel

    def reference(name, pred, target, mp, dtype):
        stub = SimpleNamespace(loss_n=name, train_max_pos_item=mp, device=torch.device("cpu"))
        p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
        loss = ImpressionModel.loss(stub, {"prediction": p}, torch.from_numpy(target))
        loss.sum().backward()
        return loss.detach().numpy().copy(), p.grad.numpy().copy()

    out = {}
    rng = np.random.default_rng(2024)

    def store(key, pred, target_bpr, mp, names=NAMES, check=False, rows_h=None):
        out[key + "/pred"], out[key + "/max_pos"] = pred, np.int64(mp)
        out[key + "/target/bpr"] = target_bpr.astype(np.int8)
        target_h = without_negatives(target_bpr, mp, one_in_six(len(pred)) if rows_h is None else rows_h)
        out[key + "/target/h"] = target_h.astype(np.int8)
        for name in names:
            target = target_h if name in H_NORMALISED else target_bpr
            l64, g64 = reference(name, pred, target, mp, torch.float64)
            l32, g32 = reference(name, pred, target, mp, torch.float32)
            k = "{}/{}/".format(key, name)
            out[k + "loss64"], out[k + "g64"], out[k + "loss32"], out[k + "g32"] = l64, g64, l32, g32
            with np.errstate(invalid="ignore"):
                el = np.abs(l32 - l64).max() / np.abs(l64).max()
                eg = np.abs(g32 - g64).max() / np.abs(g64).max()
            print("%-4s %-15s reference fp32 vs float64: loss %.2e  grad %.2e" % (key, name, el, eg))
            if check:
                assert np.isfinite(l64).all() and np.isfinite(g64).all(), (key, name)
                assert el <= 1e-5 and eg <= 1e-5, (key, name, el, eg)

    for key, (B, mp, mn), sd, check in (("a0", (4, 100, 200), 1.5, True), ("a1", (9, 70, 3), 1.5, True), ("a2", (33, 3, 10), 1.5, True),
                                        ("c0", (9, 70, 3), 12.0, False), ("c1", (33, 3, 10), 12.0, False)):
        pred, target = lists(rng, B, mp, mn, need_neg=True)
        store(key, (pred * np.float32(sd / 1.5)).astype(np.float32), target, mp, check=check)
    pred, target = gap_batch(rng)
    store("gap", pred, target, 6, names=[n for n in NAMES if n != "attention_rank"], rows_h=[])
    p1, t1 = pred.copy(), target.copy()
    p1[:, 0] = np.where(target[:, :6] == 1, pred[:, :6], -np.inf).max(axis=1)   # the one positive kept is the row's top one
    t1[:, 1:6] = -1
    store("gap1", p1, t1, 6, names=["BPRhard"], rows_h=[])

    # attention_rank, p == 1 in fp32
    mp = 2
    pred = np.array([[40.0, 1.0, 2.0, 0.5], [-3.0, 0.0, 33.0, 1.0], [5.0, 0.0, -30.0, 0.0], [0.3, -0.2, 0.1, 0.7],
                     [-35.0, 0.0, 1.5, -36.0], [2.0, 2.5, 50.0, 12.0]], dtype=np.float32)
    target = np.array([[1, 1, 0, -1], [1, -1, 0, 0], [1, -1, 0, -1], [1, 1, 0, 0], [1, -1, 0, 0], [1, 1, 0, 0]], dtype=np.int64)
    l32, g32 = reference("attention_rank", pred, target, mp, torch.float32)
    assert np.isfinite(l32) and np.isfinite(g32).all()
    out["p1/pred"], out["p1/target"], out["p1/max_pos"], out["p1/loss32"], out["p1/g32"] = pred, target.astype(np.int8), np.int64(mp), l32, g32

    # non-finite behaviour
    def store_nf(key, name, pred, target, mp):
        l32, g32 = reference(name, pred, target, mp, torch.float32)
        k = "nf/{}/{}/".format(key, name)
        for tag, v in (("loss", l32), ("g", g32)):
            out[k + tag + "_isnan"], out[k + tag + "_isinf"] = np.isnan(v), np.isinf(v)
            out[k + tag + "_finite"] = np.where(np.isfinite(v), v, 0).astype(np.float32)
        print("nf/%-6s %-15s loss %s; NaN gradient entries per row %s" % (key, name, l32, np.isnan(g32).sum(axis=1)))

    pred, target = lists(rng, 5, 3, 4, need_neg=True)
    out["nf/row/pred"], out["nf/row/max_pos"] = pred, np.int64(3)
    out["nf/row/target"] = without_negatives(target, 3, [2]).astype(np.int8)
    out["nf/all/pred"], out["nf/all/max_pos"] = pred, np.int64(3)
    out["nf/all/target"] = without_negatives(target, 3, list(range(5))).astype(np.int8)
    for name in NAMES:
        if name in H_NORMALISED:
            store_nf("all", name, pred, out["nf/all/target"].astype(np.int64), 3)
        else:
            store_nf("row", name, pred, out["nf/row/target"].astype(np.int64), 3)
    pred, target = lists(rng, 4, 100, 200, need_neg=True)
    store("c2", (pred * np.float32(8.0)).astype(np.float32), target, 100)
    path = os.path.join(HERE, "listloss_f64.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print("wrote", path, len(out), "arrays,", size, "bytes")


if __name__ == "__main__":
    main()
