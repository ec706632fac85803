"""Stored fp32 deviations for the list encoder block problems of tests/test_gpu_prm.py, on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prm.py [--out DIR]

prm_layer_dev.npz holds no tensors: <B>_<n>_<d>_<H>_<d_ff>_<seed>/<tensor> is, for every random block problem of
prm_np.LAYER_PROBLEMS (regenerated from its seed, never stored), the deviation of torch's own nn.TransformerEncoderLayer in float32 --
the module the reference stacks (models/reranker/PRM.py:64) -- from the float64 restatement in tests/prm_np.py, as
largest |difference| / largest |float64 entry|, for Y, dX and the twelve weight and bias gradients.  <key>/maxp is the largest
attention probability of the problem's least peaked list as a multiple of the uniform value (lists with more than two valid keys).
The GPU tests hold the kernels to max(2e-5, 4 x these stored figures).  The generator asserts that every problem with such a list has
maxp > 2: a kernel without the softmax would not pass.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import prm_np  # noqa: E402


def make_layer_devs(out_dir):
    import torch
    torch.set_num_threads(1)   # one summation order for every rerun
    out = {}
    for prob_id in prm_np.LAYER_PROBLEMS:
        key, H = prm_np.layer_key(*prob_id), prob_id[3]
        prob = prm_np.random_block(*prob_id)
        for name, v in prm_np.fp32_deviation(prob, H).items():
            out["%s/%s" % (key, name)] = np.float64(v)
        maxp = prm_np.largest_probability(prob[0], prob[1], prob[2], H)
        if maxp is not None:
            assert maxp > 2.0, (prob_id, maxp)
            out[key + "/maxp"] = np.float64(maxp)
    path = os.path.join(out_dir, "prm_layer_dev.npz")
    np.savez_compressed(path, **out)
    worst = max((float(v), k) for k, v in out.items() if not k.endswith("/maxp"))
    print("wrote", path, os.path.getsize(path) >> 10, "KiB; largest deviation %.2e (%s)" % worst)


# ---- the model cases, FROM THE REFERENCE ITSELF (models/reranker/PRM.py, models/BaseRerankerModel.py, helpers/BaseRunner.py) -----------
def _lists(rng, B, P, N, n_items, single):
    """(pos_num, neg_num, item lists): list 0 has every slot valid, list 2 padding inside the positives; single: list 1 has ONE valid
    slot (one positive, no negative).  The reference's list-level BPR is NaN for a list without a negative (its softmax over the
    valid negatives is over nothing; the reader drops such impressions), so the two training batches keep at least one negative in
    every list and the single-slot list lives in a third, forward-only batch."""
    pos, neg = rng.integers(1, P + 1, size=B), rng.integers(1, N + 1, size=B)
    pos[0], neg[0] = P, N
    if B > 1:
        pos[1], neg[1] = 1, (0 if single else 1)
    if B > 2 and P > 1:
        pos[2], neg[2] = P - 1, max(1, N - 1)
    # distinct items within a list: two slots with one item tie under the ranker, and the rank of tied valid slots is the sort's choice
    items = [rng.permutation(np.arange(1, n_items))[:p + k] for p, k in zip(pos, neg)]
    return pos, neg, [it[:p] for it, p in zip(items, pos)], [it[p:] for it, p in zip(items, pos)]


def make_case(out_dir, name, ranker, emb, hidden, H, blocks, P, N, opt, B, seed, history=0):
    import copy
    import tempfile
    from types import SimpleNamespace
    import yaml
    import make_golden
    torch, _, BaseRunner = make_golden._import_reference()
    from models.reranker.PRM import PRMGeneral, PRMSequential
    torch.set_num_threads(1)
    seq = ranker == "SASRec"
    n_users, n_items, n = 40, 60, P + N
    rng = np.random.default_rng(seed)
    config = dict(emb_size=emb, num_layers=1, num_heads=2, history_max=99) if seq else dict(emb_size=emb)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR",
                           emb_size=emb, train_max_pos_item=P, train_max_neg_item=N, test_max_pos_item=P, test_max_neg_item=N,
                           ranker_name=ranker, ranker_config_file=ranker + ".yaml", ranker_model_file="ranker.pt", tuneranker=0,
                           n_blocks=blocks, num_heads=H, num_hidden_unit=hidden, history_max=history)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            folder = "model/%sImpression" % ranker
            os.makedirs(folder)
            import importlib
            mod = importlib.import_module("models.%s.%s" % ("sequential" if seq else "general", ranker))
            ra = copy.deepcopy(args)
            for k, v in config.items():
                if k != "history_max":
                    setattr(ra, k, v)
            torch.manual_seed(seed + 1)
            rk = getattr(mod, ranker + "Impression")(ra, corpus)
            with torch.no_grad():      # a ranker whose scores differ visibly between candidates (its init is normal(0, 0.01))
                for p_ in rk.parameters():
                    if p_.dim() == 2 and p_.shape[1] == emb and p_.shape[0] in (n_users, n_items):
                        p_.mul_(ITEM_SCALE if p_.shape[0] == n_items else USER_SCALE)
            R = {k: v.detach().numpy().copy() for k, v in rk.state_dict().items()}
            torch.save(rk.state_dict(), folder + "/ranker.pt")
            with open(folder + "/" + ranker + ".yaml", "w") as f:
                yaml.safe_dump(config, f)
            torch.manual_seed(seed)
            model = (PRMSequential if seq else PRMGeneral)(args, corpus)
            head0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if not k.startswith("ranker.")}
            # the reference's head init re-draws the ranker it has just loaded (self.apply reaches self.ranker); the port loads the
            # checkpoint again afterwards, and so does this generator before anything is recorded
            model.ranker.load_model(folder + "/ranker.pt")
        finally:
            os.chdir(here)
    out = {"meta": np.array([n_users, n_items, emb, hidden, H, blocks, P, N, B, seed, int(seq), history], dtype=np.int64),
           "ranker": np.array(ranker), "ranker_yaml": np.array(yaml.safe_dump(config)),
           "state_keys": np.array(list(model.state_dict().keys()))}
    for k, v in R.items():
        out["R/" + k] = v
    for k, v in head0.items():
        out["I0/" + k] = v

    ds = model.Dataset.__new__(model.Dataset)
    ds.model, ds.corpus, ds.phase, ds.pos_len, ds.neg_len = model, corpus, "train", P, N

    def batch(single=False):
        pos, neg, pl, nl = _lists(rng, B, P, N, n_items, single)
        feeds = []
        for b in range(B):
            fd = {"user_id": int(rng.integers(1, n_users)), "pos_items": pl[b], "neg_items": nl[b], "pos_num": int(pos[b]), "neg_num": int(neg[b])}
            if seq:
                h = rng.integers(1, n_items, size=int(rng.integers(1, history + 1)))
                fd.update(history_items=h, neg_history_items=h[:1], history_times=np.arange(len(h)), neg_history_times=np.arange(1),
                          lengths=len(h), neg_lengths=1)
            feeds.append(fd)
        with torch.no_grad():
            return ds.collate_batch(feeds)
    batches = [batch(), batch(), batch(single=True)]      # b3: forward only
    for i, bt in enumerate(batches, 1):
        for k, v in bt.items():
            if torch.is_tensor(v) and (i == 1 or k not in ("u_v", "i_v", "his_v")):      # (the vectors of the first batch only: size)
                out["b%d/%s" % (i, k)] = prm_np.keep(v.detach().numpy()) if k in ("u_v", "i_v", "his_v") else v.detach().numpy().copy()

    # in_proj / out_proj rescaled block by block on the first batch, so that the softmax rows are visibly non-uniform and the
    # attention output counts beside the residual
    valid = ~batches[0]["padding_mask"].numpy()
    in_scale, out_scale, maxp = np.ones(blocks, np.float32), np.ones(blocks, np.float32), np.zeros(blocks)

    def block_inputs():
        seen = []
        hooks = [blk.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().transpose(0, 1).numpy().copy())) for blk in model.encoder]
        with torch.no_grad():
            model(batches[0])
        for h_ in hooks:
            h_.remove()
        return seen

    def probs(l):
        W = [dict(model.encoder[l].named_parameters())[k].detach().numpy() for k in prm_np.TORCH_KEYS]
        return prm_np.largest_probability(block_inputs()[l], (~valid).astype(np.uint8), W, H)
    # rFF0 / rFF1 (normal(0, 0.01)) x FF_SCALE as well: unscaled, the block stack's input is so small that in_proj has to be scaled by
    # several hundred for a visible softmax, and the loss sits at ln 2
    ff = FF_SCALE
    with torch.no_grad():
        model.rFF0.weight.mul_(ff)
        model.rFF1.weight.mul_(ff)
    out["ff_scale"] = np.float32(ff)
    for l in range(blocks):
        blk = model.encoder[l]
        with torch.no_grad():
            out_scale[l] = 30.0
            blk.self_attn.out_proj.weight.mul_(float(out_scale[l]))
            mp = probs(l)
            while mp is not None and mp < 3.0:
                blk.self_attn.in_proj_weight.mul_(1.5)
                in_scale[l] *= np.float32(1.5)
                mp = probs(l)
        maxp[l] = 0.0 if mp is None else mp
        assert mp is None or mp > 2.0, (name, l, mp)
    out["in_scale"], out["out_scale"], out["maxp"] = in_scale, out_scale, maxp
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    derived = prm_np.scale_state({k: v for k, v in P0.items() if k.startswith("ranker.")} | head0, out)
    for k, v in P0.items():
        assert derived[k].tobytes() == v.tobytes(), (name, k)

    def labels(bt):
        col = torch.arange(n)[None, :]
        return torch.where(col < bt["pos_num"][:, None], 1, torch.where((col >= P) & (col < P + bt["neg_num"][:, None]), 0, -1)).long()

    def run(m, bt, dtype):
        fd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in bt.items()}
        xs = []
        hooks = [blk.register_forward_hook(lambda mod_, a, o: xs.append(o.detach().transpose(0, 1).numpy().copy())) for blk in m.encoder]
        m.zero_grad()
        o = m(fd)
        for h_ in hooks:
            h_.remove()
        pred = o["prediction"]
        pred.retain_grad()
        loss = m.loss(o, labels(bt))
        loss.backward()
        G = {k: p.grad.numpy().copy() for k, p in m.named_parameters() if p.requires_grad}
        return xs, pred.detach().numpy().copy(), float(loss.item()), pred.grad.numpy().copy(), G
    model.train()
    xs, pred, loss, gpred, G = run(model, batches[0], torch.float32)
    m64 = copy.deepcopy(model).double()
    xs64, pred64, loss64, _, G64 = run(m64, batches[0], torch.float64)
    for l in range(blocks):
        # (valid slots only: a padded slot's rank, hence its position embedding and its row, is the sort's choice among ties)
        out["X%d" % l], out["dev/X%d" % l] = prm_np.keep(xs[l][valid]), np.float64(prm_np.rel_err(xs[l][valid], xs64[l][valid]))
    out["pred"], out["loss"], out["gpred"] = pred, np.float32(loss), gpred
    assert np.isfinite(loss) and np.isfinite(pred).all()

    def forward_only(m, bt, dtype):
        fd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in bt.items()}
        xs_ = []
        hooks = [blk.register_forward_hook(lambda mod_, a, o: xs_.append(o.detach().transpose(0, 1).numpy().copy())) for blk in m.encoder]
        with torch.no_grad():
            p_ = m(fd)["prediction"].numpy().copy()
        for h_ in hooks:
            h_.remove()
        return xs_, p_
    v3 = ~batches[2]["padding_mask"].numpy()
    assert B == 1 or (v3.sum(1) == 1).any()
    (f32x, f32p), (f64x, f64p) = forward_only(model, batches[2], torch.float32), forward_only(m64, batches[2], torch.float64)
    for l in range(blocks):
        out["F/X%d" % l], out["dev/F/X%d" % l] = prm_np.keep(f32x[l][v3]), np.float64(prm_np.rel_err(f32x[l][v3], f64x[l][v3]))
    out["F/pred"], out["dev/F/pred"] = f32p, np.float64(prm_np.rel_err(f32p[v3], f64p[v3]))
    out["dev/pred"] = np.float64(prm_np.rel_err(pred[valid], pred64[valid]))
    out["dev/loss"] = np.float64(abs(loss - loss64) / abs(loss64))
    gmax = max(float(np.abs(v).max()) for v in G.values())
    # exactly zero in exact arithmetic, round-off in every precision: under BPR a shift of all scores of a list changes nothing, so
    # rFF1.bias and what only shifts them (the last block's norm2.bias) get no gradient.  No dev/ for them.
    zero = [k for k, v in G64.items() if float(np.abs(v).max()) <= 1e-9 * gmax]
    out["zero_grad_keys"] = np.array(zero, dtype=str)
    for k, v in G.items():
        out["G/" + k] = prm_np.keep(v)
        if k in zero:
            assert float(np.abs(v).max()) <= 1e-5 * gmax, (name, k)
        else:
            out["dev/G/" + k] = np.float64(prm_np.rel_err(v, G64[k], 1e-6 * gmax))
    print("  fp32 vs float64: x_L %.1e, pred %.1e, loss %.1e, worst gradient %.1e; zero gradients %s; largest probability x uniform per block %s"
          % (out["dev/X%d" % (blocks - 1)], out["dev/pred"], out["dev/loss"], max(out["dev/G/" + k] for k in G if k not in zero), zero,
             np.round(maxp, 2)))

    opt_name, lr, l2 = opt
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt_name, lr, l2))

    def two_steps(m, dtype):
        m.optimizer = runner._build_optimizer(m)
        ls_ = []
        for bt in batches[:2]:
            fd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in bt.items()}
            m.optimizer.zero_grad()
            ls = m.loss(m(fd), labels(bt))
            ls.backward()
            m.optimizer.step()
            ls_.append(ls.item())
        return ls_
    m64 = copy.deepcopy(model).double()
    losses, losses64 = two_steps(model, torch.float32), two_steps(m64, torch.float64)
    # the reference's own fp32 two-step update against its float64 update under conftest.assert_update_close, as the GPU test calls
    # it, with TWICE the deviation (W = Wref + 2 (W32 - W64)): a case whose reference does not pass that cannot hold a port to it
    import conftest
    adaptive, failing = opt_name in ("Adam", "Adagrad"), []
    sd64 = m64.state_dict()
    for k, v in model.state_dict().items():
        if k.startswith("ranker.") or k in zero:
            continue
        w32, w64 = v.detach().numpy().astype(np.float64), sd64[k].numpy()
        exclude = None
        if k.endswith("in_proj_bias"):
            exclude = np.zeros(w32.shape, dtype=bool)
            exclude[w32.shape[0] // 3:2 * (w32.shape[0] // 3)] = True
        try:
            conftest.assert_update_close(w64 + 2 * (w32 - w64), P0[k], w64, what=k, extra_atol=1e-3 * lr if adaptive else 0.0,
                                         outlier_atol=2 * lr if adaptive else 0.0, exclude=exclude)
        except AssertionError as e:
            failing.append(str(e)[:150])
    print("  the reference's own fp32 two-step update, doubled, against float64: %d tensors fail; losses %s / %s" % (len(failing), losses, losses64))
    for f_ in failing[:6]:
        print("    " + f_)
    assert not failing, (name, failing)
    for k, v in model.state_dict().items():
        if not k.startswith("ranker."):
            out["%s/%s" % (opt_name, k)] = prm_np.keep(v.detach().numpy())
    out[opt_name + "_losses"] = np.array(losses, dtype=np.float32)
    out[opt_name + "_hyper"] = np.array([lr, l2], dtype=np.float64)
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 768 * 1024, (name, size)
    print("wrote", path, size >> 10, "KiB")


# Conditioning, chosen so that the REFERENCE's own fp32 run meets the two-step update check against its own float64 run with twice
# its deviation (asserted in make_case); a case where it does not cannot hold anyone else to that check.  What decides it:
#   - the rows of a list share u_v and the rFF0 bias and differ only through the candidate's vectors.  With the ranker's user and item
#     tables scaled alike (x 30) the shared part dominates, the values and keys of a list are nearly equal, and the softmax backward
#     dS = P (dP - sum P dP) subtracts nearly equal numbers: the reference's fp32 gradients in front of the first block's attention
#     then deviate 2e-5 to 1e-4 of their largest entry from float64, ten times what comes behind it.  ITEM_SCALE = 300 against
#     USER_SCALE = 30 brings that to 1e-5 and below.
#   - learning rates a tenth of the usual ones: the first step then moves the weights (0.01 to 0.3 in size) by a per cent, not by a
#     third, and the second step's gradient is taken where the first-step deviations have not been amplified by the LayerNorms.
ITEM_SCALE, USER_SCALE, FF_SCALE = 300.0, 30.0, 30.0
ADAM, SGD, ADAGRAD = ("Adam", 1e-4, 1e-4), ("SGD", 5e-3, 1e-3), ("Adagrad", 1e-3, 1e-4)
CASES = [
    # name,                              ranker, emb, hidden, H, blocks, P,  N, optimizer, B, seed, history
    ("prm_a_bprmf_e64_h64_4h_2b_3p4",    "BPRMF",  64, 64, 4, 2,  3,  4, ADAM,     7, 81),
    ("prm_b_bprmf_e16_h16_1h_1b_1p1",    "BPRMF",  16, 16, 1, 1,  1,  1, SGD,      1, 82),
    ("prm_c_bprmf_e32_h32_2h_4b_20p20",  "BPRMF",  32, 32, 2, 4, 20, 20, ADAGRAD, 33, 83),
    ("prm_d_sasrec_e16_h64_4h_1b_2p3",   "SASRec", 16, 64, 4, 1,  2,  3, SGD,      5, 84, 5),
]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--only", default="", help="'layers' or a case-name prefix")
    a = ap.parse_args()
    if a.only in ("", "layers"):
        make_layer_devs(a.out)
    for c in CASES:
        if a.only == "" or (a.only != "layers" and c[0].startswith(a.only)):
            print(c[0])
            make_case(a.out, *c)
