"""Stored fp32 deviations for the set attention block problems of tests/test_gpu_setrank.py, FROM THE REFERENCE'S OWN `MAB`
(models/reranker/SetRank.py:29-56), on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_setrank.py [--out DIR]

setrank_mab_dev.npz holds no tensors: <B>_<nq>_<nk>_<d>_<H>_<d_ff>_<shared>_<masked>_<seed>/<tensor> is, for every random problem of
setrank_np.MAB_PROBLEMS and SELF_PROBLEMS (regenerated from its seed, never stored), the deviation of the reference's MAB in float32
from the float64 restatement in tests/setrank_np.py, as largest |difference| / largest |float64 entry|, for Y, dQs, dKs and the twelve
weight and bias gradients (a shared query source is repeated over the lists, as SetRank.py:77 does, and its gradient is the sum).
<key>/f64/<tensor> is the same figure for the reference's MAB in float64: the restatement IS the reference to round-off (asserted
below 1e-12 here and again in tests/test_setrank_cpu.py).  <key>/maxp is the largest attention probability of the problem's least
peaked list as a multiple of the uniform value (lists with more than two valid keys); <key>/mask is how far Y moves, relative to its
largest entry, when the mask is ignored.  The GPU tests hold the kernels to max(2e-5, 4 x the stored fp32 figures).

Asserted here, so that a kernel without the softmax, with the wrong query rows or without the mask cannot pass:
  - every problem with a list of more than two valid keys has maxp > 2;
  - every problem with padding has mask > 100 x the bound its Y is held to.
Inputs are prm_np.random_block's: standard normal rows, in_proj 1.5 / sqrt(d) wide.  At the reference's own init (I ~ N(0, 0.01)) the
induced attention is blind: `blind_attention` measures and asserts that (MAB1's largest probability within 2.5 % of uniform at d = 64,
n = 40; 3.2 to 7.0 x uniform with I x 100), which is why no problem here takes its query rows from that init.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import setrank_np as snp  # noqa: E402


def _reference_mab(W, H, dtype):
    """the reference's MAB carrying the twelve weights -> (forward(Q, K, pad) batch-first, its parameters in WEIGHTS order)"""
    import torch
    from models.reranker.SetRank import MAB
    d, dff = W[2].shape[0], W[6].shape[0]
    mab = MAB(d, H, dff, 0)
    mab.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in zip(snp.TORCH_KEYS, W)})
    mab = mab.to(dtype).train()
    params = [mab.get_parameter(k) for k in snp.TORCH_KEYS]

    def forward(Q, K, pad):
        Kt = K.transpose(0, 1)
        return mab(Q.transpose(0, 1), Kt, Kt, None, pad).transpose(0, 1)
    return forward, params


def blind_attention():
    """the reference's IMSAB at its own init, d = 64, n = 40: MAB1's largest probability as a multiple of uniform, as drawn and x 100"""
    import torch
    from models.reranker.SetRank import IMSAB
    torch.manual_seed(7)
    blk = IMSAB(64, 4, 128, 0)
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((9, 40, 64)))
    out = []
    for scale in (1.0, 100.0):
        W = [blk.MAB1.get_parameter(k).detach().numpy() for k in snp.TORCH_KEYS]
        out.append(snp.largest_probability(blk.I.detach().numpy() * scale, x.numpy(), None, W, 4))
    return out


def make_mab_devs(out_dir):
    import torch
    import make_golden
    make_golden._import_reference()
    torch.set_num_threads(1)   # one summation order for every rerun
    drawn, scaled = blind_attention()
    print("induced attention at the reference's init: largest probability %.4f x uniform; with I x 100: %.2f x uniform" % (drawn, scaled))
    assert abs(drawn - 1.0) < 0.025 and 3.2 <= scaled <= 7.0, (drawn, scaled)
    out = {"blind/drawn": np.float64(drawn), "blind/scaled": np.float64(scaled)}
    for prob_id in snp.MAB_PROBLEMS + snp.SELF_PROBLEMS:
        key, H = snp.mab_key(*prob_id), prob_id[4]
        prob = snp.problem(prob_id)
        Qs, Ks, pad, W, _ = prob
        for dtype, prefix in ((torch.float32, ""), (torch.float64, "f64/")):
            fwd, params = _reference_mab(W, H, dtype)
            for name, v in snp.deviation(snp.run_module(fwd, params, prob, dtype), prob, H).items():
                out["%s/%s%s" % (key, prefix, name)] = np.float64(v)
                assert prefix == "" or v < 1e-12, (prob_id, name, v)
        maxp = snp.largest_probability(Qs, Ks, pad, W, H)
        if maxp is not None:
            assert maxp > 2.0, (prob_id, maxp)
            out[key + "/maxp"] = np.float64(maxp)
        if pad is not None and pad.sum() > 0:
            moved, bound = snp.mask_matters(Qs, Ks, pad, W, H), snp.stored_bound(out, key + "/Y")[0]
            assert moved > 100 * bound, (prob_id, moved, bound)
            out[key + "/mask"] = np.float64(moved)
    path = os.path.join(out_dir, "setrank_mab_dev.npz")
    np.savez_compressed(path, **out)
    worst = max((float(v), k) for k, v in out.items() if k.split("/")[1] in ("Y",) + snp.GRAD_NAMES)
    print("wrote", path, os.path.getsize(path) >> 10, "KiB; largest fp32 deviation %.2e (%s)" % worst)


# ---- the model cases, FROM THE REFERENCE ITSELF (models/reranker/SetRank.py, models/BaseRerankerModel.py, helpers/BaseRunner.py) -------
# Conditioning.  The ranker tables, rFF0 / rFF1 and every out_proj are scaled as make_golden_prm.py scales them, for its reasons (its
# header: the candidates' vectors must outweigh what the rows of a list share; learning rates a tenth of the usual ones).  What is new:
#   - I is drawn N(0, 0.01) and the induced attention is blind at that size (blind_attention above), so every block's I is x I_SCALE
#     = 100 after the init stream is recorded; the test applies the stored factor.
#   - each MAB's in_proj_weight is then x 1.25^j with the smallest j that brings the least peaked list's largest probability to
#     PEAK = 2.2 x uniform on the first batch (MAB1 over the list's valid slots, MAB2 over the 20 rows of h); one float32 product per
#     tensor.  Just above the 2 x the tests ask for, and no further: the least peaked list of these cases has three valid keys, where
#     3 x uniform is a probability of 1 -- a first version of this generator scaled until 3 x, which saturates every softmax row of
#     such a list, leaves its backward nothing to carry (whole two-step moves of 6e-6, which the reference's own fp32 run then missed
#     against its float64 run under SGD in cases c and d) and makes the loss gradient magnify the forward's round-off.
#   - what decided the learning rates: make_golden_prm.py's rates throughout.  With PEAK = 2.2 the reference's own fp32 two-step
#     update, doubled, meets its float64 update (asserted in make_case) for every tensor of all four cases as first written.
I_SCALE, PEAK = 100.0, 2.2


def make_case(out_dir, name, ranker, kind, emb, hidden, H, blocks, P, N, opt, B, seed, history=0):
    import copy
    import importlib
    import tempfile
    from types import SimpleNamespace
    import yaml
    import make_golden
    import make_golden_prm as mgp
    import prm_np
    torch, _, BaseRunner = make_golden._import_reference()
    from models.reranker.SetRank import SetRankGeneral, SetRankSequential
    torch.set_num_threads(1)
    seq = ranker == "SASRec"
    n_users, n_items, n = 40, 60, P + N
    rng = np.random.default_rng(seed)
    config = dict(emb_size=emb, num_layers=1, num_heads=2, history_max=99) if seq else dict(emb_size=emb)
    args = SimpleNamespace(device=torch.device("cpu"), model_path="", buffer=1, num_neg=1, dropout=0, test_all=0, loss_n="BPR",
                           emb_size=emb, train_max_pos_item=P, train_max_neg_item=N, test_max_pos_item=P, test_max_neg_item=N,
                           ranker_name=ranker, ranker_config_file=ranker + ".yaml", ranker_model_file="ranker.pt", tuneranker=0,
                           n_blocks=blocks, num_heads=H, num_hidden_unit=hidden, history_max=history, setrank_type=kind)
    corpus = SimpleNamespace(n_users=n_users, n_items=n_items)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            folder = "model/%sImpression" % ranker
            os.makedirs(folder)
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
                        p_.mul_(mgp.ITEM_SCALE if p_.shape[0] == n_items else mgp.USER_SCALE)
            R = {k: v.detach().numpy().copy() for k, v in rk.state_dict().items()}
            torch.save(rk.state_dict(), folder + "/ranker.pt")
            with open(folder + "/" + ranker + ".yaml", "w") as f:
                yaml.safe_dump(config, f)
            torch.manual_seed(seed)
            model = (SetRankSequential if seq else SetRankGeneral)(args, corpus)
            head0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if not k.startswith("ranker.")}
            # the reference's head init re-draws the ranker it has just loaded (self.apply reaches self.ranker); the port loads the
            # checkpoint again afterwards, and so does this generator before anything is recorded
            model.ranker.load_model(folder + "/ranker.pt")
        finally:
            os.chdir(here)
    out = {"meta": np.array([n_users, n_items, emb, hidden, H, blocks, P, N, B, seed, int(seq), history], dtype=np.int64),
           "ranker": np.array(ranker), "ranker_yaml": np.array(yaml.safe_dump(config)), "setrank_type": np.array(kind),
           "state_keys": np.array(list(model.state_dict().keys()))}
    for k, v in R.items():
        out["R/" + k] = v
    for k, v in head0.items():
        out["I0/" + k] = v

    ds = model.Dataset.__new__(model.Dataset)
    ds.model, ds.corpus, ds.phase, ds.pos_len, ds.neg_len = model, corpus, "train", P, N

    def batch(single=False):
        pos, neg, pl, nl = mgp._lists(rng, B, P, N, n_items, single)
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

    valid = ~batches[0]["padding_mask"].numpy()
    pad8 = (~valid).astype(np.uint8)
    scale = {}

    def rescale(key, factor):
        """P[key] = float32(init stream x factor): one exact product, whatever was tried before"""
        scale[key] = np.float32(factor)
        with torch.no_grad():
            model.get_parameter(key).copy_(torch.from_numpy((head0[key] * np.float32(factor)).astype(np.float32)))

    def block_input(l):
        seen = []
        hook = model.encoder[l].register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().transpose(0, 1).numpy().copy()))
        with torch.no_grad():
            model(batches[0])
        hook.remove()
        return seen[0]

    def weights(prefix):
        return [model.get_parameter(prefix + k).detach().numpy() for k in snp.TORCH_KEYS]
    for k in ("rFF0.weight", "rFF1.weight"):
        rescale(k, mgp.FF_SCALE)
    maxp = np.zeros((blocks, 2))
    for l in range(blocks):
        pre = "encoder.%d." % l
        mabs = ("MAB1", "MAB2") if kind == "IMSAB" else ("MAB1",)
        for mab in mabs:
            rescale(pre + mab + ".attn.out_proj.weight", 30.0)
        if kind == "IMSAB":
            rescale(pre + "I", I_SCALE)
        for j, mab in enumerate(mabs):
            f = 1.0
            while True:
                rescale(pre + mab + ".attn.in_proj_weight", f)
                x = block_input(l)
                if kind == "MSAB":
                    mp = snp.largest_probability(x, x, pad8, weights(pre + "MAB1."), H)
                elif mab == "MAB1":
                    mp = snp.largest_probability(model.get_parameter(pre + "I").detach().numpy(), x, pad8, weights(pre + "MAB1."), H)
                else:
                    h = snp.mab_forward(model.get_parameter(pre + "I").detach().numpy(), x, pad8, weights(pre + "MAB1."), H)
                    mp = snp.largest_probability(x, h, None, weights(pre + "MAB2."), H)
                if mp is None or mp >= PEAK:
                    break
                f *= 1.25
            maxp[l, j] = 0.0 if mp is None else mp
            assert mp is None or mp > 2.0, (name, l, mab, mp)
    out["scale_keys"], out["scale_vals"], out["maxp"] = np.array(list(scale)), np.array(list(scale.values()), np.float32), maxp
    P0 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    derived = snp.scale_state({k: v for k, v in P0.items() if k.startswith("ranker.")} | head0, out)
    for k, v in P0.items():
        assert derived[k].tobytes() == v.tobytes(), (name, k)

    def labels(bt):
        col = torch.arange(n)[None, :]
        return torch.where(col < bt["pos_num"][:, None], 1, torch.where((col >= P) & (col < P + bt["neg_num"][:, None]), 0, -1)).long()

    def cast(bt, dtype):
        return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in bt.items()}

    def hooked(m, xs):
        return [blk.register_forward_hook(lambda mod_, a, o: xs.append(o.detach().transpose(0, 1).numpy().copy())) for blk in m.encoder]

    def run(m, bt, dtype):
        xs = []
        hooks = hooked(m, xs)
        m.zero_grad()
        o = m(cast(bt, dtype))
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
        xs_ = []
        hooks = hooked(m, xs_)
        with torch.no_grad():
            p_ = m(cast(bt, dtype))["prediction"].numpy().copy()
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
    # rFF1.bias and what only shifts them (the last block's last norm2.bias) get no gradient.  No dev/ for them.
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
             np.round(maxp, 2).tolist()))

    opt_name, lr, l2 = opt
    runner = BaseRunner(make_golden._runner_args(BaseRunner, opt_name, lr, l2))

    def two_steps(m, dtype):
        m.optimizer = runner._build_optimizer(m)
        ls_ = []
        for bt in batches[:2]:
            m.optimizer.zero_grad()
            ls = m.loss(m(cast(bt, dtype)), labels(bt))
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
        try:
            conftest.assert_update_close(w64 + 2 * (w32 - w64), P0[k], w64, what=k, extra_atol=1e-3 * lr if adaptive else 0.0,
                                         outlier_atol=2 * lr if adaptive else 0.0, exclude=snp.key_bias(k, w32.shape))
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
    assert size <= 600 * 1024, (name, size)
    print("wrote", path, size >> 10, "KiB")


ADAM, SGD, ADAGRAD = ("Adam", 1e-4, 1e-4), ("SGD", 5e-3, 1e-3), ("Adagrad", 1e-3, 1e-4)
CASES = [
    # name,                                      ranker,   type,   emb, hidden, H, blocks, P, N, optimizer, B, seed, history
    ("setrank_a_bprmf_imsab_e32_h64_4h_1b_6p11", "BPRMF",  "IMSAB", 32, 64, 4, 1, 6, 11, ADAM,    7, 91),
    ("setrank_b_bprmf_msab_e16_h32_2h_2b_3p4",   "BPRMF",  "MSAB",  16, 32, 2, 2, 3,  4, ADAGRAD, 5, 92),
    ("setrank_c_sasrec_imsab_e16_h32_2h_2b_2p3", "SASRec", "IMSAB", 16, 32, 2, 2, 2,  3, SGD,     5, 93, 5),
    ("setrank_d_sasrec_msab_e16_h64_4h_1b_2p3",  "SASRec", "MSAB",  16, 64, 4, 1, 2,  3, SGD,     5, 94, 5),
]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--only", default="", help="'mab' or a case-name prefix")
    a = ap.parse_args()
    if a.only in ("", "mab"):
        make_mab_devs(a.out)
    for c in CASES:
        if a.only == "" or (a.only != "mab" and c[0].startswith(a.only)):
            print(c[0])
            make_case(a.out, *c)
