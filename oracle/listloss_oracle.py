"""CPU ORACLE -- test infrastructure, not product code (see oracle/bprmf_oracle.py header).

Every list-wise loss name of ImpressionModel.loss (the ten rc_list_kind values of rc_list_loss_fwd_bwd) as a FORWARD ONLY, in
torch float64 with per-row masks; the gradient is whatever autograd derives from that forward.  Nothing here restates the
closed-form backward of rechorus_amd/csrc/listwise_loss.hip (oracle/impression_oracle.list_bpr does, for two kinds): a mistake
in that derivation cannot hide in both.  Written from the formulas in include/rechorus_hip.h and the kernel comments and pinned
against the reference's own float64 run: tests/golden/listloss_f64.npz (tests/golden/make_golden_listloss.py).

Per row: valid = target != -1, positives i = valid columns < max_pos, negatives j = valid columns >= max_pos,
a = softmax_i(s) (softmax_i(-s) for 'hard'), b = softmax_j(s), d_ij = s_i - s_j, have_neg = valid[max_pos], H = sum have_neg.
    BPR            rows = -log sum_i a_i sum_j b_j sigmoid(d_ij)                                       loss = mean rows
    BPR...after    rows = sum_i a_i sum_j b_j softplus(-d_ij)                                          loss = mean rows
    BPR...before   rows = sum over ALL n columns c of softplus(-a_c (s_c - sum_j b_j s_j)), a_c = 0 off the positives
                   (every column that is no valid positive adds softplus(0) = log 2)                   loss = mean rows
    BPR...simple   rows = sum_ij softplus(-d_ij), returned UNREDUCED; the gradient is that of rows.sum()
    softmaxCE      p = softmax over the valid columns; rows = -(sum_i log p_i) / #(target == 1)        loss = sum rows have_neg / H
    listnet        t = softmax over the valid columns of the labels; p = softmax over ALL n columns, padding included;
                   rows = -sum_valid t log p  (so a padding column c keeps the gradient p_c)           loss = sum rows have_neg / H
    attention_rank t as listnet, p over the valid columns; rows = -sum t log p - sum_{p != 1} (1 - t) log(1 - p)
                                                                                                       loss = sum rows have_neg / H
softplus is torch's (beta 1, threshold 20: x itself above 20), which is what the reference calls and the kernel restates.
A row without a valid negative makes b = softmax(all -inf) = NaN: the re-weighting kinds return NaN for it, as the reference
does; 'simple' does not use b and gives 0.  H = 0 gives 0 / 0 = NaN.
"""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("BPR", "BPRhard", "BPRafter", "BPRhardafter", "BPRbefore", "BPRhardbefore", "listnet", "softmaxCE", "attention_rank",
         "BPRsimple")
H_NORMALISED = ("listnet", "softmaxCE", "attention_rank")


def forward(loss_n, x, target, max_pos):
    """x [B, n] float64 torch tensor, target [B, n] int64 torch tensor -> loss (0-d; [B] for 'BPR...simple')"""
    B, n = x.shape
    valid = target != -1
    col = torch.arange(n)[None, :]
    pos, neg = valid & (col < max_pos), valid & (col >= max_pos)
    ninf = torch.full_like(x, -np.inf)
    zero = torch.zeros_like(x)
    if "BPR" in loss_n:
        d = x[:, :, None] - x[:, None, :]
        pair = pos[:, :, None] & neg[:, None, :]
        if "simple" in loss_n and "after" not in loss_n and "before" not in loss_n:
            return torch.where(pair, F.softplus(-d), torch.zeros_like(d)).sum(dim=(1, 2))
        sgn = -1.0 if "hard" in loss_n else 1.0
        a = torch.softmax(torch.where(pos, sgn * x, ninf), dim=1)
        b = torch.softmax(torch.where(neg, x, ninf), dim=1)
        if "after" in loss_n:
            inner = (torch.where(pair, F.softplus(-d), torch.zeros_like(d)) * b[:, None, :]).sum(dim=2)
            rows = (inner * a).sum(dim=1)
        elif "before" in loss_n:
            m = (b * torch.where(neg, x, zero)).sum(dim=1, keepdim=True)
            rows = F.softplus(torch.where(pos, -a * (x - m), zero)).sum(dim=1)
        else:
            inner = (torch.where(pair, torch.sigmoid(d), torch.zeros_like(d)) * b[:, None, :]).sum(dim=2)
            rows = -torch.log((inner * a).sum(dim=1))
        return rows.mean()
    have_neg = valid[:, max_pos].to(x.dtype)
    if loss_n == "softmaxCE":
        logp = torch.log_softmax(torch.where(valid, x, ninf), dim=1)
        rows = -torch.where(pos, logp, zero).sum(dim=1) / (target == 1).sum(dim=1).to(x.dtype)
    elif loss_n in ("listnet", "attention_rank"):
        t = torch.softmax(torch.where(valid, target.to(x.dtype), ninf), dim=1)
        masked = x if loss_n == "listnet" else torch.where(valid, x, ninf)
        rows = -(t * torch.where(valid, torch.log_softmax(masked, dim=1), zero)).sum(dim=1)
        if loss_n == "attention_rank":
            p = torch.softmax(masked, dim=1)
            p = torch.where(valid & (p != 1), p, zero)
            rows = rows - ((1.0 - t) * torch.log1p(-p)).sum(dim=1)
    else:
        raise ValueError("Undefined loss function: {}".format(loss_n))
    return (rows * have_neg).sum() / have_neg.sum()


def list_loss(loss_n, pred, target, max_pos):
    """pred [B, n] (any float type; evaluated in float64), target [B, n] in {1, 0, -1} -> (loss, d loss / d pred) as float64 numpy;
    for 'BPR...simple' the loss is the [B] vector of rows and the gradient that of rows.sum()"""
    x = torch.tensor(np.asarray(pred, dtype=np.float64), requires_grad=True)
    loss = forward(loss_n, x, torch.as_tensor(np.asarray(target, dtype=np.int64)), int(max_pos))
    loss.sum().backward()
    return loss.detach().numpy().copy(), x.grad.numpy().copy()
