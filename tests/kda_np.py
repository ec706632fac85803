"""float64 numpy restatement of KDA's RelationalDynamicAggregation (reference models/sequential/KDA.py:265-303) and of its gradients,
written from the formulas (no autograd): the oracle the rc_kda_* kernels are held to, itself held to the goldens recorded from the
reference (tests/test_kda_cpu.py).

One deliberate difference from the reference: a row without any valid position gives a zero context and zero gradients (the
reference's softmax over nothing is NaN)."""
import numpy as np


def freqs(F):
    """the reference's float32 frequency tensor (KDA.py:272-273), first half; the second half is its negative"""
    return (np.linspace(0, 1, F) / 2.).astype(np.float32).astype(np.float64)


def decay_raw(delta_t, freq_real, freq_imag):
    """x [B, L, R] before the clamp, and the cos / sin tables [B, L, F] (KDA.py:276-285: the 2F conjugate-symmetric terms are
    pairwise equal, so the mean over them, halved, is the sum over the first F divided by 2F)"""
    F = freq_real.shape[1]
    w = 2. * np.pi * freqs(F)[None, None, :] * np.asarray(delta_t, np.float64)[:, :, None]
    c, s = np.cos(w), np.sin(w)
    x = (np.einsum('blk,rk->blr', c, freq_real) - np.einsum('blk,rk->blr', s, freq_imag)) / (2. * F)
    return x, c, s


def _ri(target, value, rel, include_val):
    rv = rel[None, None] + value if include_val else np.broadcast_to(rel[None, None], target.shape[:2] + rel.shape)
    return rv, rv * target[:, :, None, :]


def forward(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val=True, parts=False):
    seq, target, rel = (np.asarray(t, np.float64) for t in (seq, target, rel))
    value = np.asarray(value, np.float64) if include_val else None
    freq_real, freq_imag = np.asarray(freq_real, np.float64), np.asarray(freq_imag, np.float64)
    valid = np.asarray(hist) > 0                                       # [B, L]
    rv, ri = _ri(target, value, rel, include_val)                      # [B, C, R, V]
    a = np.einsum('blv,bcrv->bclr', seq, ri)
    a = np.where(valid[:, None, :, None], a, -np.inf)
    m = a.max(axis=2, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.)
    e = np.exp(a - m)
    s = e.sum(axis=2, keepdims=True)
    p = np.divide(e, s, out=np.zeros_like(e), where=s > 0)             # [B, C, L, R]; zeros on a row without a valid position
    x, c, sn = decay_raw(delta_t, freq_real, freq_imag)
    dec = np.where(valid[:, :, None], np.clip(x, 0., 1.), 0.)          # [B, L, R]
    w = p * dec[:, None]
    ctx = np.einsum('bclr,blv->bcrv', w, seq)
    if parts:
        return ctx, dict(valid=valid, rv=rv, ri=ri, p=p, x=x, cos=c, sin=sn, dec=dec, w=w)
    return ctx


def backward(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, d_context, include_val=True):
    """-> dict(dseq, dtarget, dvalue | None, drel, dfreq_real, dfreq_imag); the clamp passes on [0, 1], bounds included (torch)"""
    seq, target, rel, g = (np.asarray(t, np.float64) for t in (seq, target, rel, d_context))
    _, q = forward(seq, hist, delta_t, target, value, rel, freq_real, freq_imag, include_val, parts=True)
    p, dec, w, ri, rv, valid, x = q['p'], q['dec'], q['w'], q['ri'], q['rv'], q['valid'], q['x']
    F = np.asarray(freq_real).shape[1]
    dw = np.einsum('bcrv,blv->bclr', g, seq)                            # d / d w[b, c, l, r]
    dseq = np.einsum('bclr,bcrv->blv', w, g)
    ddec = (p * dw).sum(axis=1)                                         # [B, L, R]
    dp = dw * dec[:, None]
    da = p * (dp - (p * dp).sum(axis=2, keepdims=True))
    dseq += np.einsum('bclr,bcrv->blv', da, ri)
    dri = np.einsum('bclr,blv->bcrv', da, seq)
    drv = dri * target[:, :, None, :]
    dtarget = (dri * rv).sum(axis=2)
    dx = ddec * (valid[:, :, None] & (x >= 0.) & (x <= 1.))
    return dict(dseq=dseq, dtarget=dtarget, dvalue=drv if include_val else None, drel=drv.sum(axis=(0, 1)),
                dfreq_real=np.einsum('blr,blk->rk', dx, q['cos']) / (2. * F),
                dfreq_imag=-np.einsum('blr,blk->rk', dx, q['sin']) / (2. * F))
