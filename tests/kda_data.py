"""Inputs of the KDA aggregation kernel tests, from a seed alone: shared by tests/test_gpu_kda.py, tests/test_kda_cpu.py and by
tests/golden/make_golden_kda.py, which runs the reference's RelationalDynamicAggregation on the same arrays and records its own fp32
deviation from a float64 run (tests/golden/kda_kernel_dev.json).

What the arrays are made to contain: attention logits with a standard deviation of about 1.5 (a softmax that is not flat); id 0 in
the middle of histories and as right padding; with B > 2 one row (row 1) without any valid position; delta_t = 0 in the first
column; frequency tables whose decay has mean 0.5 and a standard deviation of about 0.7 over delta_t, so that it falls below 0,
inside (0, 1) and above 1."""
import numpy as np

# (B, C, L, R, V, F): the floor of the envelope; odd sizes; the reference's default batch shape with R at its bound and more than one
# backward tile of candidates; L, R, V, F at their upper bounds
KERNEL_SHAPES = [(1, 1, 1, 1, 16, 2), (3, 5, 7, 3, 32, 5), (33, 100, 20, 8, 64, 33), (2, 2, 64, 8, 128, 129)]


def case_name(shape, include_val):
    return "b{}_c{}_l{}_r{}_v{}_f{}_val{}".format(*shape, int(include_val))


def freq_tables(rng, R, F):
    """(freq_real, freq_imag) float32 [R, F]: x(delta_t) = (1 / 2F) sum_k (cos re - sin im) has the constant term 0.5 and a spread of
    about 0.7"""
    sigma = 0.7 * 2 * F / np.sqrt(max(F - 1, 1))
    re = rng.normal(0., sigma, size=(R, F))
    im = rng.normal(0., sigma, size=(R, F))
    re[:, 0] = 0.5 * 2 * F
    return re.astype(np.float32), im.astype(np.float32)


def history(rng, B, L, n_items=50, empty_row=True):
    hist = rng.integers(1, n_items, size=(B, L)).astype(np.int64)
    lens = rng.integers(1, L + 1, size=B)
    lens[0] = L
    hist[np.arange(L)[None, :] >= lens[:, None]] = 0            # right padding
    hist[(rng.random((B, L)) < 0.15) & (np.arange(L)[None, :] > 0)] = 0   # id 0 in the middle (never the first position of a row)
    if L > 2:
        hist[0, 1] = 0
    if empty_row and B > 2:
        hist[1] = 0                                             # a row without any valid position
    return hist


def kernel_inputs(shape, seed=0):
    B, C, L, R, V, F = shape
    rng = np.random.default_rng(1000 + seed + B + C + L + R + V + F)
    s = (1.5 / np.sqrt(2. * V)) ** (1. / 3.)                    # <seq, (rel + value) * target> with a spread of about 1.5
    f32 = np.float32
    fre, fim = freq_tables(rng, R, F)
    dt = rng.uniform(0., 20., size=(B, L)).astype(f32)
    dt[:, 0] = 0.
    return dict(seq=rng.normal(0., s, size=(B, L, V)).astype(f32), hist=history(rng, B, L), delta_t=dt,
                target=rng.normal(0., s, size=(B, C, V)).astype(f32), value=rng.normal(0., s, size=(B, C, R, V)).astype(f32),
                rel=rng.normal(0., s, size=(R, V)).astype(f32), freq_real=fre, freq_imag=fim,
                d_context=rng.normal(0., 1., size=(B, C, R, V)).astype(f32))


ARG_ORDER = ("seq", "hist", "delta_t", "target", "value", "rel", "freq_real", "freq_imag")
GRADS = ("dseq", "dtarget", "dvalue", "drel", "dfreq_real", "dfreq_imag")


def clamp_shares(x, valid):
    """shares of the valid (b, l, r) whose raw decay lies below 0, inside (0, 1), above 1"""
    v = x[np.broadcast_to(valid[:, :, None], x.shape)]
    return float((v < 0).mean()), float(((v > 0) & (v < 1)).mean()), float((v > 1).mean())
