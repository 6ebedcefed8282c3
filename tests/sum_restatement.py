"""
NumPy restatement of mrc_pac_store_decode_window_sum (include/mrc_hip.h), for tests/test_gpu_store_sum.py and
tests/test_store_sum_cpu.py.  A term's signal comes from the store's own EXISTING float64 call at that rate_divisor, mix and
resample (PacStore.decode_window: +0.0 outside the file, a mono file in both channels of a two-channel call); the fold over
an item's terms is a Python loop of float64 multiply-then-add (NumPy rounds each product, then each sum: no fused
multiply-add).
"""
import numpy as np


def fold(vs, gains, shape=None):
    """vs: the terms' float64 signals, one shape; gains: one factor per term -> the left fold from +0.0 in term order of
    gains[k] * vs[k].  shape: of the result when there is no term to take it from."""
    if len(vs) != len(gains):
        raise ValueError("fold: %d signals, %d gains" % (len(vs), len(gains)))
    acc = np.zeros(np.shape(vs[0]) if len(vs) else shape, np.float64)
    for k in range(len(vs)):
        acc = acc + np.float64(gains[k]) * np.asarray(vs[k], np.float64)
    return acc


def flatten(items):
    """items: per item a list of (file, start, gain) -> files, starts, gains [terms], offsets [n + 1]"""
    files = np.array([f for it in items for (f, _, _) in it], np.int64)
    starts = np.array([s for it in items for (_, s, _) in it], np.int64)
    gains = np.array([g for it in items for (_, _, g) in it], np.float64)
    offsets = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(it) for it in items], out=offsets[1:])
    return files, starts, gains, offsets


def restate(store, items, window, channels, rate_divisor=1, mix=None, resample=None):
    """the call's float64 result [n][channels][window]: every term through the existing call, all terms in one call of it
    (its results do not depend on what shares the call), then fold per item"""
    import torch
    files, starts, gains, offsets = flatten(items)
    c = 1 if mix is not None else channels
    if files.size:
        v = store.decode_window(files, starts, window, channels=None if mix is not None else channels, dtype=torch.float64,
                                rate_divisor=rate_divisor, mix=mix, resample=resample).cpu().numpy()
        assert v.shape == (files.size, c, window)
    out = np.zeros((len(items), c, window), np.float64)
    for i in range(len(items)):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        out[i] = fold([v[k] for k in range(lo, hi)], gains[lo:hi], (c, window))
    return out
