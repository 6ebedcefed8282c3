"""
NumPy restatement of mrc_pac_store_decode_window_speeds (include/mrc_hip.h), for tests/test_gpu_store_speed.py.  A term's
signal comes from the store's own EXISTING float64 call at that rate_divisor and mix: PacStore.decode_window(resample=the term's
ratio, band_gains=its row), or the call without resample for a ratio that reduces to 1 (+0.0 outside the file, a mono file in
both channels of a two-channel call).  The fold over an item's terms is tests/sum_restatement.py's: a Python loop of float64
multiply-then-add in the terms' order.
"""
import numpy as np

import sum_restatement as SR


def flatten(items):
    """items: per item a list of (file, start, gain, ratio index) -> files, starts, gains, index [terms], offsets [n + 1]"""
    files, starts, gains, offsets = SR.flatten([[(f, s, g) for (f, s, g, _) in it] for it in items])
    return files, starts, gains, np.array([r for it in items for (_, _, _, r) in it], np.int32), offsets


def is_unit(ratio):
    return int(ratio[0]) == int(ratio[1])


def term_windows(store, files, starts, index, window, channels, ratios, zeros, rolloff, rate_divisor=1, mix=None, dtype=None,
                 band_gains=None, band_edges_hz=None):
    """[terms][c][window] in dtype (None: float64): every term through the existing single-ratio call, the terms of one
    ratio in one call of it (its results do not depend on what shares the call)"""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    c = 1 if mix is not None else channels
    out = np.zeros((len(files), c, window), {torch.float64: np.float64, torch.float32: np.float32, torch.int16: np.int16}[dtype])
    for r, ratio in enumerate(ratios):
        sel = np.flatnonzero(np.asarray(index) == r)
        if not sel.size:
            continue
        kw = dict(channels=None if mix is not None else channels, dtype=dtype, rate_divisor=rate_divisor, mix=mix)
        if not is_unit(ratio):
            kw["resample"] = (int(ratio[0]), int(ratio[1]), zeros, rolloff)
        if band_gains is not None:
            kw.update(band_gains=np.asarray(band_gains)[sel], band_edges_hz=band_edges_hz)
        v = store.decode_window(np.asarray(files)[sel], np.asarray(starts)[sel], window, **kw).cpu().numpy()
        assert v.shape == (sel.size, c, window)
        out[sel] = v
    return out


def restate(store, items, window, channels, ratios, zeros, rolloff, rate_divisor=1, mix=None, band_gains=None, band_edges_hz=None):
    """the call's float64 result [n][channels][window]; band_gains: None or [terms][n_bands]"""
    files, starts, gains, index, offsets = flatten(items)
    c = 1 if mix is not None else channels
    v = term_windows(store, files, starts, index, window, channels, ratios, zeros, rolloff, rate_divisor, mix, None, band_gains,
                     band_edges_hz)
    out = np.zeros((len(items), c, window), np.float64)
    for i in range(len(items)):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        out[i] = SR.fold([v[k] for k in range(lo, hi)], gains[lo:hi], (c, window))
    return out
