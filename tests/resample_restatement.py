"""
NumPy restatement of mrc_pac_store_decode_window_resampled (include/mrc_hip.h), for tests/test_gpu_store_resample.py.  The
intermediate signal y comes from the store's own float64 window at that rate_divisor and mix, which is +0.0 outside the
file; the taps come from mrc_resample_taps; the fold over the taps is a Python loop of vectorised float64 multiply-then-add
(NumPy rounds each product, then each sum: no fused multiply-add).
"""
import numpy as np


def floor_div(a, b):
    return a // b                                    # (Python and NumPy floor; b > 0)


def span(start, window, up, down, W):
    """the intermediate samples output samples [start, start + window) read: (first, last), both inclusive"""
    return floor_div(int(start) * down, up) - W + 1, floor_div((int(start) + window - 1) * down, up) + W


def span_bound(window, up, down, W):
    """one bound on last - first + 1 for every start"""
    return -(-(window - 1) * down // up) + 2 * W


def fold(y, first, start, window, up, down, W, taps):
    """y float64 [..., n]: intermediate samples first, first + 1, ... -> v float64 [..., window], outputs start, start + 1, ...
    v[n] = fold from +0.0 over j ascending of taps[p][j] * y[q - W + 1 + j], q = floor(n down / up), p = n down mod up"""
    n = int(start) + np.arange(window, dtype=np.int64)
    nd = n * down
    q = floor_div(nd, up)
    p = nd - q * up
    at = q - W + 1 - int(first)
    assert at.min() >= 0 and at.max() + 2 * W - 1 < y.shape[-1]
    acc = np.zeros(y.shape[:-1] + (window,), np.float64)
    for j in range(2 * W):
        acc = acc + taps[p, j] * y[..., at + j]
    return acc


def restate(store, files, starts, window, up, down, zeros, rolloff, rate_divisor=1, mix=None, channels=None):
    """the call's float64 result [n][channels][window] from the store's own intermediate windows, read-only inputs"""
    import torch
    from mrcaudiocodec_amd.store import resample_taps
    g = int(np.gcd(up, down))
    up, down = up // g, down // g
    W, taps = resample_taps(up, down, zeros, rolloff)
    n_y = span_bound(window, up, down, W)
    firsts = [span(s, window, up, down, W)[0] for s in starts]
    y = store.decode_window(files, firsts, n_y, channels=channels, dtype=torch.float64, rate_divisor=rate_divisor,
                            mix=mix).cpu().numpy()
    return np.stack([fold(y[i], firsts[i], starts[i], window, up, down, W, taps) for i in range(len(files))])
