"""
The reference of the store's reverberated windows (tests/test_gpu_store_reverb.py, tests/test_store_reverb_cpu.py): the wet
signal of one term as np.convolve in np.longdouble of a dry window, the error scale of the header's tolerance, NumPy's own
float64 FFT convolution measured against that reference (the figure K is derived from), and the impulse responses of the tests.
NumPy only.
"""
import numpy as np

EPS = 2.0 ** -52


def error_scale(h, w, n_fft):
    """2^-52 log2(N) sum|h| max|w|: the unit the tolerance of a convolved term is stated in (w: every channel of the dry window)"""
    return EPS * np.log2(n_fft) * float(np.abs(h).sum()) * float(np.abs(w).max() if w.size else 0.0)


def wet_reference(h, w):
    """y[t] = sum_j h[j] w[len(h) - 1 + t - j] in np.longdouble, w the dry window [window + len(h) - 1] -> [window]"""
    return np.convolve(np.asarray(w, np.longdouble), np.asarray(h, np.longdouble), "valid")


def wet_numpy_fft(h, w):
    """the same by NumPy's float64 real FFT of the next power of two"""
    n = 1 << int(np.ceil(np.log2(max(w.size, 2))))
    y = np.fft.irfft(np.fft.rfft(w, n) * np.fft.rfft(h, n), n)
    return y[len(h) - 1:w.size]


def numpy_ratio(h, w, n_fft):
    """max |NumPy's FFT convolution - the longdouble reference| in units of error_scale (0 for a silent window)"""
    s = error_scale(h, w, n_fft)
    if s == 0.0:
        return 0.0
    return float(np.abs(wet_numpy_fft(h, w).astype(np.longdouble) - wet_reference(h, w)).max()) / s


def room(length, seed, decay=0.25):
    """exponentially decaying noise of `length` taps, the direct path 1.0 at tap 0: a synthetic room impulse response"""
    t = np.arange(length)
    h = np.random.default_rng(seed).standard_normal(length) * np.exp(-t / max(decay * length, 1.0)) * 0.2
    h[0] = 1.0
    return h


def bank_lengths(B):
    """the impulse-response lengths that cross every edge of a hop of B taps"""
    return [1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 17]
