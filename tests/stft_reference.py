"""
The reference of the store's STFT tests (tests/test_store_stft_cpu.py, tests/test_gpu_store_stft.py): a direct DFT in
np.longdouble of the float64 products g * x, its twiddles taken from ONE table of cos and sin of 2 pi j / n_fft at
j = (k n) mod n_fft -- the argument is reduced in integers, so no angle grows with k n -- and the unit in which the tests
state errors,
    u_m = 2^-52 * log2(n_fft) * ||g x_m||_2     per frame m,
the size of the rounding of a float64 transform of n_fft points of that frame, up to a factor of order one.
"""
import numpy as np


def frames_of(x, n_fft, hop, n_frames):
    """x [..., L] -> [..., n_frames][n_fft]: frame m is samples [m hop, m hop + n_fft)"""
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return x[..., idx]


def tables(n_fft, dtype=None):
    """cos and sin of 2 pi j / n_fft for 0 <= j < n_fft in longdouble (dtype: rounded through that type first, the GPU
    test's perturbation)"""
    ang = 2 * np.arccos(np.longdouble(-1)) * np.arange(n_fft, dtype=np.longdouble) / np.longdouble(n_fft)
    c, s = np.cos(ang), np.sin(ang)
    if dtype is not None:
        c, s = c.astype(dtype).astype(np.longdouble), s.astype(dtype).astype(np.longdouble)
    return c, s


def dft(gx, twiddle_dtype=None):
    """gx float64 [frames][n_fft], the rounded products g * x -> (re, im) longdouble [frames][n_fft // 2 + 1] of
    sum_n gx[n] e^{-2 pi i k n / n_fft}"""
    gx = np.asarray(gx, dtype=np.float64)
    n_fft = gx.shape[-1]
    c, s = tables(n_fft, twiddle_dtype)
    idx = (np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None] * np.arange(n_fft, dtype=np.int64)[None, :]) % n_fft
    C, S = c[idx], s[idx]
    g = gx.astype(np.longdouble)
    re = np.stack([(C * row[None, :]).sum(axis=1) for row in g]) if len(g) else np.zeros((0, n_fft // 2 + 1), np.longdouble)
    im = np.stack([-(S * row[None, :]).sum(axis=1) for row in g]) if len(g) else np.zeros((0, n_fft // 2 + 1), np.longdouble)
    return re, im


def unit(gx):
    """u_m per frame: float64 [frames]"""
    gx = np.asarray(gx, dtype=np.float64)
    return 2.0 ** -52 * np.log2(gx.shape[-1]) * np.sqrt(np.square(gx).sum(axis=-1))


def ratio(got_re, got_im, re, im, u):
    """the largest |got - ref| / u over frames and bins (a frame with u == 0: 0 if exact, else inf) -> float"""
    err = np.sqrt(np.square(got_re.astype(np.longdouble) - re) + np.square(got_im.astype(np.longdouble) - im)).max(axis=-1)
    err = err.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(u > 0, err / u, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def numpy_ratio(gx, re=None, im=None):
    """NumPy's own float64 real transform against the reference on the frames gx, in the unit: the largest ratio"""
    gx = np.asarray(gx, dtype=np.float64)
    if re is None:
        re, im = dft(gx)
    z = np.fft.rfft(gx, axis=-1)
    return ratio(z.real, z.imag, re, im, unit(gx))
