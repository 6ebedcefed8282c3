"""
The reduced-rate store decode (mrc_pac_store_decode_window_reduced, PacStore.decode_window(rate_divisor=), cli -d
--rate-divisor) as far as a CPU reaches: the NumPy restatement the GPU tests hold the kernel to (tests/reduced_restatement.py)
equals the oracle's whole-file decode at D = 1 bit for bit and runs at D = 2 and 4 on every kit file; the fidelity of the
transform chain alone -- short IMDCTs of the first 1 / D of the lines against the band-limited, resampled full-rate
reconstruction; the Python-side refusals, raised before any library call; the rule for synthesis-only block shapes
(mrc_synthesis_shape); the binding of the new functions.
"""
import numpy as np
import pytest

import chain_kit as kit
import reduced_restatement as RR
import settings_kit as SK
from oracle import decode as odec
from oracle.mdct import MDCT
from oracle.window import TransitionWindow

SIDS = ("B", "C", "D", "K")


@pytest.mark.parametrize("nch", [2, 1])
@pytest.mark.parametrize("sid", SIDS)
def test_restatement_at_full_rate_is_the_oracles_decode(sid, nch):
    data = SK.oracle_file(sid, nch, True)["data"]
    L, S = SK.lengths(sid)
    want = SK.oracle_decode(sid, data)
    got = RR.decode(data, S, SK.blksw(sid), 1)
    assert got.shape == want.shape and got.shape[0] == nch and np.array_equal(got, want)
    _, blks = RR.blocks(data, S, SK.blksw(sid))
    assert {(k["a"], k["b"]) for k in blks} == {(L, L), (L, S), (S, S), (S, L)}
    peak = np.abs(want).max()
    for D in (2, 4):
        x = RR.decode(data, S, SK.blksw(sid), D)
        assert x.shape == (nch, want.shape[1] // D) and np.isfinite(x).all()
        # the reduced signal is the same signal, not a scaled one: no resampler's gain, no 1 / D
        assert 0.5 * peak < np.abs(x).max() < 1.5 * peak


def test_smallest_and_factor_three_reduced_shapes():
    assert {(a // 4, b // 4) for a, b in SK.shapes_of("C")} == {(64, 64), (64, 32), (32, 32), (32, 64)}
    assert {(a + b) // 16 for a, b in SK.shapes_of("K")} == {96, 72, 48}          # N' / 4 at D = 4: factors of 3


# ------------------------------------------------------------------ the transform chain alone
L, S, HOPS, SHORT_HOPS = 1024, 128, 12, (3, 4, 8)
BARS_DB = {2: 70.0, 4: 55.0}


def _schedule():
    """[(start, a, b)]: hop h codes L new samples as one block, or as eight short ones for h in SHORT_HOPS; then the flush
    block over L zeros.  a is the b of the block before (the first: the zero prior hop)."""
    bs = []
    for h in range(HOPS):
        bs += [S] * (L // S) if h in SHORT_HOPS else [L]
    bs.append(L)
    out, start, a = [], 0, L
    for b in bs:
        out.append((start, a, b))
        start, a = start + a, b
    return out


def _band_limited_noise(D):
    """Gaussian noise, default_rng(1), brick-wall limited to 0.8 of the Nyquist frequency of the reduced rate, rms 0.1, over the
    HOPS coded hops; a zero hop before it and two behind (the flush block's zeros)"""
    n = HOPS * L
    spec = np.fft.rfft(np.random.default_rng(1).standard_normal(n))
    spec[int(0.8 * n / (2 * D)):] = 0.0
    x = np.fft.irfft(spec, n)
    x *= 0.1 / np.sqrt(np.mean(x * x))
    return np.concatenate([np.zeros(L), x, np.zeros(2 * L)])


def _snr_db(D):
    x = _band_limited_noise(D)
    n = len(x)
    full, reduced = np.zeros(n), np.zeros(n // D)
    for (p, a, b) in _schedule():
        X = MDCT(TransitionWindow(x[p:p + a + b], a, b), a, b)
        full[p:p + a + b] += TransitionWindow(odec.IMDCT(X, a, b), a, b)
        reduced[p // D:(p + a + b) // D] += RR.synthesise(X, a, b, D)
    assert np.abs(full - x)[L:(HOPS + 1) * L].max() < 1e-12                         # TDAC: the full-rate chain reconstructs
    # the yardstick: `full` brick-wall filtered at fs / (2 D) and read at the times D m + (D - 1) / 2, with an FFT
    Y = np.fft.rfft(full)[:n // (2 * D) + 1] * np.exp(2j * np.pi * np.arange(n // (2 * D) + 1) * ((D - 1) / 2.0) / n) / D
    Y[-1] = 0.0
    ref = np.fft.irfft(Y, n // D)
    lo, hi = 3 * L // D, (HOPS - 1) * L // D                                         # away from the ends
    err = reduced[lo:hi] - ref[lo:hi]
    snr = 10 * np.log10(np.sum(ref[lo:hi] ** 2) / np.sum(err ** 2))
    gain = np.sqrt(np.mean(reduced[lo:hi] ** 2) / np.mean(ref[lo:hi] ** 2))
    return snr, gain


@pytest.mark.parametrize("D", [2, 4])
def test_fidelity_of_the_transform_chain(D):
    snr, gain = _snr_db(D)
    print("D = %d: SNR %.2f dB, rms ratio 1 %+.2e" % (D, snr, gain - 1.0))
    assert snr >= BARS_DB[D], (D, snr)
    assert abs(gain - 1.0) < 1e-4, (D, gain)                                          # unscaled


def test_half_sample_offset_is_what_the_documents_say():
    """a pure tone on one long block: the reduced block's samples are the full block's at D m + (D - 1) / 2, not at D m"""
    a = b = 256
    k0 = 9
    X = np.zeros((a + b) // 2)
    X[k0] = 0.3
    full = odec.IMDCT(X, a, b)
    n0 = (b + 1) / 2.0
    for D in (2, 4):
        got = odec.IMDCT(X[:(a + b) // (2 * D)], a // D, b // D)
        t = D * np.arange((a + b) // D) + (D - 1) / 2.0
        want = 2 * 0.3 * np.cos(2 * np.pi / (a + b) * (t + n0) * (k0 + 0.5))
        assert np.abs(got - want).max() < 1e-12
        assert np.abs(got - full[::D]).max() > 1e-3                                   # ... and not the samples at D m


# ------------------------------------------------------------------ Python-side checks
def test_check_rate_divisor_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_rate_divisor_args(None, False) == 1 and cli.check_rate_divisor_args(None, True) == 1
    assert [cli.check_rate_divisor_args(d, True) for d in (1, 2, 4)] == [1, 2, 4]
    with pytest.raises(ValueError, match="--rate-divisor.*needs -d"):
        cli.check_rate_divisor_args(2, False)
    for bad in (0, 3, 8, -2, 2.0, True):
        with pytest.raises(ValueError, match="--rate-divisor"):
            cli.check_rate_divisor_args(bad, True)


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--rate-divisor", "2"], "--rate-divisor"),
    (["-d", "in.pac", "out.wav", "--rate-divisor", "3"], "is not 1, 2 or 4"),
])
def test_cli_refuses_a_rate_divisor_that_makes_no_sense(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_bad_rate_divisor_is_refused_before_any_library_call(monkeypatch):
    import store_kit
    s = store_kit.husk(monkeypatch, n_channels=(2,), handle=False)
    for bad in (0, 3, 8, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="rate_divisor must be an int in {1, 2, 4}"):
            s.decode_window([0], [0], 16, rate_divisor=bad)
        with pytest.raises(ValueError, match="rate_divisor must be an int in {1, 2, 4}"):
            s.n_samples_at(bad)
    assert s.n_samples_at(1).tolist() == [6144] and s.n_samples_at(2).tolist() == [3072]
    assert s.n_samples_at(np.int64(4)).tolist() == [1536]


# ------------------------------------------------------------------ the synthesis-shape rule and the binding
def test_synthesis_shape_rule():
    from mrcaudiocodec_amd import _lib
    ok = lambda a, b, D: _lib.lib.mrc_synthesis_shape(a, b, D)
    why = lambda: _lib.lib.mrc_last_error(None).decode()
    for sid in SIDS + ("E",):                                                        # E: the default 1024 / 128
        for (a, b) in SK.shapes_of(sid):
            for D in (1, 2, 4):
                assert ok(a, b, D) == 0, (a, b, D)
    assert ok(32, 32, 1) == 0 and ok(4, 4, 1) == 0 and ok(12, 12, 1) == 0            # no lower limit but the transform's
    assert ok(128, 128, 8) == 0                                                     # the rule, not the store's set of divisors
    for (a, b, D, text) in ((324, 108, 4, "divisible by 4"), (108, 108, 4, "divisible by 4"), (96, 24, 2, "2s and 3s"),
                            (1024, 128, 3, "no multiples of the divisor"), (1024, 1024, 0, "divisor"), (40, 40, 1, "2s and 3s"),
                            (0, 8, 1, "positive"), (6, 8, 1, "divisible by 4")):
        assert ok(a, b, D) == _lib.MRC_ERR_INVALID, (a, b, D)
        assert text in why() and ("rate_divisor %d" % D) in why() and ("(%d,%d)" % (a, b)) in why(), why()
    for (a, b) in ((324, 324), (324, 108), (108, 108), (108, 324)):                  # divides by 2 and not by 4
        assert ok(a, b, 2) == 0 and ok(a, b, 4) == _lib.MRC_ERR_INVALID


def test_binding_of_the_reduced_calls():
    kit.check_binding(("mrc_pac_store_decode_window_reduced", "mrc_synthesis_shape"))
    args = kit.header_args("mrc_pac_store_decode_window_reduced")
    assert args[1] == "int rate_divisor" and len(args) == len(kit.header_args("mrc_pac_store_decode_window")) + 1
    from mrcaudiocodec_amd import _lib
    assert _lib.lib.mrc_version() == 300
