"""
CPU checks of the noise-to-mask ratio (mrc_pac_nmr) that need no GPU: the library exports it, the NULL-handle path,
the command line refuses -d with --nmr / --measure and a missing file before any device is touched, and the NumPy
restatement the GPU tests compare with gives the known answer on hand-made blocks.
"""
import ctypes
import types

import numpy as np
import pytest

from oracle import fast

import nmr_restatement as nr


def test_library_exports_nmr():
    from mrcaudiocodec_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mrc_pac_nmr", "mrc_get_nmr_ms"):
        assert hasattr(raw, name)
        assert name in _lib.EXPORTS


def test_null_handle_is_refused():
    from mrcaudiocodec_amd import _lib
    buf = np.zeros(64, np.uint8)
    z = np.zeros(4, np.int64)
    d = np.zeros(4)
    args = [None, 1, buf.ctypes.data, z.ctypes.data, None, z.ctypes.data, z.ctypes.data, z.ctypes.data, d.ctypes.data,
            d.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0, None, None, None]
    assert _lib.lib.mrc_pac_nmr(*args) == _lib.MRC_ERR_INVALID
    assert _lib.lib.mrc_get_nmr_ms(None, d.ctypes.data) == _lib.MRC_ERR_INVALID


@pytest.fixture
def no_device(monkeypatch):
    from mrcaudiocodec_amd import cli

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(cli, "Handle", refuse)
    return cli


@pytest.mark.parametrize("flag", ["--nmr", "--measure"])
def test_cli_refuses_decode_with_nmr(no_device, tmp_path, capsys, flag):
    src = tmp_path / "in.pac"
    src.write_bytes(b"PAC ")
    with pytest.raises(SystemExit) as e:
        no_device.main([str(src), str(tmp_path / "out.wav"), "-d", flag])
    assert e.value.code == 2
    assert "-d decodes" in capsys.readouterr().err


def test_cli_measure_missing_file(no_device, tmp_path, capsys):
    wav = tmp_path / "in.wav"
    wav.write_bytes(b"RIFF")
    (tmp_path / "out_1.5.pac").write_bytes(b"PAC ")
    with pytest.raises(SystemExit) as e:
        no_device.main([str(wav), str(tmp_path / "out_{bps}.pac"), "--bits-per-sample", "1.5,4", "--measure"])
    assert e.value.code == 2
    assert "out_4.pac" in capsys.readouterr().err


def _cp(a, b):
    return types.SimpleNamespace(a=a, b=b, nScaleBits=4, sfBands=fast.bands_for(a, b))


@pytest.mark.parametrize("a,b", [(1024, 1024), (128, 128), (1024, 128)])
def test_restatement_band_without_bits_is_the_source_energy(a, b):
    """A band with bit_alloc 0 decodes to zero lines: its noise is sum 4 X^2 over its lines."""
    rng = np.random.default_rng(a + b)
    cp = _cp(a, b)
    nb, half = cp.sfBands.nBands, (a + b) // 2
    seg = rng.normal(0, 0.2, a + b)
    X = fast.mdct_batch(seg[None], a, b)[0]
    ba = np.full(nb, 6)
    j = nb // 2
    ba[j] = 0
    line_band = np.repeat(np.arange(nb), cp.sfBands.nLines)
    mant = rng.integers(0, 1 << 6, half).astype(np.int32)
    mant[line_band == j] = 0
    p = [dict(scaleFactor=list(rng.integers(0, 16, nb)), bitAlloc=list(ba), mantissa=mant, overallScale=2)]
    Xhat = nr.decoded_lines(p, cp, joint=False)[0]
    lo, hi = cp.sfBands.lowerLine[j], cp.sfBands.upperLine[j] + 1
    assert np.all(Xhat[lo:hi] == 0.0) and np.any(Xhat != 0.0)
    e = nr.entry_from_parsed(seg, cp, Xhat, 48000)
    assert e["noise"][j] == pytest.approx(np.sum(4.0 * X[lo:hi] ** 2), rel=1e-14)
    others = [k for k in range(nb) if k != j]
    assert np.all(np.isfinite(e["mask"])) and np.all(e["mask"] > 0)
    assert np.all(e["r"][others] >= 0)


def test_restatement_exact_decode_has_no_noise_and_silence_gives_minus_inf():
    cp = _cp(1024, 1024)
    seg = np.random.default_rng(3).normal(0, 0.1, 2048)
    X = fast.mdct_batch(seg[None], 1024, 1024)[0]
    e = nr.entry_from_parsed(seg, cp, X, 48000)           # a decode equal to the source lines: no noise at all
    assert np.all(e["noise"] == 0.0) and np.all(e["r"] == 0.0)
    e["b"] = 1024
    s = nr.summarise([e], 1)
    assert s["nmr_max_db"] == -np.inf and s["nmr_total_db"] == -np.inf and s["disturbed_blocks"] == 0 and s["n_blocks"] == 1
    assert nr.summarise([], 2) == dict(nmr_max_db=-np.inf, nmr_total_db=-np.inf, disturbed_blocks=0, n_blocks=0)


def test_restatement_summaries_weigh_by_new_samples():
    # eight short entries of ratio 4 weigh what one long entry of ratio 1 weighs: total = 10 log10(2.5)
    ents = [dict(r=np.array([4.0, 4.0]), b=128) for _ in range(8)] + [dict(r=np.array([0.5, 1.5]), b=1024)]
    s = nr.summarise(ents, 1)
    assert s["nmr_total_db"] == pytest.approx(10 * np.log10(2.5), abs=1e-12)
    assert s["nmr_max_db"] == pytest.approx(10 * np.log10(4.0), abs=1e-12)
    assert s["disturbed_blocks"] == 9 and s["n_blocks"] == 9


def _pac_header(n_ch, rate=48000):
    from mrcaudiocodec_amd import pacfile
    return pacfile.header(pacfile.make_config(sample_rate=rate), n_ch, 0)


def test_sources_are_checked_against_each_header():
    """The library reads nCh rows of the source from the address it is given: a source with other rows than its file's
    header names is refused before anything is staged."""
    from mrcaudiocodec_amd import _lib
    stereo, mono = _pac_header(2), _pac_header(1)
    two, one = np.zeros((2, 4096), np.int16), np.zeros((1, 4096), np.int16)
    with pytest.raises(ValueError, match="file 0 has 2 channel"):
        _lib.nmr_layout([stereo], [one])
    with pytest.raises(ValueError, match="file 1 has 2 channel"):
        _lib.nmr_layout([mono, stereo], [one, one])                    # a valid source behind it does not help
    with pytest.raises(ValueError, match="file 0 has 1 channel"):
        _lib.nmr_layout([mono], [two])
    with pytest.raises(ValueError, match="list"):
        _lib.nmr_layout([stereo, stereo], two)                          # the rows of one array are not two sources
    with pytest.raises(ValueError, match="one source per file"):
        _lib.nmr_layout([stereo, stereo], [two])
    out = _lib.nmr_layout([stereo, mono, stereo], [two, one[0], two])  # the same object is staged once
    data, fo, src, so, st, fr, n_entries = out
    assert src.size == two.size + one.size and so[0] == so[2] and n_entries == 0
    assert list(st) == [4096] * 3 and list(fr) == [4096] * 3


def _wav(path, n_ch, rate=48000, n=2048):
    from mrcaudiocodec_amd import cli
    data = np.zeros((n, n_ch), "<i2").tobytes()
    path.write_bytes(cli.wav_header(n_ch, len(data), rate) + data)


@pytest.mark.parametrize("n_ch,rate", [(1, 48000), (2, 44100)])
def test_cli_measure_refuses_a_wav_that_is_not_the_source(no_device, tmp_path, capsys, n_ch, rate):
    _wav(tmp_path / "in.wav", n_ch, rate)
    (tmp_path / "out.pac").write_bytes(_pac_header(2))
    with pytest.raises(SystemExit) as e:
        no_device.main([str(tmp_path / "in.wav"), str(tmp_path / "out.pac"), "--measure"])
    assert e.value.code == 2
    assert "not its source" in capsys.readouterr().err
