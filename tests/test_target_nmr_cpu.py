"""
CPU-side checks of the encode to a target noise-to-mask ratio: the library exports the entry points and the binding
declares them with the header's argument lists, the rule helper on hand-written tables, and the command line's refusals,
which come before a file is read or a device is touched.  No kernel is launched here.
"""
import math

import pytest

from chain_kit import check_binding, header_args

NAMES = ("mrc_encode_chained_target_nmr_pac", "mrc_dev_encode_chained_target_nmr_pac", "mrc_get_target_ms")


def test_binding_matches_the_header():
    check_binding(NAMES)
    host, dev = header_args(NAMES[0]), header_args(NAMES[1])
    assert dev[:-1] == host and dev[-1] == "void* stream"
    assert host[3] == "double target_nmr_total_db" and host[-1] == "int64_t* total_bytes"
    from mrcaudiocodec_amd import Handle, pacfile
    assert callable(Handle.encode_chained_pac_target_nmr) and callable(pacfile.encode_stream_target_nmr)


def test_rule_on_hand_written_tables():
    from mrcaudiocodec_amd.pacfile import choose_rung
    inf = math.inf
    assert choose_rung([3.0, 1.0, -2.0, -9.0], 0.0) == (2, True)
    assert choose_rung([3.0, 1.0, -2.0, -9.0], 1.0) == (1, True)            # <= is inclusive
    assert choose_rung([3.0, 1.0, -2.0, -9.0], -10.0) == (3, False)         # none met: the top rung
    assert choose_rung([3.0, 1.0, -2.0, -9.0], inf) == (0, True)
    assert choose_rung([3.0, 1.0, -2.0, -9.0], -inf) == (3, False)
    assert choose_rung([-inf, -inf], -300.0) == (0, True)                   # silence meets every finite target
    assert choose_rung([2.0, 2.0, 2.0], 2.0) == (0, True)                   # ties: the smallest index
    assert choose_rung([1.0, 3.0, 0.5], 2.0) == (0, True)                   # not monotone: still the smallest index
    assert choose_rung([5.0, 3.0, 4.0, 1.0], 3.5) == (1, True)
    assert choose_rung([7.0], 0.0) == (0, False)
    with pytest.raises(ValueError):
        choose_rung([1.0], math.nan)
    with pytest.raises(ValueError):
        choose_rung([], 0.0)


def test_cli_refusals_come_before_any_file_or_device(tmp_path, monkeypatch):
    from mrcaudiocodec_amd import cli

    def never(*a, **k):
        raise AssertionError("a refused command line must not read the file or open a device")
    monkeypatch.setattr(cli, "Handle", never)
    monkeypatch.setattr(cli, "read_wav_pcm", never)
    src, dst = str(tmp_path / "missing.wav"), str(tmp_path / "out.pac")
    good = ["--bits-per-sample", "1.5,2.86,4", "--target-nmr", "-3"]
    bad = [good + ["-d"], good + ["--certify"], good + ["--measure"],
           ["--bits-per-sample", "2.86", "--target-nmr", "-3"], ["--target-nmr", "-3"],
           ["--bits-per-sample", "4,2.86", "--target-nmr", "-3"], ["--bits-per-sample", "1.5,1.5", "--target-nmr", "-3"],
           ["--bits-per-sample", "1.5,4", "--target-nmr", "nan"], ["--bits-per-sample", "1.5,4", "--target-nmr", "quiet"],
           ["--bits-per-sample", "1.5,99", "--target-nmr", "-3"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.main([src, dst] + argv)
        assert e.value.code == 2, argv
    with pytest.raises(SystemExit) as e:
        cli.main([src, str(tmp_path / "out_{bps}.pac")] + good)
    assert e.value.code == 2
    for kw in (dict(bits_per_sample="1.5,4", target_nmr="nan"), dict(bits_per_sample="4", target_nmr=0.0),
               dict(bits_per_sample="1.5,4", target_nmr=0.0, out_path="x_{bps}.pac")):
        with pytest.raises(ValueError):
            cli.encode_wav_target_nmr(src, kw.pop("out_path", None), **kw)
    rates, target = cli.check_target_args("1.5, 2.86,4", "-inf", "out.pac")
    assert [v for (_, v) in rates] == [1.5, 2.86, 4.0] and target == -math.inf
