"""
CPU-side checks of the constant-quality VBR encode to a file size (mrc_encode_vbr_size_pac): the library exports the entry
points and the binding declares them with the header's argument lists; pacfile.bisect_ceiling states the search rule on the
host and is held against hand-made size tables; the grid is lo + i * step in double; the command line's refusals come before
a file is read or a device is touched, and --vbr-bits-per-sample becomes bytes by the stated formula.  No kernel is launched.
"""
import re

import numpy as np
import pytest

from chain_kit import check_binding, header_args, header_text

NAMES = ("mrc_encode_vbr_size_pac", "mrc_dev_encode_vbr_size_pac", "mrc_get_vbr_size_ms")


def test_binding_matches_the_header():
    from mrcaudiocodec_amd import _lib
    check_binding(NAMES)
    host, dev = header_args(NAMES[0]), header_args(NAMES[1])
    assert dev[:-1] == host and dev[-1] == "void* stream"
    assert host[1:5] == ["double ceiling_lo_db", "double ceiling_step_db", "int n_ceilings", "const int64_t* target_bytes"]
    assert host[-1] == "int64_t* total_bytes"
    # behind the grid and the targets: the VBR call's stream arguments, in its order
    vbr = header_args("mrc_encode_vbr_nmr_pac")
    assert host[5:5 + 13] == vbr[2:2 + 13]
    text = header_text(comments=True)
    assert re.search(r"#define\s+MRC_MAX_CEILINGS\s+256\b", text) and re.search(r"#define\s+MRC_MAX_PROBES\s+9\b", text)
    assert (_lib.MRC_MAX_CEILINGS, _lib.MRC_MAX_PROBES) == (256, 9)
    from mrcaudiocodec_amd import Handle, pacfile
    assert callable(Handle.encode_vbr_size_pac) and callable(Handle.vbr_size_ms)
    assert callable(pacfile.encode_stream_vbr_size) and callable(pacfile.bisect_ceiling)


def _rule(sizes, target):
    """the rule as the issue words it, apart from pacfile's own statement"""
    lo, hi, probed = 0, len(sizes) - 1, [len(sizes) - 1]
    if sizes[hi] > target:
        return hi, False, probed
    while lo < hi:
        mid = (lo + hi) // 2
        probed.append(mid)
        lo, hi = (lo, mid) if sizes[mid] <= target else (mid + 1, hi)
    return hi, True, probed


def test_bisect_ceiling_on_a_monotone_table():
    from mrcaudiocodec_amd.pacfile import bisect_ceiling
    sizes = [900, 800, 700, 600, 500, 400, 300, 200]                  # index 0: the tightest ceiling, the largest file
    assert bisect_ceiling(sizes, 650) == (3, True, [7, 3, 1, 2])
    assert bisect_ceiling(sizes, 600) == (3, True, [7, 3, 1, 2])      # the target equal to a size
    assert bisect_ceiling(sizes, 599) == (4, True, [7, 3, 5, 4])      # one byte below it
    assert bisect_ceiling(sizes, 199) == (7, False, [7])              # below the loosest: not met, the last index
    assert bisect_ceiling(sizes, 200) == (7, True, [7, 3, 5, 6])
    assert bisect_ceiling(sizes, 901) == (0, True, [7, 3, 1, 0])      # above the tightest: index 0
    assert bisect_ceiling(sizes, 0) == (7, False, [7])
    for t in range(150, 950, 7):
        chosen, met, probed = bisect_ceiling(sizes, t)
        assert (chosen, met, probed) == _rule(sizes, t)
        if met:                                                       # monotone: the rule finds the optimum
            assert sizes[chosen] <= t and (chosen == 0 or sizes[chosen - 1] > t)


def test_bisect_ceiling_with_one_ceiling():
    from mrcaudiocodec_amd.pacfile import bisect_ceiling
    assert bisect_ceiling([500], 500) == (0, True, [0])
    assert bisect_ceiling([500], 499) == (0, False, [0])
    with pytest.raises(ValueError):
        bisect_ceiling([], 1)


def test_bisect_ceiling_probes_at_most_nine_of_256():
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.pacfile import bisect_ceiling
    sizes = [100000 - 300 * i for i in range(256)]
    most = 0
    for t in [0, sizes[-1] - 1, sizes[-1], sizes[0], sizes[0] + 1] + list(range(sizes[-1], sizes[0], 997)):
        chosen, met, probed = bisect_ceiling(sizes, t)
        assert (chosen, met, probed) == _rule(sizes, t)
        assert len(probed) <= _lib.MRC_MAX_PROBES and len(set(probed)) == len(probed)
        most = max(most, len(probed))
    assert most == 9                                                  # 1 + log2(256): the bound is reached


def test_bisect_ceiling_on_a_table_that_is_not_monotone():
    from mrcaudiocodec_amd.pacfile import bisect_ceiling
    sizes = [900, 500, 820, 600, 650, 400, 450, 300]
    # 7 fits; mid 3 (600) fits: hi = 3; mid 1 (500) fits: hi = 1; mid 0 (900) does not: lo = 1.  Index 2 (820) is never seen.
    assert bisect_ceiling(sizes, 620) == (1, True, [7, 3, 1, 0])
    # 7 fits; mid 3 (600) does not: lo = 4; mid 5 (400) fits: hi = 5; mid 4 (650) does not: lo = 5 -- though index 1 would fit.
    assert bisect_ceiling(sizes, 520) == (5, True, [7, 3, 5, 4])
    # what met promises: the chosen file fits
    for t in range(250, 950, 11):
        chosen, met, probed = bisect_ceiling(sizes, t)
        assert (chosen, met, probed) == _rule(sizes, t)
        assert not met or sizes[chosen] <= t


def test_the_grid_is_one_multiply_and_one_add():
    from mrcaudiocodec_amd.pacfile import ceiling_grid
    for lo, step, n in ((-30.0, 0.25, 256), (-12.0, 3.0, 8), (-7.3, 0.1, 200), (1e-3, 1.0 / 3.0, 17)):
        g = ceiling_grid(lo, step, n)
        assert g.dtype == np.float64 and g.shape == (n,)
        for i in range(n):
            assert g[i] == np.float64(lo) + np.float64(i) * np.float64(step)       # lo + (double)i * step
            assert g[i] == lo + float(i) * step                                   # the same in Python's doubles
        assert g[0] == lo


def test_bits_per_sample_become_bytes_by_the_stated_formula():
    from mrcaudiocodec_amd import cli
    # header + floor(X * coded_samples * channels / 8) + 4 * chunks
    assert cli.vbr_size_target_bytes(2.0, 30, 12 * 1024, 2, 26) == 30 + 6144 + 104
    assert cli.vbr_size_target_bytes(2.86, 30, 10 * 1024, 1, 11) == 30 + int(np.floor(2.86 * 10240 / 8.0)) + 44
    assert cli.vbr_size_target_bytes(0.0, 30, 10 * 1024, 2, 22) == 30 + 88
    assert cli.vbr_size_target_bytes(1.0, 0, 7, 1, 0) == 0                         # floor(7 / 8)


def test_check_vbr_size_args():
    from mrcaudiocodec_amd import cli
    ok = cli.check_vbr_size_args
    assert ok(vbr_bytes="12345") == (12345, None, (-30.0, 0.25, 256))
    assert ok(vbr_bits_per_sample="2.5", vbr_grid="-12:3:8", out_path="a.pac") == (None, 2.5, (-12.0, 3.0, 8))
    assert ok(vbr_bytes="0") == (0, None, (-30.0, 0.25, 256))
    for kw in (dict(), dict(vbr_grid="-12:3:8"),
               dict(vbr_bytes="10", vbr_bits_per_sample="2"),
               dict(vbr_bytes="10", decode=True), dict(vbr_bytes="10", certify=True), dict(vbr_bytes="10", measure=True),
               dict(vbr_bytes="10", bits_per_sample="2.86"), dict(vbr_bytes="10", target_nmr="-3"),
               dict(vbr_bytes="10", vbr_nmr="0"), dict(vbr_bytes="10", out_path="out_{bps}.pac"),
               dict(vbr_bits_per_sample="2", decode=True), dict(vbr_bits_per_sample="2", vbr_nmr="0"),
               dict(vbr_bytes="-1"), dict(vbr_bytes="1.5"), dict(vbr_bytes="many"),
               dict(vbr_bits_per_sample="nan"), dict(vbr_bits_per_sample="inf"), dict(vbr_bits_per_sample="-1"),
               dict(vbr_bits_per_sample="fast"),
               dict(vbr_bytes="10", vbr_grid="-12:3"), dict(vbr_bytes="10", vbr_grid="-12:0:8"),
               dict(vbr_bytes="10", vbr_grid="-12:-1:8"), dict(vbr_bytes="10", vbr_grid="-12:3:0"),
               dict(vbr_bytes="10", vbr_grid="-12:3:257"), dict(vbr_bytes="10", vbr_grid="nan:3:8"),
               dict(vbr_bytes="10", vbr_grid="-12:inf:8"), dict(vbr_bytes="10", vbr_grid="a:b:c")):
        with pytest.raises(ValueError):
            ok(**kw)


def test_cli_refusals_come_before_any_file_or_device(tmp_path, monkeypatch):
    from mrcaudiocodec_amd import cli

    def never(*a, **k):
        raise AssertionError("a refused command line must not read the file or open a device")
    monkeypatch.setattr(cli, "Handle", never)
    monkeypatch.setattr(cli, "read_wav_pcm", never)
    src, dst = str(tmp_path / "missing.wav"), str(tmp_path / "out.pac")
    for good in (["--vbr-bytes", "5000"], ["--vbr-bits-per-sample", "2"]):
        bad = [good + ["-d"], good + ["--certify"], good + ["--measure"], good + ["--bits-per-sample", "2.86"],
               good + ["--target-nmr", "-3"], good + ["--vbr-nmr", "0"], good + ["--vbr-grid", "0:0:4"],
               [good[0], "nan"], [good[0], "-3"]]
        for argv in bad:
            with pytest.raises(SystemExit) as e:
                cli.main([src, dst] + argv)
            assert e.value.code == 2, argv
        with pytest.raises(SystemExit) as e:
            cli.main([src, str(tmp_path / "out_{bps}.pac")] + good)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main([src, dst, "--vbr-bytes", "5000", "--vbr-bits-per-sample", "2"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main([src, dst, "--vbr-grid", "-12:3:8"])
    assert e.value.code == 2


def test_cli_grid_with_negative_lo_reaches_the_encode(tmp_path, monkeypatch, capsys):
    """"--vbr-grid -12:3:8" as two words: argparse alone takes the value, with its leading minus, for an option."""
    from mrcaudiocodec_amd import cli
    seen = []

    def encode(in_path, out_path, vbr_bytes=None, vbr_bits_per_sample=None, vbr_grid=None, *a, **k):
        seen.append((vbr_bytes, vbr_bits_per_sample, vbr_grid))
        return dict(data=b"", target_bytes=0, chosen_db=0.0, met=True, probes=1, ceiling_ratio=1.0, bits_per_sample=0.0,
                    coded_bits=0, capped_bands=0, nmr_total_db=0.0, nmr_max_db=0.0, disturbed_blocks=0, n_blocks=0)
    monkeypatch.setattr(cli, "encode_wav_vbr_size", encode)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.pac")
    cli.main([src, dst, "--vbr-bytes", "5000", "--vbr-grid", "-12:3:8"])
    cli.main([src, dst, "--vbr-grid=-30:0.25:256", "--vbr-bits-per-sample", "2"])
    cli.main(["--vbr-grid", "-1.5:0.5:4", "--vbr-bytes", "7", src, dst])
    assert seen == [("5000", None, "-12:3:8"), (None, "2", "-30:0.25:256"), ("7", None, "-1.5:0.5:4")]
    assert cli.check_vbr_size_args("5000", None, "-12:3:8", out_path=dst) == (5000, None, (-12.0, 3.0, 8))
    capsys.readouterr()
