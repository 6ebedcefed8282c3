"""
The command line's --bits-per-sample checks (cli.encode_wav / cli.main): a ladder without {bps} in the output name,
--certify with several rates and values outside (0, 64] are refused BEFORE the WAV is read or a device is touched -- so
these run without a GPU, on a path that does not exist.
"""
import pytest

from mrcaudiocodec_amd import cli

MISSING = "/nonexistent/dir/in.wav"


def test_values_are_kept_as_written():
    assert cli.parse_bits_per_sample("1.5, 2.86,4") == [("1.5", 1.5), ("2.86", 2.86), ("4", 4.0)]
    assert cli.parse_bits_per_sample(3) == [("3", 3.0)]
    assert cli.ladder_paths("out_{bps}.pac", cli.parse_bits_per_sample("2,2.86")) == ["out_2.pac", "out_2.86.pac"]


@pytest.mark.parametrize("bad", ["0", "-1", "64.5", "nan", "inf", "2,,3", "two", ",".join(["2"] * 17)])
def test_out_of_range_values_are_refused_first(bad):
    with pytest.raises(ValueError):
        cli.encode_wav(MISSING, "out_{bps}.pac", bits_per_sample=bad)


def test_ladder_needs_bps_in_the_output_name():
    with pytest.raises(ValueError, match=r"\{bps\}"):
        cli.encode_wav(MISSING, "out.pac", bits_per_sample="2,2.86,4")


def test_ladder_refuses_certify():
    with pytest.raises(ValueError, match="certify"):
        cli.encode_wav(MISSING, "out_{bps}.pac", bits_per_sample="2,4", certify={})


def test_edges_of_the_range_pass_the_checks():
    # 64 and a tiny positive rate are accepted: the call gets as far as reading the (missing) file
    with pytest.raises(OSError):
        cli.encode_wav(MISSING, "out_{bps}.pac", bits_per_sample="0.001,64")


@pytest.mark.parametrize("argv", [["in.wav", "out.pac", "--bits-per-sample", "2,4"],
                                  ["in.wav", "out_{bps}.pac", "--bits-per-sample", "2,4", "--certify"]])
def test_command_line_refusals(argv):
    with pytest.raises(SystemExit) as e:
        cli.main([MISSING if a == "in.wav" else a for a in argv])
    assert e.value.code == 2


def test_command_line_refuses_out_of_range_values():
    with pytest.raises(ValueError):
        cli.main([MISSING, "out_{bps}.pac", "--bits-per-sample", "2,65"])
