"""
CPU-side checks of the constant-quality VBR encode: the library exports the entry points and the binding declares them with
the header's argument lists; the NumPy restatement of the rule (tests/vbr_restatement.py) writes files the existing host
parser and the oracle's decoder read, every band of them is first-fit, and the measure of the file stays under the ceiling;
the command line's refusals come before a file is read or a device is touched.  No kernel is launched here.
"""
import math

import numpy as np
import pytest

import nmr_restatement as nr
import vbr_restatement as vr
from chain_kit import HOP, check_binding, header_args, to_pcm as _to_pcm

NAMES = ("mrc_encode_vbr_nmr_pac", "mrc_dev_encode_vbr_nmr_pac", "mrc_get_vbr_ms")


def test_binding_matches_the_header():
    check_binding(NAMES)
    host, dev = header_args(NAMES[0]), header_args(NAMES[1])
    assert dev[:-1] == host and dev[-1] == "void* stream"
    assert host[1] == "double ceiling_db" and host[-1] == "int64_t* total_bytes"
    from mrcaudiocodec_amd import Handle, pacfile
    assert callable(Handle.encode_vbr_nmr_pac) and callable(pacfile.encode_stream_vbr_nmr)


def _stream(mono, hops=10, seed=11):
    """config C4 content and a tone common to the channels -> (int16 [nCh][(hops + 1) * HOP], the oracle's block shapes)"""
    from mrcaudiocodec_amd import synth
    from oracle import codec, transient
    chans = [synth.c4_transients(hops, seed=seed + c, period=5)[0] for c in range(1 if mono else 2)]
    pcm = _to_pcm(np.stack(chans) + synth.c1_sine(hops, freq=440.0 + seed, amp=0.1)[:len(chans[0])])
    cp = codec.default_params(nChannels=pcm.shape[0])
    shapes = transient.block_shapes(nr.pcm_to_float(pcm), cp)
    last = max(i for i, s in enumerate(shapes) if s[2] == HOP)
    return pcm, shapes[:last + 1]


_DONE = {}


def _encoded(mono, db):
    if (mono, db) not in _DONE:
        pcm, shapes = _stream(mono)
        r = vr.encode(pcm, shapes, vr.ceiling_ratio(db), num_samples=len(shapes) * HOP)
        _DONE[(mono, db)] = (pcm, shapes, r)
    return _DONE[(mono, db)]


@pytest.mark.parametrize("mono", [False, True])
def test_file_parses_and_decodes(mono):
    from mrcaudiocodec_amd import pacfile
    from oracle import decode as odec
    pcm, shapes, r = _encoded(mono, 0.0)
    assert len({(a, b) for (_, a, b) in shapes}) == 4, "all four block shapes"
    cfg, nch, num_samples, off = pacfile.read_header(r["data"])           # the host parser
    assert nch == pcm.shape[0] and num_samples == len(shapes) * HOP + HOP      # (pacfileThem.py:595-597 pads a multiple)
    chunks = pacfile.scan_chunks(r["data"], off)
    assert len(chunks) == nch * (len(shapes) + 1)
    cp, x = odec.decode_pac(r["data"])
    assert np.atleast_2d(x).shape[0] == nch and np.atleast_2d(x).shape[1] >= sum(b for (_, _, b) in shapes) + HOP
    assert vr.coded_bits(r["data"], nch) == 8 * (len(r["data"]) - off - 4 * len(chunks))


@pytest.mark.parametrize("db", [6.0, 0.0, -6.0, -60.0])
@pytest.mark.parametrize("mono", [False, True])
def test_every_band_is_first_fit_and_the_measure_holds(mono, db):
    pcm, shapes, r = _encoded(mono, db)
    c = vr.ceiling_ratio(db)
    capped = 0
    for blk in r["blocks"]:
        ms = blk["ms"]
        for s, trails in enumerate(blk["trail"]):
            for j, trail in enumerate(trails):
                if ms is not None and ms[j] == 1:
                    if s or not trail:
                        continue
                    # every step but the last exceeds the ceiling on some channel and raises one stream by one step
                    for (n, rl, rr), (n2, _, _) in zip(trail, trail[1:]):
                        assert not (rl <= c and rr <= c)
                        step = [b - a for a, b in zip(n, n2)]
                        assert sorted(step) in ([0, 1], [0, 2]) and (2 not in step or n[step.index(2)] == 0)
                    n, rl, rr = trail[-1]
                    assert tuple(blk["ba"][k][j] for k in range(2)) == n
                    if not (rl <= c and rr <= c):
                        assert n == (16, 16)
                        capped += 1
                    continue
                if not trail:
                    assert blk["ba"][s][j] == 0
                    continue
                assert [n for (n, _) in trail] == vr.candidates(16)[:len(trail)]
                assert all(not (rv <= c) for (_, rv) in trail[:-1])
                n, rv = trail[-1]
                assert blk["ba"][s][j] == n
                if not (rv <= c):
                    assert n == 16
                    capped += 1
    assert capped == r["capped"]
    m = nr.restate(r["data"], vr.source_of(pcm, shapes))
    assert m["n_blocks"] == len(shapes) + 1
    if r["capped"] == 0:
        assert m["nmr_max_db"] <= db + 1e-9
        if db <= 0.0:
            assert m["disturbed_blocks"] == 0
    if db == -60.0:
        assert r["capped"] > 0


def test_mono_bits_do_not_fall_as_the_ceiling_falls():
    prev = None
    for db in (6.0, 0.0, -6.0, -60.0):
        _, _, r = _encoded(True, db)
        bits = [blk["ba"][0] for blk in r["blocks"]]
        if prev is not None:
            for a, b in zip(prev, bits):
                assert np.all(b >= a)
        prev = bits


@pytest.mark.parametrize("mono", [False, True])
def test_infinite_ceiling_and_silence_give_no_bits(mono):
    pcm, shapes = _stream(mono, hops=8)
    r = vr.encode(pcm, shapes, math.inf)
    assert r["capped"] == 0 and all(not np.any(b) for blk in r["blocks"] for b in blk["ba"])
    quiet = np.zeros_like(pcm)
    long_shapes = [(i * HOP, HOP, HOP) for i in range(8)]
    for db in (0.0, -60.0):
        r = vr.encode(quiet, long_shapes, vr.ceiling_ratio(db))
        assert r["capped"] == 0 and all(not np.any(b) for blk in r["blocks"] for b in blk["ba"])


def test_cli_refusals_come_before_any_file_or_device(tmp_path, monkeypatch):
    from mrcaudiocodec_amd import cli

    def never(*a, **k):
        raise AssertionError("a refused command line must not read the file or open a device")
    monkeypatch.setattr(cli, "Handle", never)
    monkeypatch.setattr(cli, "read_wav_pcm", never)
    src, dst = str(tmp_path / "missing.wav"), str(tmp_path / "out.pac")
    good = ["--vbr-nmr", "0"]
    bad = [good + ["-d"], good + ["--certify"], good + ["--measure"], good + ["--bits-per-sample", "2.86"],
           good + ["--target-nmr", "-3"], ["--vbr-nmr", "nan"], ["--vbr-nmr", "quiet"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.main([src, dst] + argv)
        assert e.value.code == 2, argv
    with pytest.raises(SystemExit) as e:
        cli.main([src, str(tmp_path / "out_{bps}.pac")] + good)
    assert e.value.code == 2
    assert cli.check_vbr_args("-inf", out_path="out.pac") == -math.inf and cli.check_vbr_args(" 3 ") == 3.0
