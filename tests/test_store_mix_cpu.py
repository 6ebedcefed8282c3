"""
The store's one-channel windows (mrc_pac_store_decode_window_mix, PacStore.decode_window(mix=), cli -d --mix) as far as a CPU
reaches: the NumPy restatement of the mid the GPU tests hold the kernel to (tests/mix_restatement.py: formed on the MDCT
lines, one inverse transform per block) equals the mean of the two channels of tests/reduced_restatement.decode up to
rounding, at D = 1, 2 and 4 on every stereo file of the mix tests; those files are what the tests need; the Python-side
refusals, raised before any library call; the binding of the new function and its constants.
"""
import numpy as np
import pytest

import chain_kit as kit
import mix_restatement as MR
import reduced_restatement as RR

SIDS = MR.KIT_SIDS + ("default",)
_REF = {}


def _refs(sid, f, D):
    """(stereo restatement [2][n], mid restatement [n]) of file f of the setting, computed once, read-only"""
    if (sid, f, D) not in _REF:
        F = MR.files(sid)
        ref, mid = RR.decode(F["files"][f], F["S"], F["blksw"], D), MR.mid_decode(F["files"][f], F["S"], F["blksw"], D)
        ref.setflags(write=False)
        mid.setflags(write=False)
        _REF[(sid, f, D)] = (ref, mid)
    return _REF[(sid, f, D)]


def _stereo(sid):
    F = MR.files(sid)
    return [f for f in range(len(F["files"])) if F["nch"][f] == 2]


# ------------------------------------------------------------------ the restatement, by linearity
@pytest.mark.parametrize("D", MR.DIVISORS)
@pytest.mark.parametrize("sid", SIDS)
def test_mid_on_the_lines_is_the_mean_of_the_two_channels(sid, D):
    """rounding only -- ((l1 + l2) + (l1 - l2)) / 2 against l1, and the transform of a sum against the sum of transforms:
    1e-13 of the stereo file's peak"""
    for f in _stereo(sid):
        ref, mid = _refs(sid, f, D)
        peak = np.abs(ref).max()
        assert mid.shape == ref.shape[1:]
        err = np.abs(mid - 0.5 * (ref[0] + ref[1])).max()
        print("%s file %d D = %d: max |delta| = %.3g of the peak" % (sid, f, D, err / peak))
        assert err <= 1e-13 * peak, (sid, f, D, err / peak)


# ------------------------------------------------------------------ the files are what the tests need
@pytest.mark.parametrize("sid", SIDS)
def test_file_conditions(sid):
    F = MR.files(sid)
    L, S = F["L"], F["S"]
    assert F["nch"] == ([2] if sid == "default" else [2, 2, 1, 1, 2])
    for f in _stereo(sid):
        _, blks = MR.mid_blocks(F["files"][f], S, F["blksw"])
        assert not blks[-1]["joint"] and blks[-1]["ms"] is None and all(b["joint"] for b in blks[:-1])
        assert (blks[-1]["a"], blks[-1]["b"]) == (L, L)
        if F["full"][f]:
            assert {(b["a"], b["b"]) for b in blks} == {(L, L), (L, S), (S, S), (S, L)}
            ms = np.concatenate([b["ms"] for b in blks if b["joint"]])
            n_ms, n_lr = int((ms == 1).sum()), int((ms == 0).sum())
            assert n_ms > 0 and n_lr > 0
            if sid != "default":
                assert 92 <= n_ms <= 99 and 3 <= n_lr <= 10, (sid, f, n_ms, n_lr)
        else:
            assert len(blks) == 1                                 # the non-joint pair alone
        for D in MR.DIVISORS:
            ref, mid = _refs(sid, f, D)
            peak = np.abs(ref).max()
            mid_peak, side_peak = np.abs(mid).max() / peak, np.abs(0.5 * (ref[0] - ref[1])).max() / peak
            assert mid_peak >= 0.5, (sid, f, D, mid_peak)
            assert side_peak >= 1e-3, (sid, f, D, side_peak)       # a call that returned L for mid cannot pass at 1e-12
            if F["full"][f] and sid != "default":
                assert 0.85 <= mid_peak <= 1.0 and side_peak >= 0.010, (sid, f, D, mid_peak, side_peak)
    for f in range(len(F["files"])):
        if F["nch"][f] == 1 and not F["full"][f]:
            _, blks = RR.blocks(F["files"][f], S, F["blksw"])
            assert len(blks) == 1


def test_smallest_and_factor_three_syntheses_are_among_the_files():
    assert MR.files("C")["L"] // 4 == 64 and MR.files("C")["S"] // 4 == 32              # 32-line short blocks at D = 4
    assert MR.files("K")["L"] % 3 == 0 and MR.files("K")["S"] % 3 == 0


# ------------------------------------------------------------------ Python-side refusals
def _husk(monkeypatch):
    import store_kit
    return store_kit.husk(monkeypatch, n_channels=(2,), handle=False)


def test_bad_mix_is_refused_before_any_library_call(monkeypatch):
    s = _husk(monkeypatch)
    for bad in ("side", "Mid", "", 0, 1, True, b"mid", ("mid",)):
        with pytest.raises(ValueError, match="mix must be None"):
            s.decode_window([0], [0], 16, mix=bad)
    for mix in ("mid", "left", "right"):
        for channels in (2, 0, 3, 1.0, True):
            with pytest.raises(ValueError, match="channels must be None or 1"):
                s.decode_window([0], [0], 16, channels=channels, mix=mix)
        with pytest.raises(ValueError, match="rate_divisor"):
            s.decode_window([0], [0], 16, mix=mix, rate_divisor=3)


def test_check_mix():
    from mrcaudiocodec_amd import _lib, store
    assert store.check_mix(None) is None and store.check_mix(None, 2) is None
    assert [store.check_mix(m) for m in ("mid", "left", "right")] == [_lib.MRC_MIX_MID, _lib.MRC_MIX_LEFT, _lib.MRC_MIX_RIGHT]
    assert store.check_mix("mid", 1) == 0 and store.check_mix("right", np.int64(1)) == 2


def test_check_mix_args():
    from mrcaudiocodec_amd import cli
    assert cli.check_mix_args(None, False) is None and cli.check_mix_args(None, True) is None
    assert [cli.check_mix_args(m, True) for m in ("mid", "left", "right")] == ["mid", "left", "right"]
    with pytest.raises(ValueError, match="--mix.*needs -d"):
        cli.check_mix_args("mid", False)
    for bad in ("side", "MID", "", 0):
        with pytest.raises(ValueError, match="--mix"):
            cli.check_mix_args(bad, True)


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--mix", "mid"], "--mix"),
    (["in.wav", "out.pac", "--mix", "left", "--bits-per-sample", "2.5"], "needs -d"),
    (["-d", "in.pac", "out.wav", "--mix", "side"], "is not mid, left or right"),
])
def test_cli_refuses_a_mix_that_makes_no_sense(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


# ------------------------------------------------------------------ the binding
def test_binding_of_the_mix_call():
    from mrcaudiocodec_amd import _lib
    kit.check_binding(("mrc_pac_store_decode_window_mix",))
    args = kit.header_args("mrc_pac_store_decode_window_mix")
    reduced = kit.header_args("mrc_pac_store_decode_window_reduced")
    assert args[1] == "int rate_divisor" and args[2] == "int mix"
    assert args[:2] + args[3:] == [a for a in reduced if a != "int n_channels_out"]
    assert (_lib.MRC_MIX_MID, _lib.MRC_MIX_LEFT, _lib.MRC_MIX_RIGHT) == (0, 1, 2)
    text = kit.header_text()
    for name, value in (("MRC_MIX_MID", 0), ("MRC_MIX_LEFT", 1), ("MRC_MIX_RIGHT", 2)):
        assert ("#define %s" % name) in text and int(text.split("#define %s" % name)[1].split()[0]) == value
