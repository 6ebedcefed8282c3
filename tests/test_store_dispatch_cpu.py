"""
Which library entry each combination of arguments of PacStore.decode_window, decode_window_sum and stft_window goes to, and
with which scalar arguments: the table below is written out by hand from the docstrings of those three calls -- the bits of a
window depend on the entry that makes it -- and store.window_entry, the one function that names the entries, is asked on a
store that was never created, with integers standing in for the store's pointer, the output's and the stream.
PacStore._call_window and ._out_tensor are replaced on that store: what they do themselves -- the output's pointer (None for
an empty tensor), the call through the library -- needs a device and is exercised by the GPU tests of the store.
"""
import ctypes as C

import numpy as np
import pytest

import chain_kit as kit
import store_kit

STORE, OUT, STREAM = 0x1000, 0x2000, 0x3000
EACH, MID, LEFT, RIGHT = 3, 0, 1, 2                          # MRC_MIX_*
PCM16, F32, F64 = 0, 1, 2                                    # MRC_WINDOW_*
ZEROS, ROLLOFF = 16, 0.9475                                  # the defaults of resample=
FILES, STARTS = [0, 1], [0, 5]                               # file 0 is stereo, file 1 mono
SUM = dict(files=[[0, 1], [1, 1]], starts=[[0, 5], [7, -3]], gains=[[1.0, 0.5], [2.0, 0.25]], window=16)
STFT = dict(files=FILES, starts=STARTS, n_frames=3, hop=4, n_fft=16)
TELEPHONE = dict(band_gains=[0.0, 1.0, 0.0], band_edges_hz=[0, 300, 3400, 24000])

# (caller, its arguments, the entry, the scalar arguments by their names in the header; ratio_up, ratio_down, ratio_of and
# ir_of: the arrays' contents)
TABLE = [
    # ---- decode_window: ir_index, else speeds, else band_gains, else resample, else mix, else rate_divisor > 1, else the first call
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, dtype="float32", rate_divisor=2, mix="mid", resample=(2, 3),
                           speed_factors=[(1, 1), (11, 10)], speed_index=[1, 0], ir_index=[0, -1], **TELEPHONE),
     "mrc_pac_store_decode_window_reverb",
     dict(rate_divisor=2, mix=MID, n_ratios=2, ratio_up=[2, 20], ratio_down=[3, 33], zeros=ZEROS, rolloff=ROLLOFF, n_bands=3, n_items=2,
          ratio_of=[1, 0], ir_of=[0, -1], window=16, n_channels_out=1, format=F32)),
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, speed_factors=[(9, 10), (1, 1)], speed_index=[0, 1]),
     "mrc_pac_store_decode_window_speeds",
     dict(rate_divisor=1, mix=EACH, n_ratios=2, ratio_up=[10, 1], ratio_down=[9, 1], zeros=ZEROS, rolloff=ROLLOFF, n_bands=0, n_items=2,
          ratio_of=[0, 1], window=16, n_channels_out=2, format=PCM16)),
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, dtype="float64", rate_divisor=2, resample=(2, 3, 8, 0.9),
                           band_gains=np.ones(25)),
     "mrc_pac_store_decode_window_shaped",
     dict(rate_divisor=2, mix=EACH, up=2, down=3, zeros=8, rolloff=0.9, n_bands=25, n_items=2, window=16, n_channels_out=2, format=F64)),
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, mix="left", resample=(4, 6)),
     "mrc_pac_store_decode_window_resampled",
     dict(rate_divisor=1, mix=LEFT, up=2, down=3, zeros=ZEROS, rolloff=ROLLOFF, n_items=2, window=16, n_channels_out=1, format=PCM16)),
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, dtype="float32", rate_divisor=4, mix="right"),
     "mrc_pac_store_decode_window_mix", dict(rate_divisor=4, mix=RIGHT, n_items=2, window=16, format=F32)),
    ("decode_window", dict(files=FILES, starts=STARTS, window=16, rate_divisor=2, resample=(5, 5)),      # (a ratio of 1: no resample)
     "mrc_pac_store_decode_window_reduced", dict(rate_divisor=2, n_items=2, window=16, n_channels_out=2, format=PCM16)),
    ("decode_window", dict(files=[1], starts=[0], window=7),
     "mrc_pac_store_decode_window", dict(n_items=1, window=7, n_channels_out=1, format=PCM16)),
    # ---- decode_window_sum: ir_index, else speeds, else band_gains, else the sum call
    ("decode_window_sum", dict(SUM, dtype="float32", ir_index=[[1, -1], [-1, 0]]),
     "mrc_pac_store_decode_window_reverb",
     dict(rate_divisor=1, mix=EACH, n_ratios=1, ratio_up=[1], ratio_down=[1], zeros=ZEROS, rolloff=ROLLOFF, n_bands=0, n_items=2,
          ratio_of=[0, 0, 0, 0], ir_of=[1, -1, -1, 0], window=16, n_channels_out=2, format=F32)),
    ("decode_window_sum", dict(SUM, rate_divisor=2, mix="mid", resample=(2, 3), speed_factors=[(11, 10), (1, 1)],
                               speed_index=[[0, 1], [1, 1]], **TELEPHONE),
     "mrc_pac_store_decode_window_speeds",
     dict(rate_divisor=2, mix=MID, n_ratios=2, ratio_up=[20, 2], ratio_down=[33, 3], zeros=ZEROS, rolloff=ROLLOFF, n_bands=3, n_items=2,
          ratio_of=[0, 1, 1, 1], window=16, n_channels_out=1, format=PCM16)),
    ("decode_window_sum", dict(SUM, dtype="float64", **TELEPHONE),
     "mrc_pac_store_decode_window_shaped",
     dict(rate_divisor=1, mix=EACH, up=1, down=1, zeros=ZEROS, rolloff=ROLLOFF, n_bands=3, n_items=2, window=16, n_channels_out=2, format=F64)),
    ("decode_window_sum", dict(SUM, channels=2, resample=(3, 2)),
     "mrc_pac_store_decode_window_sum",
     dict(rate_divisor=1, mix=EACH, up=3, down=2, zeros=ZEROS, rolloff=ROLLOFF, n_items=2, window=16, n_channels_out=2, format=PCM16)),
    # ---- stft_window: always its own entry; the list defaults to the one base ratio, ir_of to -1
    ("stft_window", dict(STFT, resample=(2, 3)),
     "mrc_pac_store_stft_window",
     dict(rate_divisor=1, mix=EACH, n_ratios=1, ratio_up=[2], ratio_down=[3], zeros=ZEROS, rolloff=ROLLOFF, n_bands=0, n_items=2,
          ratio_of=[0, 0], ir_of=[-1, -1], n_fft=16, n_frames=3, hop=4, mode=1, n_filters=0, n_channels_out=2, format=F32)),
    ("stft_window", dict(STFT, dtype="float64", output="bank", bank=np.ones((2, 9)), rate_divisor=2, mix="mid",
                         speed_factors=[(1, 1), (9, 10)], speed_index=[1, 1], ir_index=[-1, 1], **TELEPHONE),
     "mrc_pac_store_stft_window",
     dict(rate_divisor=2, mix=MID, n_ratios=2, ratio_up=[1, 10], ratio_down=[1, 9], zeros=ZEROS, rolloff=ROLLOFF, n_bands=3, n_items=2,
          ratio_of=[1, 1], ir_of=[-1, 1], n_fft=16, n_frames=3, hop=4, mode=2, n_filters=2, n_channels_out=1, format=F64)),
]
ARRAYS = ("ratio_up", "ratio_down", "ratio_of", "ir_of")


@pytest.mark.parametrize("caller,kw,entry,want", TABLE, ids=["%s-to-%s" % (row[0], row[2][len("mrc_pac_store_"):]) for row in TABLE])
def test_each_combination_goes_to_its_entry_with_its_scalars(monkeypatch, caller, kw, entry, want):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import _lib, store
    s = store_kit.husk(monkeypatch, n_irs=2)
    asked = []
    s._out_tensor = lambda what, shape, dtype, out, stream: (None, STREAM)      # (no device: the tensor is never looked at)
    s._call_window = lambda rows, who, window, channels, fmt, out, stream, stft=None: asked.append(
        store.window_entry(STORE, rows, who, window, channels, fmt, OUT, stream, stft))
    if "dtype" in kw:
        kw = dict(kw, dtype=getattr(torch, kw["dtype"]))
    getattr(s, caller)(**kw)
    (name, args, _keep), = asked
    assert name == entry
    names = [a.split()[-1].lstrip("*") for a in kit.header_args(entry)]
    assert len(args) == len(names) == len(getattr(_lib.lib, entry).argtypes)
    got = dict(zip(names, args))
    assert (got["s"], got["out"], got["stream"]) == (STORE, OUT, STREAM)
    for key, value in want.items():
        if key in ARRAYS:
            held = np.ctypeslib.as_array(C.cast(got[key], C.POINTER(C.c_int32)), (len(value),))
            assert held.tolist() == value, key
        else:
            assert got[key] == value and type(got[key]) is type(value), key
    # every scalar of the entry is in the table: what is left are the pointers
    assert set(names) - set(want) - {"s", "out", "stream"} <= {"edge_hz", "band_gain", "term_offset", "file", "start", "gain",
                                                               "frame_window", "bank"}


def test_the_table_covers_every_row_of_the_docstrings():
    rows = {(caller, entry) for caller, _, entry, _ in TABLE}
    tail = lambda names: {"mrc_pac_store_decode_window" + n for n in names}
    assert {e for c, e in rows if c == "decode_window"} == tail(["_reverb", "_speeds", "_shaped", "_resampled", "_mix", "_reduced", ""])
    assert {e for c, e in rows if c == "decode_window_sum"} == tail(["_reverb", "_speeds", "_shaped", "_sum"])
    assert {e for c, e in rows if c == "stft_window"} == {"mrc_pac_store_stft_window"}


def test_the_entries_are_named_in_one_place():
    import inspect
    from mrcaudiocodec_amd import store
    code = inspect.getsource(store)
    inside = inspect.getsource(store.window_entry)
    for word in ("lib.mrc_pac_store_decode_window", "lib.mrc_pac_store_stft_window"):
        assert word not in code                              # no direct call: every one goes through window_entry's name
    for entry in {row[2] for row in TABLE}:
        assert inside.count('"%s"' % entry) == 1
        outside = code.replace(inside, "")
        assert '"%s"' % entry not in outside
