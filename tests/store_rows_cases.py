"""
The cases of tests/test_gpu_store_rows_parent.py, shared with tools/record_store_rows.py: what the store's window calls --
the nine decode_window entries and stft_window -- give on four small files, bit for bit (sha256 of the output's bytes), with
the call's statistics, and what they refuse, word for word.  The recorder runs them against the library MRC_HIP_LIBRARY names
and writes tests/golden/store_rows_parent.npz; the test runs them against the tree's own and asserts equality.

Files: setting B of tests/settings_kit.py (L 512, S 256) -- stereo Huffman, stereo raw, mono, and the mono file's last block
alone.  The bank: responses of 3 and of 1500 taps (more than one MRC_STORE_REVERB_BLOCK).  Everything a case feeds the
library is made of exact binary fractions, so that no libm stands between a machine and the recorded bits.
"""
import hashlib
import json

import numpy as np

import chain_kit as kit

SID = "B"
SLAB_OPTION = 7                                              # MRC_OPT_STORE_SLAB_SAMPLES
WINDOW = 701
PAST = "past the end of file 0"                               # a start resolved against the store: n_samples[0] + 5
EACH, MID, LEFT, RIGHT = 3, 0, 1, 2
PCM16, F32, F64 = 0, 1, 2


def bank():
    k = np.arange(1500, dtype=np.float64)
    long_ir = np.random.default_rng(11).integers(-1000, 1000, 1500).astype(np.float64) / 1024.0 * ((1500.0 - k) / 1500.0) ** 2
    return [np.array([0.5, -0.25, 0.125]), long_ir]


FRAME_WINDOW = np.minimum(np.arange(16) + 1, 16 - np.arange(16)) / 8.0
BANK_MATRIX = np.array([[0, 0.5, 1, 0.5, 0, 0, 0, 0, 0], [0, 0, 0, 0.25, 0.5, 0.75, 1, 0.5, 0]], np.float64)
TELEPHONE = dict(band_edges_hz=[0, 300, 3400, 24000])        # gains per term: a zero band among them
STFT = dict(n_frames=7, hop=5, n_fft=16, frame_window=FRAME_WINDOW)

# the items: starts at a block boundary and one either side, a negative one, one past the end
ITEMS = dict(files=[0, 1, 2, 3, 0, 1, 2], starts=[1023, 1024, 1025, -37, PAST, 511, 513])
ONE_CHANNEL = dict(files=[2, 3, 2], starts=[1023, -37, 513])
# the rows: 0, 1, 3 and 1 terms
ROWS = dict(files=[0, 2, 1, 3, 0], starts=[1023, -37, 513, 5, PAST], gains=[1.0, 0.5, -2.0, 0.25, 1.5], item_offsets=[0, 0, 1, 4, 5])
ROW_BANDS = dict(TELEPHONE, band_gains=[[0.0, 1.0, 0.5], [1.0, 0.0, 2.0], [1.0, 1.0, 1.0], [0.5, 0.0, 0.0], [0.0, 1.0, 0.0]])
ROW_SPEEDS = dict(speed_factors=[(1, 1), (11, 10)], speed_index=[1, 0, 1, 0, 0])       # base 1 / 1: the unit ratio and 10 / 11
ROW_IRS = dict(ir_index=[1, -1, 0, -1, 0])                   # row 1: the long response; rows 2 and 3: only the short one
DRY = dict(ir_index=[-1, -1, -1, -1, -1])


def success_cases():
    """[(label, method, arguments, every row a slab of its own?)]"""
    item = lambda label, **kw: (label, "decode_window", dict(ITEMS, window=WINDOW, **kw), False)
    cases = [
        item("window", dtype="float64"), item("window int16"),
        item("reduced", rate_divisor=2, dtype="float32"),
        item("mix mid", mix="mid", dtype="float64"), item("mix left at 2", mix="left", rate_divisor=2), item("mix right", mix="right"),
        item("resampled", resample=(2, 3), dtype="float64"), item("resampled mid at 2", resample=(3, 2), rate_divisor=2, mix="mid"),
        ("one channel", "decode_window", dict(ONE_CHANNEL, window=WINDOW, channels=1, dtype="float64"), False),
        item("items shaped", dtype="float64", band_gains=[0.0, 1.0, 0.5], **TELEPHONE),
        item("items at speeds", dtype="float64", speed_factors=[(1, 1), (11, 10)], speed_index=[0, 1, 1, 0, 1, 0, 1]),
        item("items in rooms", dtype="float64", ir_index=[0, -1, 1, 0, 1, -1, 0]),
    ]
    rows = [
        ("sum", {}), ("sum at 2", dict(rate_divisor=2)), ("sum resampled mid", dict(resample=(2, 3), mix="mid")),
        ("shaped", ROW_BANDS), ("shaped left at 2", dict(ROW_BANDS, rate_divisor=2, mix="left", resample=(3, 2))),
        ("speeds", ROW_SPEEDS), ("speeds shaped mid at 2", dict(ROW_SPEEDS, rate_divisor=2, mix="mid", resample=(2, 3), **ROW_BANDS)),
        ("reverb", ROW_IRS), ("reverb at 2", dict(ROW_IRS, rate_divisor=2, **ROW_SPEEDS)), ("reverb short only", dict(ir_index=[-1, -1, 0, 0, -1])),
        ("reverb dry", DRY), ("reverb shaped mid", dict(ROW_IRS, mix="mid", **ROW_BANDS)),
    ]
    for label, kw in rows:
        for slabbed in (False, True):
            cases.append((label + (", a slab per row" if slabbed else ""), "decode_window_sum",
                          dict(ROWS, window=WINDOW, dtype="float64", **kw), slabbed))
    cases.append(("sum int16", "decode_window_sum", dict(ROWS, window=WINDOW), False))
    stfts = [
        ("stft power", dict(ROW_IRS)), ("stft complex at 2", dict(ROW_IRS, output="complex", rate_divisor=2, dtype="float64")),
        ("stft bank", dict(ROW_IRS, output="bank", bank=BANK_MATRIX, dtype="float64", **ROW_SPEEDS)),
        ("stft dry", dict(dtype="float64")), ("stft shaped mid", dict(ROW_IRS, mix="mid", dtype="float64", **ROW_BANDS)),
    ]
    for label, kw in stfts:
        for slabbed in (False, True):
            cases.append((label + (", a slab per row" if slabbed else ""), "stft_window", dict(ROWS, **STFT, **kw), slabbed))
    return cases


# ---- the refused calls, raw: the header's argument names with a value each, then one or two of them changed
DEFAULTS = dict(rate_divisor=1, mix=EACH, up=2, down=3, n_ratios=2, ratio_up=[1, 2], ratio_down=[1, 3], zeros=16, rolloff=0.9475, n_bands=0,
                edge_hz=None, band_gain=None, n_items=1, term_offset=[0, 2], file=[0, 2], start=[0, 9], gain=[1.0, 0.5], ratio_of=[0, 1],
                ir_of=[-1, 0], window=16, n_channels_out=2, format=F64, out="tensor", stream=None, n_fft=16, frame_window=FRAME_WINDOW,
                n_frames=3, hop=5, mode=1, n_filters=0, bank=None)
OWN = {"": dict(n_items=2), "_reduced": dict(n_items=2), "_mix": dict(n_items=2, mix=MID), "_resampled": dict(n_items=2),
       "_shaped": dict(n_bands=2, edge_hz=[0.0, 1000.0, 8000.0], band_gain=[[1.0, 0.5], [2.0, 1.0]])}
DTYPES = dict(ratio_up=np.int32, ratio_down=np.int32, ratio_of=np.int32, ir_of=np.int32, term_offset=np.int64, file=np.int64,
              start=np.int64, edge_hz=np.float64, band_gain=np.float64, gain=np.float64, frame_window=np.float64, bank=np.float64)
ITEM_ENTRIES, ROW_ENTRIES, LIST_ENTRIES = ("", "_reduced", "_mix", "_resampled"), ("_sum", "_shaped", "_speeds", "_reverb", "stft"), ("_speeds", "_reverb", "stft")
ALL = ITEM_ENTRIES + ROW_ENTRIES
BANDS2 = dict(n_bands=2, edge_hz=[0.0, 1000.0, 8000.0], band_gain=[[1.0, 0.5], [2.0, 1.0]])
HUGE = 1 << 40


def entry_name(entry):
    return "mrc_pac_store_stft_window" if entry == "stft" else "mrc_pac_store_decode_window" + entry


def takes(entry, *names):
    have = {a.split()[-1].lstrip("*") for a in kit.header_args(entry_name(entry))}
    return all(n in have for n in names)


def refused_cases():
    """[(label, entry, changes, with a bank?)]: one bad argument per check for every entry that reaches it, then pairs of
    bad arguments that pin which is named.  A case whose window would be enormous passes no output."""
    singles = [
        ("mix 7", dict(mix=7), ALL), ("two channels under a mix", dict(mix=MID, n_channels_out=2), ALL),
        ("no ratios", dict(n_ratios=0), LIST_ENTRIES), ("nine ratios", dict(n_ratios=9), LIST_ENTRIES),
        ("up 0", dict(up=0), ALL), ("down 0", dict(down=0), ALL), ("up above 8 down", dict(up=9, down=1), ALL),
        ("a ratio of 1", dict(up=2, down=2, n_channels_out=1, file=[2, 2]), ("_resampled",)),
        ("zeros 0", dict(zeros=0), ("_resampled", "_sum", "_shaped")), ("rolloff 0.3", dict(rolloff=0.3), ("_resampled", "_sum", "_shaped")),
        ("n_items -1", dict(n_items=-1), ALL), ("no term_offset", dict(term_offset=None), ROW_ENTRIES),
        ("term_offset from 1", dict(term_offset=[1, 2]), ROW_ENTRIES),
        ("term_offset decreases", dict(n_items=2, term_offset=[0, 2, 1]), ROW_ENTRIES),
        ("no file", dict(file=None), ALL), ("no gain", dict(gain=None), ROW_ENTRIES), ("a gain is nan", dict(gain=[1.0, float("nan")]), ROW_ENTRIES),
        ("no ratio_up", dict(ratio_up=None), LIST_ENTRIES), ("a ratio's up is 0", dict(ratio_up=[1, 0]), LIST_ENTRIES),
        ("a ratio of 9", dict(ratio_up=[1, 9], ratio_down=[1, 1]), LIST_ENTRIES), ("a ratio's zeros", dict(zeros=65), LIST_ENTRIES),
        ("ratio_of 5", dict(ratio_of=[0, 5]), LIST_ENTRIES), ("ratio_of -1", dict(ratio_of=[-1, 0]), LIST_ENTRIES),
        ("300 bands", dict(BANDS2, n_bands=300), ("_shaped",) + LIST_ENTRIES), ("no bands in the shaped call", dict(n_bands=0), ("_shaped",)),
        ("no edges", dict(BANDS2, edge_hz=None), ("_shaped",) + LIST_ENTRIES),
        ("edges do not increase", dict(BANDS2, edge_hz=[0.0, 9000.0, 8000.0]), ("_shaped",) + LIST_ENTRIES),
        ("a band gain is inf", dict(BANDS2, band_gain=[[1.0, 0.5], [float("inf"), 1.0]]), ("_shaped",) + LIST_ENTRIES),
        ("edges without bands", dict(edge_hz=[0.0, 1000.0]), LIST_ENTRIES),
        ("divisor 3", dict(rate_divisor=3), ALL), ("window -1", dict(window=-1), ALL),
        ("window above 2^40", dict(window=HUGE + 1, out=None), ALL), ("three channels", dict(n_channels_out=3), ALL),
        ("format 9", dict(format=9), ALL), ("format int16 in the stft", dict(format=PCM16), ("stft",)),
        ("no out", dict(out=None), ALL), ("file 99", dict(file=[0, 99]), ALL), ("file -1", dict(file=[-1, 0]), ALL),
        ("a stereo file in one channel", dict(n_channels_out=1), ALL),
        ("no ir_of", dict(ir_of=None), ("_reverb", "stft")), ("ir_of 5", dict(ir_of=[0, 5]), ("_reverb", "stft")),
        ("ir_of -2", dict(ir_of=[-2, 0]), ("_reverb", "stft")),
        ("window and pre-roll above 2^40", dict(window=HUGE, ir_of=[-1, 1], out=None), ("_reverb",)),
        ("rows and pre-roll above 2^40", dict(n_frames=HUGE - 15, hop=1, ir_of=[-1, 1]), ("stft",)),
        ("n_fft 22", dict(n_fft=22), ("stft",)), ("no frame window", dict(frame_window=None), ("stft",)),
        ("frames -1", dict(n_frames=-1), ("stft",)), ("hop 0", dict(hop=0), ("stft",)),
        ("rows above 2^40", dict(n_frames=HUGE, hop=1, out=None), ("stft",)), ("mode 3", dict(mode=3), ("stft",)),
        ("filters without the bank mode", dict(n_filters=2), ("stft",)), ("the bank mode without a bank", dict(mode=2, n_filters=2), ("stft",)),
    ]
    # (an entry is asked where its header has every argument the case changes)
    cases = [(label, e, change, True) for label, change, entries in singles for e in entries if takes(e, *change)]
    cases += [("ir_of without a bank", e, {}, False) for e in ("_reverb", "stft")]
    pairs = [
        ("mix before bands", "_shaped", dict(mix=7, n_bands=300)), ("gain before ratio_of", "_speeds", dict(gain=[float("inf"), 1.0], ratio_of=[0, 5])),
        ("n_fft before ir_of", "stft", dict(n_fft=22, ir_of=[0, 5])), ("out before the stereo file", "", dict(n_channels_out=1, out=None)),
        ("the stereo file before out", "_reverb", dict(n_channels_out=1, out=None)), ("divisor before window", "_reduced", dict(rate_divisor=3, window=-1)),
        ("window before term_offset", "_reverb", dict(window=-1, term_offset=None)), ("term_offset before window", "_speeds", dict(window=-1, term_offset=None)),
        ("edges without bands before mix", "_speeds", dict(edge_hz=[0.0, 1000.0], mix=7)), ("up before n_items", "_sum", dict(up=0, n_items=-1)),
        ("format before the file", "", dict(format=9, file=[0, 99])), ("ir_of before out", "_reverb", dict(ir_of=[0, 5], out=None)),
        ("divisor before channels", "_sum", dict(rate_divisor=3, n_channels_out=3)), ("the stft's format before mix", "stft", dict(format=PCM16, mix=7)),
        ("the ratio before the band gain", "_speeds", dict(BANDS2, ratio_up=[1, 0], band_gain=[[1.0, 0.5], [float("nan"), 1.0]])),
        ("out before rows and pre-roll", "stft", dict(n_frames=HUGE - 15, hop=1, ir_of=[-1, 1], out=None)),
        ("channels under a mix before the ratio", "_resampled", dict(mix=LEFT, n_channels_out=2, up=0)),
    ]
    return cases + [(label, e, change, True) for label, e, change in pairs]


class Kitchen:
    """the handle, the store with the bank, a store without one and a small output for the raw calls"""

    def __init__(self, files):
        import torch
        import settings_kit as SK
        from mrcaudiocodec_amd.store import PacStore
        self.torch = torch
        self.h = kit.handle(**SK.handle_kwargs(SID))
        self.store, self.bare = PacStore(self.h, files), PacStore(self.h, files)
        self.store.set_impulse_responses(bank())
        self.out = torch.zeros(4096, dtype=torch.float64, device=torch.device("cuda", 0))

    def close(self):
        self.store.close()
        self.bare.close()

    def succeed(self, method, kw, slabbed):
        torch = self.torch
        kw = dict(kw)
        kw["starts"] = [int(self.store.n_samples[0]) + 5 if v == PAST else v for v in kw["starts"]]
        if "dtype" in kw:
            kw["dtype"] = getattr(torch, kw["dtype"])
        slab_was = self.h.get_option(SLAB_OPTION)
        try:
            if slabbed:
                self.h.set_option(SLAB_OPTION, 1)
            out = getattr(self.store, method)(**kw)
        finally:
            self.h.set_option(SLAB_OPTION, slab_was)
        if out.is_complex():
            out = torch.view_as_real(out)
        got = dict(shape=list(out.shape), sha256=hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest())
        got.update({k: v for k, v in self.store.stats().items() if k != "ms"})
        if "ir_index" in kw or method == "stft_window":
            got["reverb_ms_positive"] = sum(self.store.reverb_ms().values()) > 0
        if method == "stft_window":
            got["stft_ms_positive"] = self.store.stft_ms() > 0
        return got

    def refuse(self, entry, change, banked):
        from mrcaudiocodec_amd import _lib
        name = entry_name(entry)
        values = dict(DEFAULTS, **OWN.get(entry, {}))
        values.update(change)
        held, args = [], []
        for a in kit.header_args(name):
            key = a.split()[-1].lstrip("*")
            if key == "s":
                args.append((self.store if banked else self.bare)._s)
                continue
            v = values[key]
            if key == "out":
                v = None if v is None else self.out.data_ptr()
            elif key in DTYPES and v is not None:
                held.append(np.ascontiguousarray(v, dtype=DTYPES[key]))
                v = held[-1].ctypes.data
            args.append(v)
        rc = getattr(_lib.lib, name)(*args)
        return dict(status=int(rc), error=_lib.lib.mrc_last_error(self.h._h).decode() if rc else "")


def load(path):
    """a file of tools/record_store_rows.py -> (the four files' bytes, the results)"""
    z = np.load(path)
    return [z["file%d" % i].tobytes() for i in range(4)], json.loads(str(z["results"]))


def run_all(files):
    """every case against the loaded library -> dict(success={label: ...}, refused={label: ...})"""
    k = Kitchen(files)
    try:
        success = {label: k.succeed(method, kw, slabbed) for label, method, kw, slabbed in success_cases()}
        refused = {"%s: %s" % (entry_name(e), label): k.refuse(e, change, banked) for label, e, change, banked in refused_cases()}
    finally:
        k.close()
    return json.loads(json.dumps(dict(success=success, refused=refused)))
