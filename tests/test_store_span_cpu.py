"""
The store's terms with spans and fades (mrc_pac_store_decode_window_spans, mrc_pac_store_stft_window_spans,
PacStore.decode_window_sum / stft_window(span_first=, span_len=, fade_in=, fade_out=), store.check_spans, store.concat_spans) as
far as a CPU reaches: the binding against the header and the argument lists of the two entries; every ValueError of check_spans
and concat_spans, raised before any library call; concat_spans' arithmetic on hand-made cases; which entry a call with spans
goes to; the envelope's crossfade property in NumPy, the figure the GPU test's bound rests on.
"""
import numpy as np
import pytest

import chain_kit as kit

SPANS = ["span_first", "span_len", "fade_in", "fade_out"]


def _names(entry):
    return [a.split()[-1].lstrip("*") for a in kit.header_args(entry)]


# ------------------------------------------------------------------ the binding and the header
def test_binding_and_argument_lists_of_the_span_entries():
    names = ("mrc_pac_store_decode_window_spans", "mrc_pac_store_stft_window_spans")
    kit.check_binding(names)
    for new, old in zip(names, ("mrc_pac_store_decode_window_reverb", "mrc_pac_store_stft_window")):
        got, base = _names(new), _names(old)
        at = got.index("ir_of") + 1
        assert got[at:at + 4] == SPANS                               # right after ir_of, in this order
        assert got[:at] + got[at + 4:] == base                        # ... and every argument of the entry, in its order
        decl = kit.header_args(new)[at:at + 4]
        assert all(d.startswith("const int64_t*") for d in decl), decl


# ------------------------------------------------------------------ check_spans
def test_check_spans_gives_flat_int64_arrays_and_broadcasts_a_scalar_fade():
    from mrcaudiocodec_amd.store import MAX_SPAN, check_spans
    assert check_spans(None, None, None, None, (2, 3)) is None
    first, length, fin, fout = check_spans([[0, -5, 7]], [[10, 3, 0]], [[1, 1, 0]], None, (1, 3))
    for a in (first, length, fin, fout):
        assert a.dtype == np.int64 and a.shape == (3,) and a.flags.c_contiguous
    assert first.tolist() == [0, -5, 7] and length.tolist() == [10, 3, 0] and fin.tolist() == [1, 1, 0] and not fout.any()
    with pytest.raises(ValueError, match="at term 2"):               # (a scalar fade reaches the empty span too: 1 + 0 > 0)
        check_spans([[0, -5, 7]], [[10, 3, 0]], 1, None, (1, 3))
    first, length, fin, fout = check_spans([0, -5], [10, 3], 1, np.array([9, 2]), (2,))
    assert fin.tolist() == [1, 1] and fout.tolist() == [9, 2]                      # fade_in + fade_out == span_len is allowed
    first, length, fin, fout = check_spans([-MAX_SPAN, MAX_SPAN], [MAX_SPAN, 0], None, None, (2,))
    assert first.tolist() == [-MAX_SPAN, MAX_SPAN] and length.tolist() == [MAX_SPAN, 0] and not fin.any() and not fout.any()
    assert check_spans(np.float64([2.0]), [3], None, None, (1,))[0].tolist() == [2]   # whole numbers in a float array pass


BAD_SPANS = [
    (dict(span_first=[0, 0]), "span_first and span_len go together, got only span_first"),
    (dict(span_len=[4, 4]), "span_first and span_len go together, got only span_len"),
    (dict(fade_in=2), "fade_in goes with span_first and span_len"),
    (dict(fade_out=[1, 1]), "fade_out goes with span_first and span_len"),
    (dict(span_first=[0], span_len=[4, 4]), r"span_first must have the shape of files \(2,\), got \(1,\)"),
    (dict(span_first=[0, 0], span_len=[[4, 4]]), r"span_len must have the shape of files \(2,\), got \(1, 2\)"),
    (dict(span_first=[0, 0], span_len=[4, 4], fade_in=[1]), r"fade_in must have the shape of files \(2,\) or be a scalar, got \(1,\)"),
    (dict(span_first=[0, 0], span_len=4), r"span_len must have the shape of files \(2,\), got \(\)"),
    (dict(span_first=[0.5, 0], span_len=[4, 4]), "span_first must hold whole numbers"),
    (dict(span_first=[0, 0], span_len=["a", "b"]), "span_len must hold whole numbers"),
    (dict(span_first=[0, 0], span_len=[4, float("nan")]), "span_len must hold whole numbers"),
    (dict(span_first=[0, 0], span_len=[4, 4], fade_out=True), "fade_out must hold whole numbers"),
    (dict(span_first=[0, 0], span_len=[4, -1]), r"span_len must lie in \[0, 2\^40\], got .* span_len -1, .* at term 1"),
    (dict(span_first=[0, 0], span_len=[(1 << 40) + 1, 4]), r"span_len must lie in \[0, 2\^40\], got .* at term 0"),
    (dict(span_first=[0, (1 << 40) + 1], span_len=[4, 4]), r"span_first must lie in \[-2\^40, 2\^40\], got .* at term 1"),
    (dict(span_first=[-(1 << 40) - 1, 0], span_len=[4, 4]), r"span_first must lie in \[-2\^40, 2\^40\], got .* at term 0"),
    (dict(span_first=[0, 0], span_len=[4, 4], fade_in=[0, -1]), "fade_in must not be negative, got .* fade_in -1, .* at term 1"),
    (dict(span_first=[0, 0], span_len=[4, 4], fade_out=-3), "fade_out must not be negative, got .* at term 0"),
    (dict(span_first=[0, 0], span_len=[4, 5], fade_in=3, fade_out=2), "fade_in . fade_out must not exceed span_len, got .* at term 0"),
    (dict(span_first=[0, 0], span_len=[4, 0], fade_in=[4, 1]), "fade_in . fade_out must not exceed span_len, got .* at term 1"),
]


@pytest.mark.parametrize("kw,text", BAD_SPANS)
def test_bad_spans_are_refused_before_any_library_call(monkeypatch, kw, text):
    pytest.importorskip("torch")
    import store_kit
    from mrcaudiocodec_amd.store import check_spans
    full = dict(dict(span_first=None, span_len=None, fade_in=None, fade_out=None), **kw)
    with pytest.raises(ValueError, match="decode_window_sum: " + text):
        check_spans(full["span_first"], full["span_len"], full["fade_in"], full["fade_out"], (2,))
    s = store_kit.husk(monkeypatch)
    with pytest.raises(ValueError, match="decode_window_sum: " + text):
        s.decode_window_sum([0, 1], [0, 5], [1.0, 0.5], 16, item_offsets=[0, 2], **kw)
    with pytest.raises(ValueError, match="stft_window: " + text):
        s.stft_window([0, 1], [0, 5], 3, 5, 16, gains=[1.0, 0.5], item_offsets=[0, 2], **kw)


def test_spans_do_not_go_with_routes_and_come_after_the_calls_own_refusals(monkeypatch):
    pytest.importorskip("torch")
    import store_kit
    s = store_kit.husk(monkeypatch, n_channels=(1, 1))
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs do not go with spans"):
        s.stft_window([0, 1], [0, 5], 3, 5, 16, route_gains=[[1.0], [1.0]], route_irs=[[-1], [-1]], span_first=[0, 0], span_len=[4, 4])
    with pytest.raises(ValueError, match="decode_window_sum: gains must be finite"):
        s.decode_window_sum([[0, 1]], [[0, 5]], [[1.0, float("inf")]], 16, span_first=[0], span_len=[4])


# ------------------------------------------------------------------ which entry a call goes to
def test_a_call_with_spans_goes_to_the_span_entries_and_one_without_does_not():
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import WindowRows, check_spans, window_entry
    files, starts, gains = np.array([0, 1], np.int64), np.array([3, 4], np.int64), np.ones(2)
    spans = check_spans([0, 8], [8, 8], 2, 0, (2,))
    rows = WindowRows(1, None, None, 2, None, None, None, np.array([0, 2], np.int64), files, starts, gains)
    assert rows.spans is None and rows.routes is None
    assert window_entry(1, rows, "decode_window_sum", 16, 2, _lib.MRC_WINDOW_F64, 7, None)[0] == "mrc_pac_store_decode_window_sum"
    name, args, keep = window_entry(1, rows._replace(spans=spans), "decode_window_sum", 16, 2, _lib.MRC_WINDOW_F64, 7, None)
    assert name == "mrc_pac_store_decode_window_spans" and len(args) == len(kit.header_args(name))
    at = [a.split()[-1].lstrip("*") for a in kit.header_args(name)].index("span_first")
    assert list(args[at:at + 4]) == [a.ctypes.data for a in spans] and args[at + 4:] == (16, 2, _lib.MRC_WINDOW_F64, 7, None)
    stft = (16, np.ones(16), 3, 5, _lib.MRC_STFT_POWER, None)
    name, args, keep = window_entry(1, rows._replace(spans=spans), "stft_window", 3, 2, _lib.MRC_WINDOW_F32, 7, None, stft=stft)
    assert name == "mrc_pac_store_stft_window_spans" and len(args) == len(kit.header_args(name))
    assert list(args[at:at + 4]) == [a.ctypes.data for a in spans] and args[at + 4] == 16
    assert window_entry(1, rows, "stft_window", 3, 2, _lib.MRC_WINDOW_F32, 7, None, stft=stft)[0] == "mrc_pac_store_stft_window"


def test_center_moves_the_spans_with_the_starts(monkeypatch):
    pytest.importorskip("torch")
    import store_kit
    from mrcaudiocodec_amd import store
    s = store_kit.husk(monkeypatch)
    seen = {}

    def call(rows, *a, **kw):
        seen["rows"] = rows
        raise KeyError("stop")
    monkeypatch.setattr(s, "_call_window", call)
    monkeypatch.setattr(s, "_out_side", lambda *a, **kw: (2, 1, None))
    for center, shift in ((False, 0), (True, 8)):
        with pytest.raises(KeyError):
            s.stft_window([0, 1], [100, 50], 3, 5, 16, gains=[1.0, 0.5], item_offsets=[0, 2], center=center, span_first=[0, 4],
                          span_len=[4, 9], fade_in=1)
        rows = seen["rows"]
        assert rows.starts.tolist() == [100 - shift, 50 - shift] and rows.spans[0].tolist() == [shift, 4 + shift]
        assert rows.spans[1].tolist() == [4, 9] and rows.spans[2].tolist() == [1, 1] and rows.spans[3].tolist() == [0, 0]
    assert store.MAX_SPAN == 1 << 40


# ------------------------------------------------------------------ concat_spans
def test_concat_spans_lays_pieces_end_to_end():
    from mrcaudiocodec_amd.store import concat_spans
    starts, first, length, fin, fout = concat_spans([[100, 50, 30]], [[1000, 2000, 3000]])
    assert first.tolist() == [[0, 100, 150]] and length.tolist() == [[100, 50, 30]] and not fin.any() and not fout.any()
    assert starts.tolist() == [[1000, 1900, 2850]]                    # the source position that stands at row sample 0
    assert all(a.dtype == np.int64 and a.shape == (1, 3) for a in (starts, first, length, fin, fout))
    # a crossfade: every later piece begins that much before its predecessor ends; the outer ends are not faded
    starts, first, length, fin, fout = concat_spans([[100, 50, 30], [20, 20, 20]], [[1000, 2000, 3000], [0, 0, 0]], crossfade=10)
    assert first.tolist() == [[0, 90, 130], [0, 10, 20]] and length.tolist() == [[100, 50, 30], [20, 20, 20]]
    assert fin.tolist() == [[0, 10, 10]] * 2 and fout.tolist() == [[10, 10, 0]] * 2
    assert starts.tolist() == [[1000, 1910, 2870], [0, -10, -20]]
    assert int(first[0, -1] + length[0, -1]) == 100 + 50 + 30 - 2 * 10             # the row's length
    # ragged rows: a row of one piece has no fade, an empty row and an empty piece are allowed
    starts, first, length, fin, fout = concat_spans([7, 5, 0, 9], [1, 2, 3, 4], crossfade=0, item_offsets=[0, 1, 1, 4])
    assert first.tolist() == [0, 0, 5, 5] and starts.tolist() == [1, 2, -2, -1] and length.tolist() == [7, 5, 0, 9]
    starts, first, length, fin, fout = concat_spans([7, 5, 4, 9], [1, 2, 3, 4], crossfade=2, item_offsets=[0, 1, 1, 4])
    assert fin.tolist() == [0, 0, 2, 2] and fout.tolist() == [0, 2, 2, 0] and first.tolist() == [0, 0, 3, 5]
    e = concat_spans(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64))
    assert all(a.shape == (0, 3) for a in e)


@pytest.mark.parametrize("args,kw,text", [
    (([[4, 4]], [[0]]), {}, "lengths and source_starts must have one shape"),
    (([4, 4], [0, 0]), {}, r"lengths must be \[n\]\[K\], or 1-D with item_offsets"),
    (([[4, 4]], [[0, 0]]), dict(item_offsets=[0, 2]), "with item_offsets, lengths must be 1-D"),
    (([4, 4], [0, 0]), dict(item_offsets=[0, 1]), "end at the number of pieces"),
    (([4, 4], [0, 0]), dict(item_offsets=[1, 2]), "start at 0"),
    (([4, 4], [0, 0]), dict(item_offsets=[0, 2, 1, 2]), "not decrease"),
    (([[4, -1]], [[0, 0]]), {}, "lengths must not be negative, got -1 at piece 1"),
    (([[4, 4]], [[0, 0]]), dict(crossfade=-1), "crossfade must be a whole number >= 0"),
    (([[4, 4]], [[0, 0]]), dict(crossfade=1.5), "crossfade must be a whole number >= 0"),
    (([[4, 4]], [[0, 0]]), dict(crossfade=True), "crossfade must be a whole number >= 0"),
    (([[9, 5, 9]], [[0, 0, 0]]), dict(crossfade=3), "crossfade 3 does not fit piece 1 of 5 samples, which fades over 6"),
    (([[2, 9]], [[0, 0]]), dict(crossfade=3), "crossfade 3 does not fit piece 0 of 2 samples, which fades over 3"),
    (([[9, 2]], [[0, 0]]), dict(crossfade=3), "crossfade 3 does not fit piece 1 of 2 samples"),
])
def test_concat_spans_refusals(args, kw, text):
    from mrcaudiocodec_amd.store import concat_spans
    with pytest.raises(ValueError, match="concat_spans: .*" + text):
        concat_spans(*args, **kw)
    from mrcaudiocodec_amd.store import check_spans
    # ... and half an inner piece exactly is allowed: check_spans takes what concat_spans gives
    out = concat_spans([[9, 6, 9]], [[0, 0, 0]], crossfade=3)
    assert check_spans(*out[1:], (1, 3)) is not None


# ------------------------------------------------------------------ the envelope, restated (the GPU test's crossfade bound)
def envelope(span_len, fade_in, fade_out, lo=0, hi=None):
    """e of the header at j = lo .. hi - 1 (all of the span by default) in float64: one division of two exact integers per ramp
    sample, 1.0 between the ramps"""
    j = np.arange(lo, span_len if hi is None else hi, dtype=np.float64)
    e = np.ones(j.size)
    rise, fall = j < fade_in, j >= span_len - fade_out
    e[rise] = (2 * j[rise] + 1) / (2.0 * max(fade_in, 1))
    e[fall] = (2 * (span_len - 1 - j[fall]) + 1) / (2.0 * max(fade_out, 1))
    return e


def test_the_ramp_is_symmetric_never_0_or_1_and_a_crossfade_adds_to_one_within_three_roundings():
    worst = 0.0
    rng = np.random.default_rng(0)
    for F in [1, 2, 3, 7, 160] + [int(v) for v in rng.integers(1, 5000, 345)]:
        up, down = envelope(F, F, 0), envelope(F, 0, F)
        assert np.array_equal(up, down[::-1]) and up.min() > 0.0 and up.max() < 1.0
        v = rng.standard_normal(F)
        row = up * v + down * v                                        # two divisions, two products, one addition
        worst = max(worst, float(np.max(np.abs(row - v) / np.abs(v))) / 2.0 ** -53)
    assert worst <= 4.0, worst                                         # |row - v| <= 2^-51 |v|
    assert envelope(5, 2, 3).tolist() == [0.25, 0.75, 5 / 6, 0.5, 1 / 6] and envelope(4, 0, 0).tolist() == [1.0] * 4
