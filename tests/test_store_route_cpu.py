"""
The store's routed windows (mrc_pac_store_decode_window_routed, mrc_pac_store_stft_window_routed, mrc_pac_store_route_info;
PacStore.decode_window_routed / stft_window(route_gains=, route_irs=), store.check_routes, store.array_routes, cli -d
--array-ir) as far as a CPU reaches: the binding against the header, the entry and the argument tuple window_entry gives for
routed rows, the Python-side refusals raised before any library call, the layout array_routes builds, and the command line's
flag checks before a file is read.
"""
import ctypes as C

import numpy as np
import pytest

import chain_kit as kit
import store_kit

STORE, OUT, STREAM = 0x1000, 0x2000, 0x3000
NONE = -2


# ------------------------------------------------------------------ the binding
def test_binding_of_the_routed_calls():
    from mrcaudiocodec_amd import _lib, store
    names = ("mrc_pac_store_decode_window_routed", "mrc_pac_store_stft_window_routed", "mrc_pac_store_route_info")
    kit.check_binding(names)
    assert all(hasattr(_lib.lib, n) for n in names)
    name = lambda a: a.split()[-1].lstrip("*")
    # the reverb call's arguments without gain and ir_of, the two route arrays behind ratio_of
    reverb = [name(a) for a in kit.header_args("mrc_pac_store_decode_window_reverb")]
    routed = [name(a) for a in kit.header_args("mrc_pac_store_decode_window_routed")]
    at = reverb.index("ratio_of")
    assert routed == [n for n in reverb[:at + 1] if n != "gain"] + ["route_gain", "route_ir"] + reverb[at + 2:]
    stft = [name(a) for a in kit.header_args("mrc_pac_store_stft_window")]
    stft_routed = [name(a) for a in kit.header_args("mrc_pac_store_stft_window_routed")]
    at = stft.index("ratio_of")
    assert stft_routed == [n for n in stft[:at + 1] if n != "gain"] + ["route_gain", "route_ir"] + stft[at + 2:]
    text = kit.header_text()
    assert "#define MRC_MAX_STORE_ROUTE_CHANNELS 16" in text and "#define MRC_ROUTE_NONE (-2)" in text
    assert "#define MRC_OPT_STORE_ROUTE_GROUP 8" in text and _lib.MRC_OPT_STORE_ROUTE_GROUP == 8
    assert store.ROUTE_NONE == _lib.MRC_ROUTE_NONE == NONE and store.MAX_ROUTE_CHANNELS == _lib.MRC_MAX_STORE_ROUTE_CHANNELS == 16


# ------------------------------------------------------------------ window_entry
def _asked(monkeypatch, caller, **kw):
    """the (name, args by the header's names) window_entry gives for that call on a store that was never created"""
    from mrcaudiocodec_amd import store
    s = store_kit.husk(monkeypatch, n_irs=4)
    asked = []
    s._out_tensor = lambda what, shape, dtype, out, stream: (asked.append(shape) or None, STREAM)
    s._call_window = lambda rows, who, window, channels, fmt, out, stream, stft=None: asked.append(
        store.window_entry(STORE, rows, who, window, channels, fmt, OUT, stream, stft))
    getattr(s, caller)(**kw)
    shape, (name, args, _keep) = asked
    names = [a.split()[-1].lstrip("*") for a in kit.header_args(name)]
    assert len(args) == len(names)
    return shape, name, dict(zip(names, args))


def _held(ptr, ctype, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).tolist()


def test_routed_rows_go_to_the_routed_entry(monkeypatch):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import _lib
    gains = [[[1.0, 0.5, 0.0], [0.25, 2.0, 1.0]], [[1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]]
    irs = [[[0, -1, NONE], [NONE, 3, -1]], [[1, 2, 3], [-1, -1, -1]]]
    shape, name, got = _asked(monkeypatch, "decode_window_routed", files=[[0, 1], [1, 1]], starts=[[0, 5], [7, -3]], route_gains=gains,
                              route_irs=irs, window=16, dtype=torch.float32, rate_divisor=2, mix="mid", resample=(2, 3),
                              speed_factors=[(1, 1), (11, 10)], speed_index=[[1, 0], [0, 0]])
    assert name == "mrc_pac_store_decode_window_routed" and shape == (2, 3, 16)
    assert (got["s"], got["out"], got["stream"]) == (STORE, OUT, STREAM)
    want = dict(rate_divisor=2, mix=_lib.MRC_MIX_MID, n_ratios=2, zeros=16, rolloff=0.9475, n_bands=0, edge_hz=None, band_gain=None,
                n_items=2, window=16, n_channels_out=3, format=_lib.MRC_WINDOW_F32)
    assert {key: got[key] for key in want} == want
    assert _held(got["ratio_up"], C.c_int32, 2) == [2, 20] and _held(got["ratio_down"], C.c_int32, 2) == [3, 33]
    assert _held(got["term_offset"], C.c_int64, 3) == [0, 2, 4] and _held(got["file"], C.c_int64, 4) == [0, 1, 1, 1]
    assert _held(got["start"], C.c_int64, 4) == [0, 5, 7, -3] and _held(got["ratio_of"], C.c_int32, 4) == [1, 0, 0, 0]
    assert _held(got["route_gain"], C.c_double, 12) == np.ravel(gains).tolist()
    assert _held(got["route_ir"], C.c_int32, 12) == np.ravel(irs).tolist()
    assert "gain" not in got and "ir_of" not in got
    # 1-D terms with item_offsets, every term on one channel, the defaults of everything else
    shape, name, got = _asked(monkeypatch, "decode_window_routed", files=[1, 1, 1], starts=[0, 1, 2], route_gains=[[1.0], [2.0], [3.0]],
                              route_irs=[[0], [-1], [NONE]], window=7, item_offsets=[0, 0, 3])
    assert name == "mrc_pac_store_decode_window_routed" and shape == (2, 1, 7)
    assert (got["rate_divisor"], got["mix"], got["n_ratios"], got["n_channels_out"], got["format"]) == (1, _lib.MRC_MIX_EACH, 1, 1, _lib.MRC_WINDOW_PCM16)
    assert _held(got["term_offset"], C.c_int64, 3) == [0, 0, 3] and _held(got["route_ir"], C.c_int32, 3) == [0, -1, NONE]


def test_routed_stft_goes_to_the_routed_stft_entry(monkeypatch):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd import _lib
    routes = dict(route_gains=[[1.0, 0.5], [0.25, 2.0]], route_irs=[[0, -1], [NONE, 3]])
    shape, name, got = _asked(monkeypatch, "stft_window", files=[0, 1], starts=[0, 5], n_frames=3, hop=4, n_fft=16, mix="left",
                              dtype=torch.float64, center=True, **routes)
    assert name == "mrc_pac_store_stft_window_routed" and shape == (2, 2, 9, 3)
    want = dict(rate_divisor=1, mix=_lib.MRC_MIX_LEFT, n_ratios=1, n_items=2, n_fft=16, n_frames=3, hop=4, mode=_lib.MRC_STFT_POWER,
                n_filters=0, bank=None, n_channels_out=2, format=_lib.MRC_WINDOW_F64)
    assert {key: got[key] for key in want} == want and "gain" not in got and "ir_of" not in got
    assert _held(got["term_offset"], C.c_int64, 3) == [0, 1, 2] and _held(got["start"], C.c_int64, 2) == [-8, -3]
    assert _held(got["route_gain"], C.c_double, 4) == [1.0, 0.5, 0.25, 2.0] and _held(got["route_ir"], C.c_int32, 4) == [0, -1, NONE, 3]
    # rows of several terms: 1-D with item_offsets, or [n][K]
    shape, name, got = _asked(monkeypatch, "stft_window", files=[0, 1], starts=[0, 5], n_frames=3, hop=4, n_fft=16, mix="mid",
                              item_offsets=[0, 2], output="bank", bank=np.ones((5, 9)), **routes)
    assert name == "mrc_pac_store_stft_window_routed" and shape == (1, 2, 5, 3) and got["n_items"] == 1 and got["n_filters"] == 5
    shape, name, got = _asked(monkeypatch, "stft_window", files=[[0, 1]], starts=[[0, 5]], n_frames=3, hop=4, n_fft=16, mix="mid",
                              route_gains=[routes["route_gains"]], route_irs=[routes["route_irs"]])
    assert name == "mrc_pac_store_stft_window_routed" and shape == (1, 2, 9, 3) and _held(got["term_offset"], C.c_int64, 2) == [0, 2]


def test_rows_built_without_routes_stay_valid():
    from mrcaudiocodec_amd import store
    rows = store.WindowRows(1, None, None, 2, None, None, None, np.arange(3, dtype=np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64),
                            np.ones(2))
    assert rows.routes is None
    name, args, _ = store.window_entry(STORE, rows, "decode_window_sum", 16, 2, 0, OUT, STREAM)
    assert name == "mrc_pac_store_decode_window_sum"


def test_stft_window_refuses_routes_beside_gains_or_ir_index(monkeypatch):
    pytest.importorskip("torch")
    s = store_kit.husk(monkeypatch, n_irs=4)
    base = dict(files=[0, 1], starts=[0, 5], n_frames=3, hop=4, n_fft=16, mix="mid")
    routes = dict(route_gains=[[1.0, 0.5], [0.25, 2.0]], route_irs=[[0, -1], [NONE, 3]])
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs stand in the place of gains and ir_index.* gains must be None"):
        s.stft_window(gains=[1.0, 1.0], item_offsets=[0, 1, 2], **base, **routes)
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs stand in the place.* ir_index must be None"):
        s.stft_window(ir_index=[0, -1], **base, **routes)
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs stand in the place.* channels must be None"):
        s.stft_window(channels=1, **dict(base, mix=None), **routes)
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs go together, got only route_irs"):
        s.stft_window(route_irs=routes["route_irs"], **base)
    with pytest.raises(ValueError, match="stft_window: route_gains and route_irs go together, got only route_gains"):
        s.stft_window(route_gains=routes["route_gains"], **base)
    with pytest.raises(ValueError, match=r"stft_window: files and starts must have one shape, got \(2,\) and \(3,\)"):
        s.stft_window(**dict(base, starts=[0, 5, 6]), **routes)
    with pytest.raises(ValueError, match=r"stft_window: route_irs must be ROUTE_NONE \(-2\), -1 or lie in 0\.\.3 .* got 4 at term 1, channel 0"):
        s.stft_window(route_gains=routes["route_gains"], route_irs=[[0, -1], [4, 3]], **base)


# ------------------------------------------------------------------ check_routes
def test_check_routes_gives_the_two_arrays():
    from mrcaudiocodec_amd.store import check_routes
    g, i = check_routes([[[1, 2], [3, 4]], [[5, 6], [7, 8]]], [[[0, -1], [NONE, 2]], [[2, 2], [-1, -1]]], 4, 3, "f")
    assert g.dtype == np.float64 and g.shape == (4, 2) and g.flags.c_contiguous and g.ravel().tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert i.dtype == np.int32 and i.shape == (4, 2) and i.flags.c_contiguous and i.ravel().tolist() == [0, -1, NONE, 2, 2, 2, -1, -1]
    g, i = check_routes(np.zeros((0, 5)), np.zeros((0, 5), np.int64), 0, 0, "f")
    assert g.shape == i.shape == (0, 5)
    g, i = check_routes(np.ones((3, 16), np.float32), np.full((3, 16), NONE), 3, 0, "f")     # no bank: absent and dry are fine
    assert g.shape == (3, 16) and check_routes([[1.0]], [[-1]], 1, 0, "f")[1].tolist() == [[-1]]


@pytest.mark.parametrize("gains,irs,n_terms,n_irs,text", [
    ([1.0, 2.0], [0, -1], 2, 3, r"route_gains and route_irs must have one shape, the 2 terms and a last axis of 1 to 16 channels, got \(2,\) and \(2,\)"),
    ([[1.0, 2.0]], [[0], [-1]], 2, 3, r"must have one shape, the 2 terms .* got \(1, 2\) and \(2, 1\)"),
    ([[1.0, 2.0]], [[0, -1]], 2, 3, r"must have one shape, the 2 terms .* got \(1, 2\) and \(1, 2\)"),
    (np.ones((1, 17)), np.zeros((1, 17), int), 1, 3, r"a last axis of 1 to 16 channels, got \(1, 17\)"),
    (np.ones((1, 0)), np.zeros((1, 0), int), 1, 3, r"a last axis of 1 to 16 channels, got \(1, 0\)"),
    ([["a", "b"]], [[0, -1]], 1, 3, "route_gains must be numbers"),
    ([[1.0, 2.0]], [[0.0, -1.0]], 1, 3, "route_irs must be ints"),
    ([[1.0, 2.0]], [["a", "b"]], 1, 3, "route_irs must be ints"),
    ([[1.0, 2.0], [float("nan"), 1.0]], [[0, -1], [0, 0]], 2, 3, "route_gains must be finite, got nan at term 1, channel 0"),
    ([[1.0, float("inf")]], [[0, -1]], 1, 3, "route_gains must be finite, got inf at term 0, channel 1"),
    ([[1.0, 2.0], [1.0, 1.0]], [[0, -1], [0, -3]], 2, 3, r"route_irs must be ROUTE_NONE \(-2\), -1 or an index into the bank, got -3 at term 1, channel 1"),
    ([[1.0, 2.0]], [[3, -1]], 1, 3, r"route_irs must be ROUTE_NONE \(-2\), -1 or lie in 0\.\.2 \(the store's impulse responses\), got 3 at term 0, channel 0"),
    ([[1.0, 2.0]], [[NONE, 0]], 1, 0, r"route_irs names impulse response 0 at term 0, channel 1, but the store has none \(set_impulse_responses\)"),
])
def test_check_routes_refusals(gains, irs, n_terms, n_irs, text):
    from mrcaudiocodec_amd.store import check_routes
    with pytest.raises(ValueError, match="decode_window_routed: .*" + text):
        check_routes(gains, irs, n_terms, n_irs)


def test_decode_window_routed_refuses_before_any_library_call(monkeypatch):
    pytest.importorskip("torch")
    s = store_kit.husk(monkeypatch, n_irs=2)
    ok = dict(files=[[0, 1]], starts=[[0, 5]], route_gains=[[[1.0], [0.5]]], route_irs=[[[0], [-1]]], window=16, mix="mid")
    for change, text in ((dict(route_irs=[[[0], [2]]]), r"route_irs must be ROUTE_NONE \(-2\), -1 or lie in 0\.\.1 .* got 2 at term 1, channel 0"),
                         (dict(route_gains=[[1.0, 0.5]]), "must have one shape, the 2 terms"),
                         (dict(starts=[[0, 5, 6]]), r"files and starts must have one shape, got \(1, 2\) and \(1, 3\)"),
                         (dict(mix="side"), "mix"), (dict(rate_divisor=3), "rate_divisor"),
                         (dict(speed_index=[[0, 0]]), "speed_factors and speed_index go together"),
                         (dict(files=[0, 1], starts=[0, 5]), r"must be \[n\]\[K\], or 1-D with item_offsets")):
        with pytest.raises(ValueError, match="decode_window_routed: .*" + text):
            s.decode_window_routed(**dict(ok, **change))


# ------------------------------------------------------------------ array_routes
def test_array_routes_lays_the_bank_out_room_major():
    from mrcaudiocodec_amd.store import array_routes
    g, i = array_routes([0, 2, -1], 4)
    assert g.dtype == np.float64 and i.dtype == np.int32 and g.shape == i.shape == (3, 4)
    assert i.tolist() == [[0, 1, 2, 3], [8, 9, 10, 11], [-1, -1, -1, -1]] and np.all(g == 1.0)
    g, i = array_routes([[1, -1]], 2, gains=[[0.5, 3.0]])                                     # a gain per term, [n][K] terms
    assert i.tolist() == [[[2, 3], [-1, -1]]] and g.tolist() == [[[0.5, 0.5], [3.0, 3.0]]]
    g, i = array_routes([1], 3, gains=[[1.0, 2.0, 4.0]])                                      # ... or per term and microphone
    assert i.tolist() == [[3, 4, 5]] and g.tolist() == [[1.0, 2.0, 4.0]]
    g, i = array_routes(np.zeros(0, np.int64), 16)
    assert g.shape == i.shape == (0, 16)
    for kw, text in ((dict(room_of=[0], n_mics=0), "n_mics must be an int in 1..16"), (dict(room_of=[0], n_mics=17), "n_mics must be an int in 1..16"),
                     (dict(room_of=[0], n_mics=2.0), "n_mics must be an int"), (dict(room_of=[-2], n_mics=2), "room_of must be ints >= -1"),
                     (dict(room_of=[0.5], n_mics=2), "room_of must be ints >= -1"),
                     (dict(room_of=[0, 1], n_mics=2, gains=[1.0]), r"gains must have shape \(2,\) or \(2, 2\), got \(1,\)")):
        with pytest.raises(ValueError, match="array_routes: " + text):
            array_routes(**kw)


# ------------------------------------------------------------------ the command line
def test_check_array_ir_args_and_read_array_ir(tmp_path):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import ir_at_rate
    assert cli.check_array_ir_args(None, None, True) is None and cli.check_array_ir_args(None, "room.npy", False) is None
    assert cli.check_array_ir_args("mics.npy", None, True) == "mics.npy"
    with pytest.raises(ValueError, match="--array-ir decodes a file through the responses of a microphone array: it needs -d"):
        cli.check_array_ir_args("mics.npy", None, False)
    with pytest.raises(ValueError, match="--array-ir and --ir both convolve the decoded file: give one of them"):
        cli.check_array_ir_args("mics.npy", "room.npy", True)
    npy, wav = str(tmp_path / "m.npy"), str(tmp_path / "m.wav")
    mics = np.random.default_rng(1).standard_normal((3, 40)).astype(np.float32)
    np.save(npy, mics)
    got = cli.read_array_ir(npy, 16000)
    assert len(got) == 3 and all(np.array_equal(g, m.astype(np.float64)) and g.dtype == np.float64 for g, m in zip(got, mics))
    codes = np.clip(np.rint(mics * 8000), -32767, 32767).astype(np.int16)
    with open(wav, "wb") as fp:
        fp.write(cli.wav_bytes(codes, 48000))
    x = np.sign(codes) * 2.0 * np.abs(codes.astype(np.float64)) / 65535
    got = cli.read_array_ir(wav, 16000)
    assert len(got) == 3 and all(np.array_equal(g, ir_at_rate(x[c], 48000, 16000)) for c, g in enumerate(got))
    for bad, text in ((np.zeros(4), r"the array must be \[C\]\[taps\] with 1 to 16 microphones, got shape \(4,\)"),
                      (np.zeros((17, 2)), r"with 1 to 16 microphones, got shape \(17, 2\)"),
                      (np.array([[1.0, float("nan")]]), "--array-ir: impulse response 0 must be finite")):
        np.save(npy, bad)
        with pytest.raises(ValueError, match=text):
            cli.read_array_ir(npy, 48000)
    with pytest.raises(ValueError, match="--array-ir: "):
        cli.read_array_ir(str(tmp_path / "none.wav"), 48000)


@pytest.mark.parametrize("argv,text", [
    (["in.wav", "out.pac", "--array-ir", "mics.npy"], "--array-ir decodes a file through the responses of a microphone array: it needs -d"),
    (["--levels", "a.pac", "--array-ir", "mics.npy"], "--array-ir decodes a file through the responses of a microphone array: it needs -d"),
    (["-d", "in.pac", "out.wav", "--array-ir", "mics.npy", "--ir", "room.npy"], "--array-ir and --ir both convolve the decoded file"),
    (["in.pac", "out.npy", "--band-energies", "--hop", "256", "--array-ir", "mics.npy"], "--array-ir decodes a file through"),
])
def test_cli_refuses_the_flag_before_a_file_is_read(argv, text, capsys):
    from mrcaudiocodec_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err
