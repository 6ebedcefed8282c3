"""
GPU tests of the store's filter-bank energies (mrc_pac_store_filterbank_window, PacStore.filterbank_window, cli
--filterbank-energies) on the few-hop files of the mix tests (settings B, C, D, K and the default five-hop stereo file), at
most 24 frames a call: every value against the restatement in the library's stated order (tests/filterbank_restatement.py),
to the bit, for both formats, five filter sets (the 256-filter one in the default setting), four hops, starts before, inside,
across the end of and behind the files, and every mix; left and right against the two-channel call; the sum over a bank
against the band call's one band; bit-identity from call to call, under shuffled items, alone and in company and over slab
sizes; damage; the refusals; the command line.  Everything oracle-side is computed once per module and never written to.
"""
import re

import numpy as np
import pytest

import bands_restatement as BR
import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import filterbank_restatement as FR
import mix_restatement as MR
import settings_kit as SK

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = MR.KIT_SIDS + ("default",)
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
FN = "mrc_pac_store_filterbank_window"
MIXES = (None, "mid", "left", "right")
N_FRAMES = 24
SETS = ("mel", "slaney", "one", "narrow", "full")


class _Kitchen:
    """one setting: its handle, files, store, index and restated lines (computed on first use)"""

    def __init__(self, sid):
        from mrcaudiocodec_amd import pacfile as ppac
        from mrcaudiocodec_amd.store import PacStore
        F = MR.files(sid)
        self.sid, self.L, self.S, self.blksw = sid, F["L"], F["S"], F["blksw"]
        self.files, self.nch = F["files"], F["nch"]
        if sid == "default":
            self.h, self.cfg = kit.handle(), ppac.make_config()
        else:
            self.h, self.cfg = kit.handle(**SK.handle_kwargs(sid)), SK.config(sid)
        self.fs = int(self.cfg.sample_rate)
        self.index = [ppac.index(b, self.cfg) for b in self.files]
        self.store = PacStore(self.h, self.files)
        self._ff, self._ref = {}, {}
        self.sets = FR.filter_sets(self.fs)

    def ff(self, f):
        if f not in self._ff:
            self._ff[f] = FR.FileFilters(BR.FileBands(self.files[f], self.S, self.blksw, self.L, self.fs))
        return self._ff[f]

    def ref(self, f, name, start, n_frames, hop, mix, channels):
        """float64 [channels][n_filters][n_frames] of one item, read-only, and the blocks the item parses"""
        key = (f, name, int(start), n_frames, hop, mix, channels)
        if key not in self._ref:
            points, norm = self.sets[name]
            out, needed = self.ff(f).window(points, norm, start, n_frames, hop, mix, channels)
            out.setflags(write=False)
            self._ref[key] = (out, needed)
        return self._ref[key]

    def starts(self, f):
        """before the first tile, inside the file's first run of short blocks (a file without one: sample 5), across the
        file's end, behind the last tile"""
        ix = self.index[f]
        short = np.flatnonzero(np.asarray(ix["block_b"]) == self.S)
        inside = int(ix["block_start"][short[0]]) - self.L + 5 if short.size else 5
        n = int(self.store.n_samples[f])
        return [-self.L, inside, n - 100, n + 5 * self.L]

    def hops(self):
        return (self.S // 2, self.S, self.L, 1000)

    def call(self, name, files, starts, hop, n_frames=N_FRAMES, **kw):
        points, norm = self.sets[name]
        return self.store.filterbank_window(files, starts, n_frames, hop, points, norm=norm, **kw)


_KITCHENS = {}


def _kitchen(sid):
    if sid not in _KITCHENS:
        _KITCHENS[sid] = _Kitchen(sid)
    return _KITCHENS[sid]


@pytest.fixture(scope="module", params=SIDS)
def kitchen(request):
    return _kitchen(request.param)


@pytest.fixture(scope="module", autouse=True)
def stores_closed_after_module():
    yield
    for k in _KITCHENS.values():
        k.store.close()
    _KITCHENS.clear()


def _same(a, b):
    view = np.int64 if a.dtype == np.float64 else np.int32
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(view), b.view(view))


def _items(k, mono_only=False):
    files, starts = [], []
    for f in range(len(k.files)):
        if mono_only and k.nch[f] != 1:
            continue
        for s in k.starts(f):
            files.append(f)
            starts.append(s)
    return files, starts


# ------------------------------------------------------------------ 1: equality with the restatement, to the bit
@pytest.mark.parametrize("name", SETS)
def test_values_equal_the_restatement_to_the_bit(kitchen, name):
    k = kitchen
    if name == "full" and k.sid != "default":
        return                                                        # (256 filters: the default setting only)
    points, norm = k.sets[name]
    whole = np.array([0.0, k.fs / 2.0])
    cases = [(mix, 1 if mix else 2, False) for mix in MIXES] + [(None, 1, True)]
    n_values = 0
    for hop in k.hops():
        for mix, channels, mono_only in cases:
            files, starts = _items(k, mono_only)
            if not files:                                             # (a setting without a mono file)
                continue
            want = np.array([k.ref(f, name, s, N_FRAMES, hop, mix, channels)[0] for f, s in zip(files, starts)])
            assert want.shape == (len(files), channels, len(points) - 2, N_FRAMES) and want.any()
            assert not want[3::4].any()                               # the starts behind the files: all zeros
            got = k.call(name, files, starts, hop, channels=channels, dtype=torch.float64, mix=mix)
            assert got.is_cuda and tuple(got.shape) == want.shape
            assert _same(got.cpu().numpy(), want), (k.sid, name, hop, mix, channels, np.abs(got.cpu().numpy() - want).max())
            parsed = k.store.stats()["chunks_parsed"]
            got32 = k.call(name, files, starts, hop, channels=channels, mix=mix)
            assert got32.dtype == torch.float32 and _same(got32.cpu().numpy(), want.astype(np.float32))     # one conversion
            assert k.store.stats()["chunks_parsed"] == parsed > 0
            k.store.band_energy_window(files, starts, N_FRAMES, hop, whole, channels=channels, mix=mix)
            assert k.store.stats()["chunks_parsed"] == parsed         # the band call parses the same blocks
            n_values += 2 * want.size
    if name in ("mel", "narrow"):                                     # no filter is empty, also in a short block
        points = np.asarray(points)
        for a, b in ((k.S, k.S), (k.L, k.L)):
            _, _, rows = FR.line_weights(k.fs, a, b, points, norm)
            assert all(len(r) and r.max() > 0 for r in rows)
    print("%s, %s filters: %d values equal to the restatement" % (k.sid, name, n_values))


# ------------------------------------------------------------------ 2: left, right and the channel map
def test_left_and_right_are_the_channels_of_the_two_channel_call(kitchen):
    k = kitchen
    files, starts = _items(k)
    for dtype in (torch.float64, torch.float32):
        both = k.call("mel", files, starts, 1000, channels=2, dtype=dtype).cpu().numpy()
        left = k.call("mel", files, starts, 1000, dtype=dtype, mix="left").cpu().numpy()
        right = k.call("mel", files, starts, 1000, dtype=dtype, mix="right").cpu().numpy()
        mid = k.call("mel", files, starts, 1000, dtype=dtype, mix="mid").cpu().numpy()
        assert _same(left[:, 0], both[:, 0]) and _same(right[:, 0], both[:, 1])
        for i, f in enumerate(files):
            if k.nch[f] == 1:                                        # a mono file fills both channels, and is its own mid
                assert _same(both[i, 0], both[i, 1]) and _same(mid[i, 0], both[i, 0])
        loud = [i for i, f in enumerate(files) if k.nch[f] == 2 and i % 4 == 1]      # the starts inside the stereo files
        assert loud and all(not _same(both[i, 0], both[i, 1]) for i in loud)


# ------------------------------------------------------------------ 3: a bound against the band call
def test_a_banks_sum_stays_below_the_band_calls_one_band(kitchen):
    """a line's un-normalised weights add up to at most 1 (1e-12: the CPU test's bound on their sum), so a frame's sum over the
    filters is at most the energy of the one band [0, fs / 2]; the one filter of "one" weighs every line below 1 except none at
    1, so it lies strictly below wherever there is energy"""
    k = kitchen
    files, starts = _items(k)
    whole = np.array([0.0, k.fs / 2.0])
    for hop in (k.S, 1000):
        band = k.store.band_energy_window(files, starts, N_FRAMES, hop, whole, channels=2, dtype=torch.float64).cpu().numpy()[:, :, 0]
        mel = k.call("mel", files, starts, hop, channels=2, dtype=torch.float64).cpu().numpy().sum(axis=2)
        one = k.call("one", files, starts, hop, channels=2, dtype=torch.float64).cpu().numpy()[:, :, 0]
        assert band.any() and np.all(mel <= (1 + 1e-12) * band)
        assert np.all(one[band > 0] < band[band > 0]) and not one[band == 0].any()
        print("%s, hop %d: the mel bank holds %.3f to %.3f of the one band's energy" % (
            k.sid, hop, (mel[band > 0] / band[band > 0]).min(), (mel[band > 0] / band[band > 0]).max()))


# ------------------------------------------------------------------ 4: bit-identity
@pytest.mark.parametrize("mix", [None, "mid"])
def test_values_do_not_depend_on_call_order_company_or_slabs(kitchen, mix):
    k = kitchen
    hop = k.S
    files, starts = _items(k)
    n, span = len(files), N_FRAMES * hop
    call = lambda fs_, ss: k.call("mel", fs_, ss, hop, channels=1 if mix else 2, dtype=torch.float64, mix=mix).cpu().numpy()
    base = call(files, starts)
    st = k.store.stats()
    assert st["slabs"] == 1 and 1 <= st["decode_launches"] <= 8 and st["plan_bytes_uploaded"] > 0
    assert all(st["ms"][name] > 0.0 for name in ("plan_upload", "unpack", "synthesis", "window_out"))
    assert _same(call(files, starts), base)                          # call to call
    for order in (list(range(n))[::-1], list(np.random.default_rng(3).permutation(n)), [0, 0] + list(range(n))):
        got = call([files[i] for i in order], [starts[i] for i in order])
        assert _same(got, base[order]), (k.sid, mix, order)
    for i in range(n):                                               # alone
        assert _same(call([files[i]], [starts[i]]), base[i:i + 1])
    try:
        for slab in (1, span, 2 * span + 1, 5 * span, 0, SLAB_DEFAULT):
            k.h.set_option(SLAB_OPTION, slab)
            assert _same(call(files, starts), base), (k.sid, mix, slab)
            per = n if slab == 0 else max(1, slab // span)
            assert k.store.stats()["slabs"] == -(-n // per), (k.sid, slab)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)


# ------------------------------------------------------------------ 5: damage
def _words(err):
    """an error's text behind the name of the entry point"""
    return re.sub(r"^.*?mrc_pac_store_\w+: ", "", str(err))


def test_damage_is_reported_inside_a_needed_block_and_never_read_outside(kitchen):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    ix, L = k.index[0], k.L
    reason = re.escape("table id not in {0..3, 15}")
    j = int(ix["n_blocks"]) - 2                                   # the last joint block
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                             # table id 4
    pj, aj, bj = (int(ix[name][j]) for name in ("block_start", "block_a", "block_b"))
    t0, t1 = 2 * pj + aj - 2 * L, 2 * pj + 2 * aj + bj - 2 * L    # its tile, doubled
    points, norm = k.sets["slaney"]
    with PacStore(k.h, [k.files[0], bytes(bad)]) as store:
        with pytest.raises(MrcError, match=r"file 1: chunk at byte %d: %s" % (at - 4, reason)) as w:
            store.decode_window([1], [pj - L], 3, channels=2)
        for mix in MIXES:
            for start, n_frames, hop in ((t1 // 2 - 1, 1, 1), (t0 // 2 - 50, 2, 26), (-L, 20, L)):
                with pytest.raises(MrcError, match=r"%s: file 1: chunk at byte %d: %s" % (FN, at - 4, reason)) as e:
                    store.filterbank_window([0, 1], [0, start], n_frames, hop, points, norm=norm, mix=mix)
                assert e.value.code == -1 and _words(e.value) == _words(w.value)            # the window's words
            # frames that end at the tile's start or begin at its end never read it: the undamaged file's values
            seen = False
            for start, n_frames, hop in ((t0 // 2 - 3 * 40, 3, 40), ((t1 + 1) // 2, 2, 500)):
                got = store.filterbank_window([1, 0], [start, start], n_frames, hop, points, norm=norm, dtype=torch.float64,
                                              mix=mix).cpu().numpy()
                assert _same(got[0], got[1])
                seen = seen or bool(got.any())
            assert seen


# ------------------------------------------------------------------ 6: refusals
def test_refusals_leave_out_untouched(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    nf = len(k.files)
    out = torch.full((4 * 2 * 80 * 8,), 77.0, dtype=torch.float64, device="cuda:0")
    mel = k.sets["mel"][0]
    stereo = k.nch.index(2)
    ok = dict(mix=_lib.MRC_MIX_EACH, files=[0], starts=[0], n_frames=8, hop=100, points=mel, norm=0, nch=2, fmt=_lib.MRC_WINDOW_F64,
              out=True)

    def call(**kw):
        a = dict(ok, **kw)
        files, starts = np.ascontiguousarray(a["files"], dtype=np.int64), np.ascontiguousarray(a["starts"], dtype=np.int64)
        points = np.ascontiguousarray(a["points"], dtype=np.float64)
        torch.cuda.synchronize()
        rc = _lib.lib.mrc_pac_store_filterbank_window(k.store._s, a["mix"], len(files), files.ctypes.data, starts.ctypes.data,
                                                      a["n_frames"], a["hop"], a.get("n_filters", len(points) - 2),
                                                      points.ctypes.data, a["norm"], a["nch"], a["fmt"],
                                                      out.data_ptr() if a["out"] else None, None)
        return rc, _lib.lib.mrc_last_error(k.h._h).decode()

    def refused(*words, **kw):
        rc, text = call(**kw)
        assert rc == _lib.MRC_ERR_INVALID and FN in text and all(w in text for w in words), (kw, text)
        assert bool((out == 77.0).all()) and k.store.stats()["chunks_parsed"] == 0

    for mix in (4, -1, 7):
        refused("mix %d" % mix, mix=mix)
    for nch in (0, 3):
        refused("n_channels_out must be 1 or 2", nch=nch)
    for mix in (_lib.MRC_MIX_MID, _lib.MRC_MIX_LEFT, _lib.MRC_MIX_RIGHT):
        refused("n_channels_out must be 1", mix=mix, nch=2)
    for fmt in (_lib.MRC_WINDOW_PCM16, 3, -1):
        refused("format %d" % fmt, fmt=fmt)
    refused("n_frames < 0", n_frames=-1)
    for hop in (0, -4):
        refused("hop < 1", hop=hop)
    refused("2^62", n_frames=(1 << 31) + 1, hop=1 << 31)
    refused("n_filters 0", n_filters=0)
    refused("n_filters 257", n_filters=257, points=np.arange(259.0))
    refused("point_hz[1] is not finite", points=[0.0, np.inf, 5.0])
    refused("point_hz[0] is not finite", points=[np.nan, 1.0, 2.0])
    refused("point_hz[0] < 0", points=[-0.5, 100.0, 200.0])
    refused("not strictly increasing at [2]", points=[0.0, 100.0, 100.0])
    for norm in (2, -1):
        refused("norm %d" % norm, norm=norm)
    refused("file[1] = %d" % nf, "outside the store's %d files" % nf, files=[0, nf], starts=[0, 0])
    refused("file[0] = -1", files=[-1])
    refused("out is NULL", out=False)
    refused("item 0: file %d is stereo, the call asks for one channel" % stereo, files=[stereo, stereo], starts=[9, 0], nch=1)
    # nothing to write: MRC_OK, out untouched, also without out
    for kw in (dict(files=[], starts=[]), dict(n_frames=0), dict(files=[], starts=[], out=False), dict(n_frames=0, out=False)):
        rc, _ = call(**kw)
        assert rc == 0 and bool((out == 77.0).all()) and k.store.stats()["slabs"] == 0
    # the extremes of start are starts like any other
    rc, _ = call(files=[0, 0, 0], starts=[-(1 << 63), (1 << 63) - 1, -(1 << 62)], n_frames=2, hop=1 << 61)
    assert rc == 0
    got = out[:3 * 2 * 80 * 2].reshape(3, 2, 80, 2).cpu().numpy()
    assert not got[:2].any() and not got[2, :, :, 0].any()
    want = k.ref(0, "mel", -(1 << 62), 2, 1 << 61, None, 2)[0]
    assert _same(got[2], want) and not want[:, :, 0].any()


# ------------------------------------------------------------------ 7: the command line
def test_cli_writes_the_whole_files_filterbank_energies(tmp_path):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import mel_points
    k = _kitchen("default")
    src, dst = str(tmp_path / "s.pac"), str(tmp_path / "e.npy")
    with open(src, "wb") as f:
        f.write(k.files[0])
    n, fs = int(k.store.n_samples[0]), k.fs
    for argv, hop, points, norm, mix in (
            (["--hop", "480", "--mel", "80"], 480, mel_points(80, 0, fs / 2), None, None),
            (["--hop", "1000", "--mel", "40", "--f-min", "50", "--f-max", "8000", "--mel-scale", "slaney", "--filter-norm", "slaney",
              "--mix", "mid"], 1000, mel_points(40, 50, 8000, "slaney"), "slaney", "mid"),
            (["--hop", "300", "--filter-points", "0,250.5,1e3,4000,30000", "--mix", "right"], 300,
             [0.0, 250.5, 1000.0, 4000.0, 30000.0], None, "right")):
        cli.main(["--filterbank-energies", src, dst] + argv)
        got = np.load(dst)
        n_frames = -(-n // hop)
        want = k.store.filterbank_window([0], [0], n_frames, hop, points, norm=norm, mix=mix)[0].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (1 if mix else 2, len(points) - 2, n_frames)
        assert _same(got, want) and got.any()
