"""
GPU tests of the store's one-channel windows (mrc_pac_store_decode_window_mix, PacStore.decode_window(mix=), cli -d --mix):
left and right are the bits of channel 0 / 1 of the two-channel call, in all three formats at D = 1, 2 and 4, and a mono file
under every mix is the one-channel call; the float64 mid against the NumPy restatement on the MDCT lines
(tests/mix_restatement.py) to 1e-12 of the stereo file's peak, the bar tests/test_gpu_decode.py and the reduced-rate tests hold
the inverse transform to; the other two formats as conversions of the call's own float64 window; independence of order,
company, slab size and how a window is cut; the chunks parsed per mix; damage inside, outside and in the chunk a mix does
not parse; refusals; the command line.  Files: tests/mix_restatement.files -- per kit setting B, C, D, K the stereo Huffman,
stereo raw, mono, one-block mono and ONE-BLOCK STEREO file, and the default-setting five-hop stereo file.  Everything
oracle-side is computed once per module and never written to.
"""
import re
import struct

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import mix_restatement as MR
import reduced_restatement as RR
import settings_kit as SK
from oracle import decode as odec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = MR.KIT_SIDS + ("default",)
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
FORMATS = (torch.int16, torch.float32, torch.float64)
MIXES = ("mid", "left", "right")
FN = "mrc_pac_store_decode_window_mix"


class _Kitchen:
    """one setting: its handle, files, store, index, and per file and D the restatements in the store's coordinates (the
    MDCT's delay dropped), computed on first use"""

    def __init__(self, sid):
        from mrcaudiocodec_amd import pacfile as ppac
        from mrcaudiocodec_amd.store import PacStore
        F = MR.files(sid)
        self.sid, self.L, self.S, self.blksw = sid, F["L"], F["S"], F["blksw"]
        self.files, self.nch, self.full = F["files"], F["nch"], F["full"]
        if sid == "default":
            self.h, cfg = kit.handle(), ppac.make_config()
        else:
            self.h, cfg = kit.handle(**SK.handle_kwargs(sid)), SK.config(sid)
        self.index = [ppac.index(b, cfg) for b in self.files]
        assert [int(ix["n_channels"]) for ix in self.index] == self.nch
        self.store = PacStore(self.h, self.files)
        self._ref = {}

    def ref(self, f, D):
        """the file's channels, float64 [nCh][n_samples / D], read-only"""
        if ("ref", f, D) not in self._ref:
            x = np.ascontiguousarray(RR.decode(self.files[f], self.S, self.blksw, D)[:, self.L // D:])
            x.setflags(write=False)
            self._ref[("ref", f, D)] = x
        return self._ref[("ref", f, D)]

    def mid(self, f, D):
        """what mix="mid" is held against, float64 [n_samples / D]: a stereo file's mid on the lines, a mono file's channel"""
        if ("mid", f, D) not in self._ref:
            if self.nch[f] == 2:
                x = np.ascontiguousarray(MR.mid_decode(self.files[f], self.S, self.blksw, D)[self.L // D:])
            else:
                x = self.ref(f, D)[0].copy()
            x.setflags(write=False)
            self._ref[("mid", f, D)] = x
        return self._ref[("mid", f, D)]

    def stereo(self):
        return [f for f in range(len(self.files)) if self.nch[f] == 2]

    def boundaries(self, f, D):
        ix = self.index[f]
        p = (ix["block_start"].astype(np.int64) - self.L) // D
        return sorted({0, int(ix["n_samples"]) // D} | {int(v) for v in p})

    def items(self, D):
        """(file, start) at every reduced block boundary and +- 1 around it, a negative start and one past the end"""
        out = []
        for f in range(len(self.files)):
            n = int(self.index[f]["n_samples"]) // D
            out += [(f, s + d) for s in self.boundaries(f, D) for d in (-1, 0, 1)] + [(f, -37), (f, n + 5)]
        return out


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


def _cut(ref, start, window):
    out = np.zeros(ref.shape[:-1] + (window,), ref.dtype)
    lo, hi = max(start, 0), min(start + window, ref.shape[-1])
    if hi > lo:
        out[..., lo - start:hi - start] = ref[..., lo:hi]
    return out


def _raw(k, D, mix, items, window, dtype):
    """the new entry point itself, rate_divisor and mix as given -> (status, tensor filled with 77 before the call)"""
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import _formats
    files = np.ascontiguousarray([f for f, _ in items], dtype=np.int64)
    starts = np.ascontiguousarray([s for _, s in items], dtype=np.int64)
    out = torch.full((len(items), 1, window), 77, dtype=dtype, device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_mix(k.store._s, D, mix, len(items), files.ctypes.data, starts.ctypes.data, window,
                                                  _formats()[dtype], out.data_ptr(), None)
    return rc, out


def _needed_blocks(ix, start, window, L, D):
    """the overlap rule in reduced coordinates -> the indices of the needed blocks"""
    p, n = ix["block_start"] // D, (ix["block_a"] + ix["block_b"]) // D
    return np.flatnonzero((p < start + window + L // D) & (p + n > start + L // D))


def _chunks_wanted(ix, blocks, mix):
    """section "Work" of the contract: a joint block has both chunks parsed, the last block of a stereo file two for mid and
    one for left / right, a mono file's block its one"""
    nch, nb = int(ix["n_channels"]), int(ix["n_blocks"])
    if nch == 1:
        return len(blocks)
    n_joint = nb - 1 if nb > 1 else 0
    return sum(2 if (b < n_joint or mix == "mid") else 1 for b in blocks)


def _same(a, b):
    return torch.equal(a, b) and (a.dtype == torch.int16 or torch.equal(torch.signbit(a), torch.signbit(b)))


# ------------------------------------------------------------------ 1: left / right, and mono files, bit for bit
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_left_and_right_are_the_two_channel_calls_channels(kitchen, D):
    k = kitchen
    items = k.items(D)
    files, starts = zip(*items)
    mono = [i for i, (f, _) in enumerate(items) if k.nch[f] == 1]
    for dtype in FORMATS:
        for window in (3 * k.S // D + 5, k.L // D + 3):
            both = k.store.decode_window(files, starts, window, channels=2, dtype=dtype, rate_divisor=D)
            left = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, mix="left")
            right = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, mix="right", channels=1)
            assert tuple(left.shape) == tuple(right.shape) == (len(items), 1, window) and left.dtype == dtype
            assert _same(left[:, 0], both[:, 0]) and _same(right[:, 0], both[:, 1]), (k.sid, D, dtype, window)
            assert bool(both.any())
            if mono:                                                 # a mono file gives its one channel under every mix
                alone = k.store.decode_window([files[i] for i in mono], [starts[i] for i in mono], window, channels=1, dtype=dtype,
                                              rate_divisor=D)
                for mix in MIXES:
                    got = k.store.decode_window([files[i] for i in mono], [starts[i] for i in mono], window, dtype=dtype,
                                                rate_divisor=D, mix=mix)
                    assert _same(got, alone), (k.sid, D, dtype, mix)
                mid = k.store.decode_window(files, starts, window, dtype=dtype, rate_divisor=D, mix="mid")
                assert _same(mid[mono], alone)


# ------------------------------------------------------------------ 2: the float64 mid against the restatement
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_f64_mid_equals_the_restatement(kitchen, D):
    k = kitchen
    margin = 2 * k.L // D + 7
    # (a mono file under mid is the one-channel call bit for bit, test 1: the bar here is for the stereo files)
    peak = {f: np.abs(k.ref(f, D)).max() for f in k.stereo()}                   # the STEREO file's peak, both channels
    for f in k.stereo():
        want = k.mid(f, D)
        n = want.shape[0]
        assert n == int(k.index[f]["n_samples"]) // D
        whole = k.store.decode_window([f], [-margin], n + 2 * margin, dtype=torch.float64, rate_divisor=D, mix="mid")[0].cpu().numpy()
        assert whole.shape == (1, n + 2 * margin)
        err = np.abs(whole[0, margin:margin + n] - want).max()
        print("%s file %d D = %d: max |delta| = %.3g of the peak" % (k.sid, f, D, err / peak[f]))
        assert err <= 1e-12 * peak[f], (k.sid, f, D, err / peak[f])
        ref = k.ref(f, D)                                            # ... which is the mean of the two channels
        assert np.abs(whole[0, margin:margin + n] - 0.5 * (ref[0] + ref[1])).max() <= 1e-12 * peak[f]
        outside = np.concatenate([whole[:, :margin], whole[:, margin + n:]], axis=1)
        assert not outside.any() and not np.signbit(outside).any()
    items = k.items(D)
    files, starts = zip(*items)
    window = 3 * k.S // D + 5
    got = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, mix="mid").cpu().numpy()
    assert got.shape == (len(items), 1, window)
    for i, (f, s) in enumerate(items):
        want = _cut(k.mid(f, D), s, window)
        if k.nch[f] == 2:
            assert np.abs(got[i, 0] - want).max() <= 1e-12 * peak[f], (k.sid, f, s, D)
        t = s + np.arange(window)
        out = (t < 0) | (t >= k.mid(f, D).shape[0])
        assert not got[i, 0][out].any() and not np.signbit(got[i, 0][out]).any()


# ------------------------------------------------------------------ 3: the other formats
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_formats_are_conversions_of_the_f64_mid(kitchen, D):
    k = kitchen
    items = k.items(D)
    files, starts = zip(*items)
    window = k.L // D + 9
    f64 = k.store.decode_window(files, starts, window, dtype=torch.float64, rate_divisor=D, mix="mid").cpu().numpy()
    i16 = k.store.decode_window(files, starts, window, rate_divisor=D, mix="mid")
    f32 = k.store.decode_window(files, starts, window, dtype=torch.float32, rate_divisor=D, mix="mid")
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32 and f64.any()
    assert tuple(i16.shape) == tuple(f32.shape) == f64.shape == (len(items), 1, window)
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))        # the code of the float64 mid, not the mean of two codes
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))
    assert np.array_equal(np.signbit(f32.cpu().numpy()), np.signbit(f64))


# ------------------------------------------------------------------ 4: independence
@pytest.mark.parametrize("D", [1, 2])
def test_mid_does_not_depend_on_order_company_slabs_or_cuts(kitchen, D):
    k = kitchen
    items = k.items(D)
    files, starts = map(np.array, zip(*items))
    window = 2 * k.S // D + 6
    kw = dict(dtype=torch.float64, rate_divisor=D, mix="mid")
    base = k.store.decode_window(files, starts, window, **kw)
    assert k.store.stats()["slabs"] == 1
    perm = np.random.default_rng(3).permutation(len(items))
    back = torch.from_numpy(np.argsort(perm)).to(base.device)
    assert _same(k.store.decode_window(files[perm], starts[perm], window, **kw)[back], base)
    for i in range(len(items)):
        assert _same(k.store.decode_window(files[i:i + 1], starts[i:i + 1], window, **kw)[0], base[i])
    try:
        k.h.set_option(SLAB_OPTION, 3 * window)                  # three items per slab
        got = k.store.decode_window(files, starts, window, **kw)
        assert k.store.stats()["slabs"] == (len(items) + 2) // 3 and _same(got, base)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    half = window // 2
    left = k.store.decode_window(files, starts, half, **kw)
    right = k.store.decode_window(files, starts + half, window - half, **kw)
    assert _same(torch.cat([left, right], dim=2), base)


# ------------------------------------------------------------------ 5: work
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_chunks_parsed_follow_the_mix(kitchen, D):
    k = kitchen
    seen = set()
    cases = [(f, s, w) for f in range(len(k.files)) for s in k.boundaries(f, D) for w in (1, k.S // D)]
    cases += [(f, -3 * k.L, 5) for f in range(len(k.files))]         # nothing needed
    for f in k.stereo():                                             # only the last block of a stereo file
        n = int(k.index[f]["n_samples"]) // D
        cases.append((f, n - 5, 20))
        assert _needed_blocks(k.index[f], n - 5, 20, k.L, D).tolist() == [int(k.index[f]["n_blocks"]) - 1]
    for (f, s, w) in cases:
        blocks = _needed_blocks(k.index[f], s, w, k.L, D)
        for mix in MIXES:
            k.store.decode_window([f], [s], w, rate_divisor=D, mix=mix)
            st = k.store.stats()
            want = _chunks_wanted(k.index[f], blocks, mix)
            assert st["chunks_parsed"] == want, (k.sid, f, s, w, D, mix)
            assert (st["decode_launches"] == 0) == (len(blocks) == 0)
            seen.add((mix, want))
    for f in k.stereo():
        n, last = int(k.index[f]["n_samples"]) // D, int(k.index[f]["n_blocks"]) - 1
        got = {}
        for mix in MIXES:
            k.store.decode_window([f], [n - 5], 20, rate_divisor=D, mix=mix)
            got[mix] = k.store.stats()["chunks_parsed"]
        assert got == {"mid": 2, "left": 1, "right": 1}, (k.sid, f, last)
        k.store.decode_window([f], [0], n, rate_divisor=D, mix="mid")     # the whole file at mid: every chunk
        assert k.store.stats()["chunks_parsed"] == 2 * int(k.index[f]["n_blocks"])
    assert len({w for (_, w) in seen}) > 2


# ------------------------------------------------------------------ 6: damage
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_damage_counts_only_in_what_a_window_parses(kitchen, D):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    ix, L = k.index[0], k.L
    reason = re.escape("table id not in {0..3, 15}")
    j = int(ix["n_blocks"]) - 2                                   # the last joint block
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                             # table id 4
    pj = int(ix["block_start"][j])
    peak = np.abs(k.ref(0, D)).max()
    with PacStore(k.h, [bytes(bad)]) as store:
        w = (int(ix["block_start"][j - 1]) - L) // D              # [0, w) needs the blocks that start before w + L / D
        assert w > 0 and len(_needed_blocks(ix, 0, w, L, D)) == j - 1
        got = store.decode_window([0], [0], w, dtype=torch.float64, rate_divisor=D, mix="mid")[0, 0].cpu().numpy()
        assert np.abs(got - k.mid(0, D)[:w]).max() <= 1e-12 * peak
        with pytest.raises(MrcError, match=r"%s: file 0: chunk at byte %d: %s" % (FN, at - 4, reason)) as e:
            store.decode_window([0], [(pj - L) // D], 3, rate_divisor=D, mix="mid")
        assert e.value.code == -1
    # the RIGHT chunk of the last block: not in the plan of mix="left" on a window that needs only that block
    last = int(ix["n_blocks"]) - 1
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][last, 1]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40
    n = int(ix["n_samples"]) // D
    assert _needed_blocks(ix, n - 5, 20, L, D).tolist() == [last]
    with PacStore(k.h, [bytes(bad)]) as store:
        got = store.decode_window([0], [n - 5], 20, dtype=torch.float64, rate_divisor=D, mix="left")[0, 0].cpu().numpy()
        assert store.stats()["chunks_parsed"] == 1
        assert np.array_equal(got, k.store.decode_window([0], [n - 5], 20, dtype=torch.float64, rate_divisor=D, mix="left")[0, 0].cpu().numpy())
        with pytest.raises(MrcError, match=r"%s: file 0: chunk at byte %d: %s" % (FN, at - 4, reason)) as e:
            store.decode_window([0], [n - 5], 20, rate_divisor=D, mix="mid")
        assert e.value.code == -1


# ------------------------------------------------------------------ 7: refusals
def test_refusals(kitchen):
    from mrcaudiocodec_amd import MrcError, _lib
    k = kitchen
    for mix in (3, -1):
        rc, out = _raw(k, 1, mix, [(0, 0)], 16, torch.float64)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all())
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert ("mix %d" % mix) in text and FN in text, text
    for D in (0, 3, 8, -2):
        rc, out = _raw(k, D, _lib.MRC_MIX_MID, [(0, 0)], 16, torch.float64)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all())
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert ("rate_divisor %d" % D) in text and FN in text, text
    for mix in (_lib.MRC_MIX_MID, _lib.MRC_MIX_LEFT, _lib.MRC_MIX_RIGHT):     # the raw call, taken
        rc, out = _raw(k, 2, mix, [(0, 0), (0, 7)], 16, torch.float64)
        assert rc == 0 and not bool((out == 77).any())
    # the old calls still refuse a stereo file in a one-channel call
    out = torch.full((1, 1, 32), 12345, dtype=torch.int16, device=torch.device("cuda", 0))
    for D in (1, 2, 4):
        with pytest.raises(MrcError, match=r"item 0: file 0 is stereo") as e:
            k.store.decode_window([0], [0], 32, channels=1, out=out, rate_divisor=D)
        assert e.value.code == -1 and bool((out == 12345).all())
    # Python side: before any library call
    for bad_out in (torch.empty((1, 2, 32), dtype=torch.int16, device=out.device), torch.empty((1, 32), dtype=torch.int16, device=out.device)):
        with pytest.raises(ValueError, match="out must be a contiguous"):
            k.store.decode_window([0], [0], 32, out=bad_out, mix="mid")
    with pytest.raises(ValueError, match="channels must be None or 1"):
        k.store.decode_window([0], [0], 32, channels=2, mix="mid")
    with pytest.raises(ValueError, match="mix must be None"):
        k.store.decode_window([0], [0], 32, mix="side")
    got = k.store.decode_window([0], [0], 32, out=out, mix="mid")
    assert got is out and not bool((out == 12345).all())


# ------------------------------------------------------------------ 8: the command line
def test_cli_writes_one_channel(tmp_path):
    from mrcaudiocodec_amd import cli
    k = _kitchen("default")
    src, dst = str(tmp_path / "x.pac"), str(tmp_path / "x.wav")
    with open(src, "wb") as f:
        f.write(k.files[0])
    n = int(k.index[0]["n_samples"]) // 2
    want = k.store.decode_window([0], [0], n, rate_divisor=2, mix="mid")[0].cpu().numpy()
    f64 = k.store.decode_window([0], [0], n, dtype=torch.float64, rate_divisor=2, mix="mid")[0].cpu().numpy()
    assert want.shape == (1, n) and np.array_equal(want, odec.pcm16(f64)) and want.any()
    cli.main(["-d", src, dst, "--mix", "mid", "--rate-divisor", "2"])
    wav = open(dst, "rb").read()
    assert struct.unpack("<L", wav[24:28])[0] == 48000 // 2 and struct.unpack("<H", wav[22:24])[0] == 1
    assert wav == cli.wav_bytes(want, 24000)
    cli.main(["-d", src, dst, "--mix", "left", "--start", "100", "--samples", "300"])
    whole = k.store.decode_window([0], [0], 2 * n, channels=2)[0].cpu().numpy()
    assert open(dst, "rb").read() == cli.wav_bytes(whole[:1, 100:400], 48000)
    cli.main(["-d", src, dst, "--mix", "right"])
    assert open(dst, "rb").read() == cli.wav_bytes(whole[1:], 48000)
