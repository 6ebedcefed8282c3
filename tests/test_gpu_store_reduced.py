"""
GPU tests of the store's reduced-rate windows (mrc_pac_store_decode_window_reduced, PacStore.decode_window(rate_divisor=),
cli -d --rate-divisor): at D = 1 the bits of mrc_pac_store_decode_window; at D = 2 and 4 the float64 windows against the
NumPy restatement from the oracle's functions (tests/reduced_restatement.py) to 1e-12 of the file's peak, the bar
tests/test_gpu_decode.py holds the IMDCT to; the other two formats as conversions of the call's own float64 window;
independence of order, company, slab size and how a window is cut; that work follows the windows, in reduced coordinates;
refusals; the command line.  Files: the kit's stereo Huffman, stereo raw and mono files at settings B, C, D and K
(tests/settings_kit.py) with a one-block mono file each, and a default-setting (1024 / 128) stereo file of five hops from
the oracle's encoder.  Everything oracle-side is computed once per module and never written to.
"""
import re
import struct

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import reduced_restatement as RR
import settings_kit as SK
from oracle import codec as ocodec, decode as odec, pacfile as opac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = ("B", "C", "D", "K", "default")
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
FORMATS = (torch.int16, torch.float32, torch.float64)


def _oracle_stereo_file(L, S, seed, rate=48000):
    """a five-hop stereo file at block lengths L / S from oracle.pacfile.encode_stereo_stream: (L,L), (L,L), (L,S), (S,S)..,
    (S,L), (L,L) and Close()'s block; a tone common to both channels (M/S bands) over independent noise (L/R bands)"""
    cp = ocodec.default_params(sampleRate=rate, nChannels=2, targetBitsPerSample=2.86)
    cp.nMDCTLines = cp.nSamplesPerBlock = cp.a = cp.b = L
    cp.nSamplesShort = S
    cp.sfBands = ocodec.bands_for_block(L, L, L, rate)
    cp.bitReservoir = 0
    ab = [(L, L)] * 2 + [(L, S)] + [(S, S)] * (L // S - 1) + [(S, L)] + [(L, L)]
    offs = np.concatenate([[0], np.cumsum([a for a, _ in ab])[:-1]])
    n = 5 * L
    t = np.arange(n)
    tone = 0.25 * np.sin(2 * np.pi * 1000.0 / rate * t) + 0.075 * np.sin(2 * np.pi * 5200.0 / rate * t)
    sigma = np.where(t < n // 2, 0.05, 2e-4)
    x = tone[None] + sigma[None] * np.random.default_rng(seed).standard_normal((2, n))
    pcm = np.zeros((2, n + L), np.int16)
    pcm[:, L:] = np.clip(np.rint(x * 32767.5), -32767, 32767).astype(np.int16)
    return opac.encode_stereo_stream(SK.to_float(pcm), [(int(o), a, b) for o, (a, b) in zip(offs, ab)], cp, huffman=True)


def _one_block(buf, ix):
    """the file's header and its last block alone"""
    return buf[:int(ix["chunk_offset"][0, 0])] + buf[int(ix["chunk_offset"][-1, 0]):]


class _Kitchen:
    """one setting: its handle, files, store, index, and the restatement of every file at every D in the coordinates of the
    store (the MDCT's delay dropped), computed on first use"""

    def __init__(self, sid):
        from mrcaudiocodec_amd import pacfile as ppac
        from mrcaudiocodec_amd.store import PacStore
        self.sid = sid
        if sid == "default":
            self.L, self.S, self.blksw = 1024, 128, (1, 1)
            self.h, cfg = kit.handle(), ppac.make_config()
            self.files = [_oracle_stereo_file(1024, 128, 5)]
            self.full = [True]                                   # files that must hold every shape
        else:
            (self.L, self.S), self.blksw = SK.lengths(sid), SK.blksw(sid)
            self.h, cfg = kit.handle(**SK.handle_kwargs(sid)), SK.config(sid)
            mono = SK.oracle_file(sid, 1, True)["data"]
            self.files = [SK.oracle_file(sid, 2, True)["data"], SK.oracle_file(sid, 2, False)["data"], mono,
                          _one_block(mono, ppac.index(mono, cfg))]
            self.full = [True, True, True, False]
        self.index = [ppac.index(b, cfg) for b in self.files]
        self.store = PacStore(self.h, self.files)
        self._ref = {}

    def ref(self, f, D):
        """float64 [nCh][n_samples / D], read-only"""
        if (f, D) not in self._ref:
            x = np.ascontiguousarray(RR.decode(self.files[f], self.S, self.blksw, D)[:, self.L // D:])
            x.setflags(write=False)
            self._ref[(f, D)] = x
        return self._ref[(f, D)]

    def boundaries(self, f, D):
        """the reduced block boundaries of file f in the store's coordinates, and both file ends"""
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


@pytest.fixture(scope="module", params=SIDS)
def kitchen(request):
    sid = request.param
    if sid not in _KITCHENS:
        _KITCHENS[sid] = _Kitchen(sid)
    return _KITCHENS[sid]


@pytest.fixture(scope="module", autouse=True)
def stores_closed_after_module():
    yield
    for k in _KITCHENS.values():
        k.store.close()
    _KITCHENS.clear()


def _cut(ref, start, window):
    out = np.zeros((ref.shape[0], window), ref.dtype)
    lo, hi = max(start, 0), min(start + window, ref.shape[1])
    if hi > lo:
        out[:, lo - start:hi - start] = ref[:, lo:hi]
    return out


def _raw(k, D, items, window, channels, dtype):
    """the new entry point itself, rate_divisor as given -> (status, tensor)"""
    from mrcaudiocodec_amd import _lib
    from mrcaudiocodec_amd.store import _formats
    files = np.ascontiguousarray([f for f, _ in items], dtype=np.int64)
    starts = np.ascontiguousarray([s for _, s in items], dtype=np.int64)
    out = torch.full((len(items), channels, window), 77, dtype=dtype, device=torch.device("cuda", 0))
    rc = _lib.lib.mrc_pac_store_decode_window_reduced(k.store._s, D, len(items), files.ctypes.data, starts.ctypes.data, window,
                                                      channels, _formats()[dtype], out.data_ptr(), None)
    return rc, out


def _needed(ix, start, window, L, D):
    """the overlap rule in reduced coordinates"""
    p, n = ix["block_start"] // D, (ix["block_a"] + ix["block_b"]) // D
    return int(np.count_nonzero((p < start + window + L // D) & (p + n > start + L // D)))


# ------------------------------------------------------------------ 0: the files are what the tests need
def test_files_hold_every_shape_and_both_kinds_of_band(kitchen):
    k = kitchen
    L, S = k.L, k.S
    for f, buf in enumerate(k.files):
        _, blks = RR.blocks(buf, S, k.blksw)
        if not k.full[f]:
            assert len(blks) == 1 and k.index[f]["n_channels"] == 1 and k.index[f]["n_samples"] == L
            continue
        assert {(b["a"], b["b"]) for b in blks} == {(L, L), (L, S), (S, S), (S, L)}
        if k.index[f]["n_channels"] == 2:
            ms = np.concatenate([b["ms"] for b in blks if b["joint"]])
            assert (ms == 1).any() and (ms == 0).any()
            if k.sid != "default":                               # the oracle's integers as the kit kept them
                kept = SK.oracle_file(k.sid, 2, f == 0)["blocks"]
                assert np.array_equal(ms, np.concatenate([b["ms"] for b in kept if b["joint"]]))
        assert int(k.index[f]["n_samples"]) % 4 == 0 and all(int(v) % 4 == 0 for v in k.index[f]["block_start"])
    assert k.store.n_samples_at(2).tolist() == [int(ix["n_samples"]) // 2 for ix in k.index]
    assert k.store.n_samples_at(4).tolist() == [int(ix["n_samples"]) // 4 for ix in k.index]


# ------------------------------------------------------------------ 1: D = 1 is the existing call
def test_divisor_one_is_decode_window_bit_for_bit(kitchen):
    k = kitchen
    items = k.items(1)
    files, starts = zip(*items)
    for dtype in FORMATS:
        for window in (200, k.L + 3):
            rc, got = _raw(k, 1, items, window, 2, dtype)
            assert rc == 0
            want = k.store.decode_window(files, starts, window, channels=2, dtype=dtype)
            assert torch.equal(got, want)
            if dtype != torch.int16:
                assert torch.equal(torch.signbit(got), torch.signbit(want))
    assert torch.equal(k.store.decode_window(files, starts, 64, channels=2, rate_divisor=1),
                       k.store.decode_window(files, starts, 64, channels=2))


# ------------------------------------------------------------------ 2: float64 against the restatement
@pytest.mark.parametrize("D", [2, 4])
def test_f64_equals_the_restatement(kitchen, D):
    k = kitchen
    margin = 2 * k.L // D + 7
    for f in range(len(k.files)):
        ref = k.ref(f, D)
        n, nch = ref.shape[1], ref.shape[0]
        assert n == int(k.index[f]["n_samples"]) // D
        peak = np.abs(ref).max()
        whole = k.store.decode_window([f], [-margin], n + 2 * margin, dtype=torch.float64, rate_divisor=D)[0].cpu().numpy()
        assert whole.shape == (nch, n + 2 * margin)
        err = np.abs(whole[:, margin:margin + n] - ref).max()
        print("%s file %d D = %d: max |delta| = %.3g of the peak" % (k.sid, f, D, err / peak))
        assert err <= 1e-12 * peak, (k.sid, f, D, err / peak)
        outside = np.concatenate([whole[:, :margin], whole[:, margin + n:]], axis=1)
        assert not outside.any() and not np.signbit(outside).any()
    items = k.items(D)
    files, starts = zip(*items)
    window = 3 * k.S // D + 5
    got = k.store.decode_window(files, starts, window, channels=2, dtype=torch.float64, rate_divisor=D).cpu().numpy()
    for i, (f, s) in enumerate(items):
        ref = k.ref(f, D)
        want = _cut(ref, s, window)
        assert np.abs(got[i] - want).max() <= 1e-12 * np.abs(ref).max(), (k.sid, f, s, D)
        t = s + np.arange(window)
        out = (t < 0) | (t >= ref.shape[1])
        assert not got[i][:, out].any() and not np.signbit(got[i][:, out]).any()


# ------------------------------------------------------------------ 3: the other formats
@pytest.mark.parametrize("D", [2, 4])
def test_formats_are_conversions_of_the_f64_window(kitchen, D):
    k = kitchen
    items = k.items(D)
    files, starts = zip(*items)
    window = k.L // D + 9
    f64 = k.store.decode_window(files, starts, window, channels=2, dtype=torch.float64, rate_divisor=D).cpu().numpy()
    i16 = k.store.decode_window(files, starts, window, channels=2, rate_divisor=D)
    f32 = k.store.decode_window(files, starts, window, channels=2, dtype=torch.float32, rate_divisor=D)
    assert i16.dtype == torch.int16 and f32.dtype == torch.float32 and f64.any()
    assert np.array_equal(i16.cpu().numpy(), odec.pcm16(f64))
    assert np.array_equal(f32.cpu().numpy(), f64.astype(np.float32))
    mono = [i for i, (f, _) in enumerate(items) if k.index[f]["n_channels"] == 1]
    if mono:                                                     # a mono file fills both channels; alone, it has one
        assert np.array_equal(f64[mono][:, 0], f64[mono][:, 1])
        alone = k.store.decode_window([files[i] for i in mono], [starts[i] for i in mono], window, dtype=torch.float64,
                                      rate_divisor=D)
        assert tuple(alone.shape) == (len(mono), 1, window) and np.array_equal(alone.cpu().numpy()[:, 0], f64[mono][:, 0])


# ------------------------------------------------------------------ 4: independence
@pytest.mark.parametrize("D", [2, 4])
def test_result_does_not_depend_on_order_company_slabs_or_cuts(kitchen, D):
    k = kitchen
    items = k.items(D)
    files, starts = map(np.array, zip(*items))
    window = 2 * k.S // D + 6
    kw = dict(channels=2, dtype=torch.float64, rate_divisor=D)
    base = k.store.decode_window(files, starts, window, **kw)
    assert k.store.stats()["slabs"] == 1
    same = lambda a, b: torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
    perm = np.random.default_rng(3).permutation(len(items))
    back = torch.from_numpy(np.argsort(perm)).to(base.device)
    assert same(k.store.decode_window(files[perm], starts[perm], window, **kw)[back], base)
    for i in range(len(items)):
        assert same(k.store.decode_window(files[i:i + 1], starts[i:i + 1], window, **kw)[0], base[i])
    try:
        k.h.set_option(SLAB_OPTION, 3 * window)                  # three items per slab
        got = k.store.decode_window(files, starts, window, **kw)
        assert k.store.stats()["slabs"] == (len(items) + 2) // 3 and same(got, base)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)
    half = window // 2
    left = k.store.decode_window(files, starts, half, **kw)
    right = k.store.decode_window(files, starts + half, window - half, **kw)
    assert same(torch.cat([left, right], dim=2), base)


# ------------------------------------------------------------------ 5: work follows the windows
@pytest.mark.parametrize("D", [2, 4])
def test_only_the_needed_chunks_are_parsed(kitchen, D):
    k = kitchen
    rng = np.random.default_rng(11 + D)
    seen = set()
    cases = [(f, s, w) for f in range(len(k.files)) for s in k.boundaries(f, D) for w in (1, k.S // D)]
    cases += [(int(rng.integers(0, len(k.files))), int(rng.integers(-k.L, 7 * k.L // D)), int(rng.choice([1, 100, k.L // D, 3 * k.L // D])))
              for _ in range(12)]
    for (f, s, w) in cases:
        k.store.decode_window([f], [s], w, rate_divisor=D)
        want = _needed(k.index[f], s, w, k.L, D) * int(k.index[f]["n_channels"])
        st = k.store.stats()
        assert st["chunks_parsed"] == want, (k.sid, f, s, w, D)
        assert (st["decode_launches"] == 0) == (want == 0)
        seen.add(want)
    assert len(seen) > 3
    n = int(k.index[0]["n_samples"]) // D
    k.store.decode_window([0], [0], n, rate_divisor=D)            # the whole file: every chunk
    assert k.store.stats()["chunks_parsed"] == int(k.index[0]["n_blocks"]) * int(k.index[0]["n_channels"])


@pytest.mark.parametrize("D", [2, 4])
def test_damage_counts_only_inside_a_window(kitchen, D):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    k = kitchen
    ix, L = k.index[0], k.L
    j = int(ix["n_blocks"]) - 2                                   # the last joint block
    bad = bytearray(k.files[0])
    at = int(ix["chunk_offset"][j, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                             # table id 4
    pj = int(ix["block_start"][j])
    with PacStore(k.h, [bytes(bad)]) as store:
        w = (int(ix["block_start"][j - 1]) - L) // D              # [0, w) needs the blocks that start before w + L / D
        assert w > 0 and _needed(ix, 0, w, L, D) == j - 1
        got = store.decode_window([0], [0], w, dtype=torch.float64, rate_divisor=D)[0].cpu().numpy()
        assert np.abs(got - k.ref(0, D)[:, :w]).max() <= 1e-12 * np.abs(k.ref(0, D)).max()
        with pytest.raises(MrcError, match=r"file 0: chunk at byte %d: %s" % (at - 4, re.escape("table id not in {0..3, 15}"))) as e:
            store.decode_window([0], [(pj - L) // D], 3, rate_divisor=D)
        assert e.value.code == -1


# ------------------------------------------------------------------ 6: refusals
def test_refusals_come_before_any_device_work(kitchen):
    from mrcaudiocodec_amd import MrcError, _lib
    k = kitchen
    for D in (0, 3, 8, -2):
        rc, out = _raw(k, D, [(0, 0)], 16, 2, torch.float64)
        assert rc == _lib.MRC_ERR_INVALID and bool((out == 77).all())
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert ("rate_divisor %d" % D) in text and "mrc_pac_store_decode_window_reduced" in text
        with pytest.raises(MrcError, match="rate_divisor %d" % D):
            k.h._check(rc)
    mono = [f for f in range(len(k.files)) if k.index[f]["n_channels"] == 1]
    items = ([mono[0]] if mono else []) + [0]
    out = torch.full((len(items), 1, 32), 12345, dtype=torch.int16, device=torch.device("cuda", 0))
    for D in (2, 4):
        with pytest.raises(MrcError, match=r"item %d: file 0 is stereo" % (len(items) - 1)) as e:
            k.store.decode_window(items, [0] * len(items), 32, channels=1, out=out, rate_divisor=D)
        assert e.value.code == -1 and bool((out == 12345).all())
    for bad in (0, 3, 8, -2, 2.0):
        with pytest.raises(ValueError, match="rate_divisor"):
            k.store.decode_window([0], [0], 16, rate_divisor=bad)


@pytest.mark.parametrize("L,S", [(96, 24), (324, 108)])
def test_shapes_that_divide_by_two_and_not_by_four(L, S):
    """block lengths whose four shapes have a half-rate synthesis shape and no quarter-rate one: D = 4 is refused with the
    shape named, D = 2 decodes and equals the restatement.  (96, 24): (96 + 24) / 4 = 30 has a factor 5, so the handle
    itself may refuse these lengths; (324, 108) = 4 (81, 27): every shape and its half factor into 2s and 3s, and a
    quarter of them has a sum or a difference that 4 does not divide."""
    from mrcaudiocodec_amd import Handle, MrcError
    from mrcaudiocodec_amd.store import PacStore
    try:
        h = Handle(device_id=0, n_mdct_lines=L, n_short=S)
    except MrcError as e:
        pytest.skip("Handle refuses n_mdct_lines=%d, n_short=%d: %s" % (L, S, e))
    try:
        buf = _oracle_stereo_file(L, S, 9)
        with PacStore(h, [buf]) as store:
            n = int(store.n_samples[0])
            assert n == 6 * L                               # five hops and the tail Close() flushed
            with pytest.raises(MrcError, match=r"rate_divisor 4: block shape \(%d,%d\)" % (L, L)) as e:
                store.decode_window([0], [0], 16, dtype=torch.float64, rate_divisor=4)
            assert e.value.code == -1
            ref = RR.decode(buf, S, (1, 1), 2)[:, L // 2:]
            got = store.decode_window([0], [-5], n // 2 + 10, dtype=torch.float64, rate_divisor=2)[0].cpu().numpy()
            assert np.abs(got[:, 5:5 + n // 2] - ref).max() <= 1e-12 * np.abs(ref).max()
            assert not got[:, :5].any() and not got[:, 5 + n // 2:].any()
            full = odec.decode_pac(buf, S, (1, 1))[1][:, L:]
            got1 = store.decode_window([0], [0], n, dtype=torch.float64)[0].cpu().numpy()
            assert np.abs(got1 - full).max() <= 1e-12 * np.abs(full).max()
    finally:
        h.close()


# ------------------------------------------------------------------ 7: the command line
def test_cli_decodes_at_half_rate(tmp_path):
    from mrcaudiocodec_amd import cli
    k = _KITCHENS.get("default") or _KITCHENS.setdefault("default", _Kitchen("default"))
    src, dst = str(tmp_path / "x.pac"), str(tmp_path / "x.wav")
    with open(src, "wb") as f:
        f.write(k.files[0])
    n = int(k.index[0]["n_samples"]) // 2
    want = k.store.decode_window([0], [0], n, rate_divisor=2)[0].cpu().numpy()
    f64 = k.store.decode_window([0], [0], n, dtype=torch.float64, rate_divisor=2)[0].cpu().numpy()
    assert np.array_equal(want, odec.pcm16(f64))
    cli.main(["-d", src, dst, "--rate-divisor", "2"])
    wav = open(dst, "rb").read()
    assert struct.unpack("<L", wav[24:28])[0] == 48000 // 2 and struct.unpack("<H", wav[22:24])[0] == 2
    assert wav == cli.wav_bytes(want, 24000)
    cli.main(["-d", src, dst, "--rate-divisor", "4", "--start", "100", "--samples", "300"])
    want4 = k.store.decode_window([0], [100], 300, rate_divisor=4)[0].cpu().numpy()
    assert open(dst, "rb").read() == cli.wav_bytes(want4, 12000)
