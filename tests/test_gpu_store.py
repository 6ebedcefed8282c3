"""
GPU tests of the resident `.pac` store (mrc_pac_store_*, mrcaudiocodec_amd/store.py): windows of six small files -- the
reference's block-switched stereo files, a chained mono encode with every block shape, one-block files and a header alone
-- against slices of the whole-file decodes, bit for bit in all three formats; the channel map; independence of item order
and slab size; that work follows the windows (chunks parsed = the overlap rule restated from pacfile.index); damage inside
and outside a window; refusals and lifetime; the command line's excerpt.
"""
import ctypes as C
import re

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import refgold as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

L, S = 1024, 128
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24


def _cut(ref, start, window):
    """samples [start, start + window) of ref [nCh][n], zeros (+0.0) outside"""
    out = np.zeros((ref.shape[0], window), ref.dtype)
    lo, hi = max(start, 0), min(start + window, ref.shape[1])
    if hi > lo:
        out[:, lo - start:hi - start] = ref[:, lo:hi]
    return out


@pytest.fixture(scope="module")
def kitchen():
    """the six files, their store, and the whole-file decodes every test slices (computed once, never written to)"""
    from mrcaudiocodec_amd import pacfile as ppac
    from mrcaudiocodec_amd.store import PacStore
    h = kit.handle()
    g = G.load("ref_pac.npz")
    a48, a48_raw = g["a48_pac"].tobytes(), g["a48_pac_raw"].tobytes()
    ab = [(L, L), (L, L), (L, S)] + [(S, S)] * 7 + [(S, L), (L, L)]
    offs = np.concatenate([[0], np.cumsum([a for a, _ in ab])[:-1]])
    mono = ppac.encode_mono_stream(h, kit.clicks(12, 5, True, 4), [(int(o), a, b) for o, (a, b) in zip(offs, ab)])
    ix_a, ix_m = ppac.index(a48), ppac.index(mono)
    head_a, head_m = ppac.read_header(a48)[3], ppac.read_header(mono)[3]
    one_stereo = a48[:head_a] + a48[int(ix_a["chunk_offset"][-1, 0]):]
    header_only = a48[:head_a]
    one_mono = mono[:head_m] + mono[int(ix_m["chunk_offset"][-1, 0]):]
    files = [a48, a48_raw, mono, one_stereo, header_only, one_mono]
    pcm = [np.ascontiguousarray(p) for p in h.decode_pac_pcm16(files, interleaved=False)]
    f64 = []
    for buf, p in zip(files, pcm):
        x = ppac.decode_pac(h, buf)[1][:, L:].cpu().numpy() if p.shape[1] else np.zeros(p.shape, np.float64)
        assert x.shape == p.shape
        f64.append(np.ascontiguousarray(x))
    for a in pcm + f64:
        a.setflags(write=False)
    store = PacStore(h, files)
    assert store.n_channels.tolist() == [2, 2, 1, 2, 2, 1] and store.n_blocks.tolist() == [35, 35, 13, 1, 0, 1]      # (the mono file: its 12 blocks + Close()'s)
    assert store.n_samples.tolist() == [p.shape[1] for p in pcm] == [14336, 14336, 6 * L, L, 0, L]
    assert store.device_bytes >= sum(len(f) for f in files)
    # the big call of tests 1, 2 and 4: every file, starts from before to past it
    items = [(f, s) for f in range(len(files)) for s in range(-1100, int(store.n_samples[f]) + 1100, 97)]
    yield dict(h=h, files=files, pcm=pcm, f64=f64, store=store, items=items, index=[ppac.index(b) for b in files])
    store.close()


def _expect(refs, items, window, channels):
    out = np.zeros((len(items), channels, window), refs[0].dtype)
    for k, (f, s) in enumerate(items):
        out[k] = _cut(refs[f], s, window)            # (a mono reference broadcasts to both channels)
    return out


def _singles(n):
    return [(w, s) for w in (1, 128, 1024, 5000, n + 2048) for s in (0, -1, n - 1, -w, n)]


def test_pcm16_equals_the_whole_file_decode(kitchen):
    store, pcm = kitchen["store"], kitchen["pcm"]
    files, starts = zip(*kitchen["items"])
    got = store.decode_window(files, starts, 300)
    assert got.dtype == torch.int16 and tuple(got.shape) == (len(files), 2, 300) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), _expect(pcm, kitchen["items"], 300, 2))
    st = store.stats()
    assert st["slabs"] == 1 and 1 <= st["decode_launches"] <= 8 and st["chunks_parsed"] > 0
    far = store.decode_window([0, 0, 2], [-2 ** 63, 2 ** 63 - 1, 2 ** 62], 64)    # no sum of these with a window is formed
    assert not bool(far.any()) and store.stats()["chunks_parsed"] == 0
    for f in range(len(pcm)):
        for w, s in _singles(pcm[f].shape[1]):
            one = store.decode_window([f], [s], w)                       # channels: the file's own
            assert tuple(one.shape) == (1, pcm[f].shape[0], w)
            assert np.array_equal(one[0].cpu().numpy(), _cut(pcm[f], s, w)), (f, w, s)


def test_f64_and_f32_equal_the_plane(kitchen):
    store, f64 = kitchen["store"], kitchen["f64"]
    files, starts = zip(*kitchen["items"])
    want = _expect(f64, kitchen["items"], 300, 2)
    got = store.decode_window(files, starts, 300, dtype=torch.float64).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    outside = np.array([[s + t < 0 or s + t >= f64[f].shape[1] for t in (0, 299)] for f, s in kitchen["items"]])
    assert outside.any() and not np.signbit(got[:, :, [0, 299]][np.broadcast_to(outside[:, None, :], (len(files), 2, 2))]).any()
    got32 = store.decode_window(files, starts, 300, dtype=torch.float32)
    assert got32.dtype == torch.float32 and np.array_equal(got32.cpu().numpy(), want.astype(np.float32))
    for f in range(len(f64)):
        for w, s in _singles(f64[f].shape[1]):
            one = store.decode_window([f], [s], w, dtype=torch.float64)[0].cpu().numpy()
            ref = _cut(f64[f], s, w)
            assert np.array_equal(one, ref) and np.array_equal(np.signbit(one), np.signbit(ref)), (f, w, s)
        w, s = 5000, -1
        one = store.decode_window([f], [s], w, dtype=torch.float32)[0].cpu().numpy()
        assert np.array_equal(one, _cut(f64[f], s, w).astype(np.float32))


def test_channel_map(kitchen):
    from mrcaudiocodec_amd import MrcError
    store, pcm = kitchen["store"], kitchen["pcm"]
    starts = [-200, 0, 2900, 5000]
    alone = store.decode_window([2] * 4, starts, 700)
    assert tuple(alone.shape) == (4, 1, 700)
    both = store.decode_window([2] * 4, starts, 700, channels=2)
    assert torch.equal(both[:, 0], alone[:, 0]) and torch.equal(both[:, 1], alone[:, 0])
    assert np.array_equal(alone.cpu().numpy(), _expect(pcm, [(2, s) for s in starts], 700, 1))
    out = torch.full((3, 1, 64), 12345, dtype=torch.int16, device=alone.device)
    with pytest.raises(MrcError, match=r"item 1: file 0 is stereo") as e:
        store.decode_window([2, 0, 5], [0, 0, 0], 64, channels=1, out=out)
    assert e.value.code == -1 and bool((out == 12345).all())


def test_result_does_not_depend_on_order_or_slabs(kitchen):
    store, h, items = kitchen["store"], kitchen["h"], kitchen["items"]
    files, starts = map(np.array, zip(*items))
    base = store.decode_window(files, starts, 300, dtype=torch.float64)
    assert store.stats()["slabs"] == 1
    perm = np.random.default_rng(3).permutation(len(items))
    back = torch.from_numpy(np.argsort(perm)).to(base.device)
    try:
        for slab, n_slabs in ((SLAB_DEFAULT, 1), (300, len(items)), (0, 1)):
            h.set_option(SLAB_OPTION, slab)
            assert h.get_option(SLAB_OPTION) == slab
            got = store.decode_window(files[perm], starts[perm], 300, dtype=torch.float64)
            assert store.stats()["slabs"] == n_slabs
            assert torch.equal(got[back], base) and torch.equal(torch.signbit(got[back]), torch.signbit(base))
        h.set_option(SLAB_OPTION, 700)                       # two items per slab, the last slab one
        got = store.decode_window(files, starts, 300, dtype=torch.float64)
        assert store.stats()["slabs"] == (len(items) + 1) // 2 and torch.equal(got, base)
    finally:
        h.set_option(SLAB_OPTION, SLAB_DEFAULT)


def _needed(ix, start, window):
    """the overlap rule, restated: blocks with block_start < start + window + L and block_start + a + b > start + L"""
    p = ix["block_start"]
    return int(np.count_nonzero((p < start + window + L) & (p + ix["block_a"] + ix["block_b"] > start + L)))


def test_only_the_needed_chunks_are_parsed(kitchen):
    store, index, files = kitchen["store"], kitchen["index"], kitchen["files"]
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(40):
        f = int(rng.integers(0, len(files)))
        n = int(store.n_samples[f])
        s, w = int(rng.integers(-1500, n + 1500)), int(rng.choice([1, 100, 1024, 3000]))
        store.decode_window([f], [s], w)
        want = _needed(index[f], s, w) * index[f]["n_channels"]
        st = store.stats()
        assert st["chunks_parsed"] == want, (f, s, w)
        assert (st["decode_launches"] == 0) == (want == 0)
        seen.add(want)
    assert 0 in seen and len(seen) > 4
    store.decode_window([0], [100], 300)                     # inside the first long region of a48_pac
    assert 0 < store.stats()["chunks_parsed"] <= 3 * 2
    store.decode_window([3], [10], 300)                      # the one-block stereo file
    st = store.stats()
    assert st["chunks_parsed"] == 2 and 0 < st["plan_bytes_uploaded"] < len(files[0])
    store.decode_window([0, 1], [0, 0], 14336)               # the whole files: every chunk
    assert store.stats()["chunks_parsed"] == 2 * 70


def test_damage_counts_only_inside_a_window(kitchen):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    h, good, pcm, ix = kitchen["h"], kitchen["store"], kitchen["pcm"], kitchen["index"][0]
    bad = bytearray(kitchen["files"][0])
    at = int(ix["chunk_offset"][20, 0]) + 4
    bad[at] = (bad[at] & 0x0F) | 0x40                        # table id 4
    p19, p20 = int(ix["block_start"][19]), int(ix["block_start"][20])
    with PacStore(h, [bytes(bad)]) as store:
        w = p19 - L                                          # [0, w) needs blocks that start before w + L = p19
        assert w > 2000 and _needed(ix, 0, w) == 19
        assert np.array_equal(store.decode_window([0], [0], w)[0].cpu().numpy(), _cut(pcm[0], 0, w))
        with pytest.raises(MrcError, match=r"file 0: chunk at byte %d: %s" % (at - 4, re.escape("table id not in {0..3, 15}"))) as e:
            store.decode_window([0], [p20 - L], 300)
        assert e.value.code == -1
    f, s = kitchen["items"][0]
    assert np.array_equal(good.decode_window([f], [s], 300)[0].cpu().numpy(), _cut(pcm[f], s, 300))


def test_refusals_and_lifetime(kitchen):
    from mrcaudiocodec_amd import Handle, MrcError, _lib
    from mrcaudiocodec_amd.store import PacStore
    h, store, files = kitchen["h"], kitchen["store"], kitchen["files"]
    dev = torch.device("cuda", 0)
    for args, kw, text in ((([6], [0], 10), {}, r"file\[0\] = 6 is outside"), (([0, -1], [0, 0], 10), {}, r"file\[1\] = -1"),
                           (([0], [0], -1), {}, "window"), (([2], [0], 10), dict(channels=3), "n_channels_out")):
        with pytest.raises(MrcError, match=text) as e:
            store.decode_window(*args, **kw)
        assert e.value.code == -1
    one = np.zeros(1, np.int64)
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    raw = lambda fmt, out: _lib.lib.mrc_pac_store_decode_window(store._s, 1, one.ctypes.data, one.ctypes.data, 8, 2, fmt, out, None)
    assert raw(3, buf.data_ptr()) == -1 and b"format" in _lib.lib.mrc_last_error(h._h)
    assert raw(-1, buf.data_ptr()) == -1
    assert raw(0, None) == -1 and b"out is NULL" in _lib.lib.mrc_last_error(h._h)
    assert raw(2, buf.data_ptr()) == 0
    with pytest.raises(MrcError, match="has sample_rate = 44100"):
        PacStore(h, [files[0], G.load("ref_pac.npz")["b44_pac"].tobytes()])
    assert tuple(store.decode_window([0, 2], [0, 5], 0).shape) == (2, 2, 0)
    assert tuple(store.decode_window([], [], 16).shape) == (0, 1, 16)
    for kw in (dict(dtype=torch.int16, out=torch.zeros((1, 2, 8), dtype=torch.float32, device=dev)),
               dict(out=torch.zeros((1, 2, 9), dtype=torch.int16, device=dev)),
               dict(out=torch.zeros((1, 2, 8), dtype=torch.int16)),
               dict(out=torch.zeros((1, 2, 16), dtype=torch.int16, device=dev)[:, :, ::2]),
               dict(dtype=torch.int32)):
        with pytest.raises(ValueError):
            store.decode_window([0], [0], 8, **kw)
    into = torch.zeros((1, 2, 8), dtype=torch.float32, device=dev)
    assert store.decode_window([0], [3000], 8, out=into) is into and bool(into.any())
    h2 = Handle()
    s2 = PacStore(h2, files[:1])
    s2.close()
    s2.close()                                               # twice: harmless
    s3 = PacStore(h2, files[:1])
    assert bool(s3.decode_window([0], [3000], 8).any())
    h2.close()                                               # the handle first
    with pytest.raises(MrcError, match="handle has been destroyed") as e:
        s3.decode_window([0], [3000], 8)
    assert e.value.code == -1
    with pytest.raises(MrcError):
        s3.stats()
    s3.close()


def test_cli_decodes_an_excerpt(kitchen, tmp_path):
    from mrcaudiocodec_amd import cli
    src, dst = str(tmp_path / "a48.pac"), str(tmp_path / "x.wav")
    with open(src, "wb") as f:
        f.write(kitchen["files"][0])
    cli.main(["-d", src, dst, "--start", "5000", "--samples", "3000"])
    assert open(dst, "rb").read() == cli.wav_bytes(kitchen["pcm"][0][:, 5000:8000], 48000)
    cli.main(["-d", src, dst, "--start", "14000"])           # to the end
    assert open(dst, "rb").read() == cli.wav_bytes(kitchen["pcm"][0][:, 14000:], 48000)
