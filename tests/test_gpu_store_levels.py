"""
GPU tests of the store's block energies (mrc_pac_store_block_energy, PacStore.block_energy / levels, cli --levels): every
energy against the NumPy restatement on the decoded lines (tests/levels_restatement.py) -- equal to the bit where the
restatement adds in the kernel's documented order, and within 2 (n_lines + 1) 2^-53 of a plain sum -- per channel and for the
mid, at D = 1, 2 and 4, on the files of the mix tests (settings B, C, D, K: stereo Huffman, stereo raw, mono, one-block mono,
one-block stereo; the default five-hop stereo file); entry offsets and blocks against pacfile.index; bit-identity from call to
call, under reversed and shuffled selections, alone and in company, and over slab sizes; the work counters; the energy of
whole files against the decoded windows, through LevelMap; damage; capacity; the refusals; the command line.
Everything oracle-side is computed once per module and never written to.
"""
import json
import re

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401
import levels_restatement as LR
import mix_restatement as MR
import settings_kit as SK

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDS = MR.KIT_SIDS + ("default",)
SLAB_OPTION, SLAB_DEFAULT = 7, 1 << 24
FN = "mrc_pac_store_block_energy"
MIXES = (None, "mid")


class _Kitchen:
    """one setting: its handle, files, store, index and restated energies (computed on first use)"""

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
        self.index = [ppac.index(b, self.cfg) for b in self.files]
        self.store = PacStore(self.h, self.files)
        self._ref = {}

    def ref(self, f, D, mix, order="kernel"):
        """(blocks [n][3], energy [n][columns], lines summed [n]) of file f, read-only"""
        if (f, D, mix, order) not in self._ref:
            _, blocks, e, n = LR.block_energies(self.files[f], self.S, self.blksw, D, mix == "mid", order)
            for a in (blocks, e, n):
                a.setflags(write=False)
            self._ref[(f, D, mix, order)] = (blocks, e, n)
        return self._ref[(f, D, mix, order)]

    def columns(self, f, mix):
        return 1 if mix == "mid" else self.nch[f]


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


def _raw(store, D, mix, files, cap, fill=77.0, blocks=True):
    """the entry point itself -> (status, entry_offset, entry_block, energy), the arrays filled with `fill` before the call"""
    from mrcaudiocodec_amd import _lib
    n = len(store) if files is None else len(files)
    sel = None if files is None else np.ascontiguousarray(files, dtype=np.int64)
    off = np.full(n + 1, -5, np.int64)
    blk = np.full((max(cap, 1), 3), int(fill), np.int64)
    e = np.full(max(cap, 1), fill, np.float64)
    rc = _lib.lib.mrc_pac_store_block_energy(store._s, D, mix, n, None if sel is None else sel.ctypes.data, off.ctypes.data, cap,
                                             blk.ctypes.data if blocks else None, e.ctypes.data, None)
    return rc, off, blk, e


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------ 1: the energies against the restatement
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", MR.DIVISORS)
def test_energies_equal_the_restatement(kitchen, D, mix):
    k = kitchen
    off, blocks, energy = k.store.block_energy(D, mix)
    assert off[0] == 0 and energy.dtype == np.float64 and blocks.shape == (off[-1], 3)
    worst = 0.0
    for f in range(len(k.files)):
        want_blocks, want, n_lines = k.ref(f, D, mix)
        cols = k.columns(f, mix)
        got = energy[off[f]:off[f + 1]].reshape(-1, cols)
        assert got.shape == want.shape and want.any()
        assert np.array_equal(blocks[off[f]:off[f + 1]:cols], want_blocks)
        assert np.array_equal(got, want), (k.sid, f, D, mix, np.abs(got - want).max())      # the kernel's order: the same bits
        # ... and the bound that needs no order: both sides add at most n non-negative terms and multiply once
        plain = k.ref(f, D, mix, "plain")[1]
        bound = 2.0 * (n_lines[:, None] + 1) * 2.0 ** -53
        rel = np.abs(got - plain) / np.where(plain > 0, plain, 1.0)
        worst = max(worst, float((rel / bound).max()))
        assert np.all(rel <= bound), (k.sid, f, D, mix)
    print("%s D = %d mix = %s: equal to the kernel-order restatement; largest difference from a plain sum %.3g of the bound"
          % (k.sid, D, mix, worst))


# ------------------------------------------------------------------ 2: entries
@pytest.mark.parametrize("mix", MIXES)
def test_entry_offsets_and_blocks_follow_the_index(kitchen, mix):
    k = kitchen
    sel = [len(k.files) - 1, 0, 0, 2 % len(k.files)]
    for files in (None, sel):
        off, blocks, energy = k.store.block_energy(2, mix, files)
        chosen = range(len(k.files)) if files is None else files
        assert len(off) == len(chosen) + 1
        at = 0
        for j, f in enumerate(chosen):
            ix, cols = k.index[f], k.columns(f, mix)
            assert off[j] == at
            at += int(ix["n_blocks"]) * cols
            b = blocks[off[j]:at]
            assert np.array_equal(b[:, 0], np.repeat(ix["block_start"], cols))
            assert np.array_equal(b[:, 1], np.repeat(ix["block_a"], cols)) and np.array_equal(b[:, 2], np.repeat(ix["block_b"], cols))
        assert off[-1] == at == len(energy)
    rc, off, blk, e = _raw(k.store, 1, 3, None, 1 << 12, blocks=False)                      # entry_block may be NULL
    assert rc == 0 and _same(e[:off[-1]], k.store.block_energy(1, None)[2])


# ------------------------------------------------------------------ 3: bit-identity
def _planned_slabs(k, files, D, slab):
    """the slab rule: runs of whole blocks, in entry order, whose b / D sum to at most `slab` (one block at least)"""
    n, samples = 0, None
    for f in files:
        for b in k.index[f]["block_b"]:
            if samples is None or (slab and samples + int(b) // D > slab):
                n, samples = n + 1, 0
            samples += int(b) // D
    return n


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("D", [1, 2])
def test_energies_do_not_depend_on_call_order_company_or_slabs(kitchen, D, mix):
    k = kitchen
    nf = len(k.files)
    off, _, base = k.store.block_energy(D, mix)
    st = k.store.stats()
    assert st["slabs"] == 1 and st["chunks_parsed"] == sum(int(ix["n_blocks"]) * int(ix["n_channels"]) for ix in k.index)
    assert 1 <= st["decode_launches"] <= 8 and st["plan_bytes_uploaded"] > 0 and st["ms"]["window_out"] == 0.0
    per_file = [base[off[f]:off[f + 1]] for f in range(nf)]
    assert _same(k.store.block_energy(D, mix)[2], base)                                     # call to call
    orders = [list(range(nf))[::-1], list(np.random.default_rng(3).permutation(nf)), [0, 0] + list(range(nf))]
    for sel in orders:
        o, _, e = k.store.block_energy(D, mix, sel)
        for j, f in enumerate(sel):
            assert _same(e[o[j]:o[j + 1]], per_file[f]), (k.sid, D, mix, sel, f)
    for f in range(nf):                                                                      # alone
        o, _, e = k.store.block_energy(D, mix, [f])
        assert _same(e, per_file[f])
        assert k.store.stats()["chunks_parsed"] == int(k.index[f]["n_blocks"]) * int(k.index[f]["n_channels"])
    try:
        for slab in (k.S, k.L + k.S, 2 * k.L, 0, SLAB_DEFAULT):
            k.h.set_option(SLAB_OPTION, slab)
            assert _same(k.store.block_energy(D, mix)[2], base), (k.sid, D, mix, slab)
            assert k.store.stats()["slabs"] == _planned_slabs(k, range(nf), D, slab), (k.sid, D, slab)
        if D == 1:                                                   # n_short: one block per slab
            k.h.set_option(SLAB_OPTION, k.S)
            k.store.block_energy(D, mix)
            assert k.store.stats()["slabs"] == sum(int(ix["n_blocks"]) for ix in k.index)
    finally:
        k.h.set_option(SLAB_OPTION, SLAB_DEFAULT)


# ------------------------------------------------------------------ 4: whole files against their decoded windows
@pytest.mark.parametrize("nch", [2, 1])
def test_level_map_of_a_whole_file_is_the_energy_of_its_decoded_window(nch):
    """first and last hop digital silence: block 0 decodes to zeros, so nothing lies in the MDCT's delay, which decode_window
    drops, and the window [0, n_samples) holds every tile but half of block 0's.  Parseval to rounding: 1e-12 relative."""
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen("default")
    buf = LR.silent_ends_file(nch, 21 + nch)
    with PacStore(k.h, [buf, k.files[0]]) as store:
        n = int(store.n_samples[0])
        assert n == 7 * k.L and int(store.n_channels[0]) == nch
        for D, mix in ((1, None), (2, None), (1, "mid"), (2, "mid"), (4, None)):
            m = store.levels(D, mix)
            assert store.levels(D, mix) is m and m.D == D and len(m) == 2               # cached per (D, mix)
            x = store.decode_window([0], [0], n // D, dtype=torch.float64, rate_divisor=D, mix=mix)[0].cpu().numpy()
            want = (x ** 2).sum(-1)
            got = m.window_energy([0], [0], n // D)[0, :len(want)]
            assert want.shape == ((1,) if mix == "mid" else (nch,)) and np.all(want > 1.0)
            rel = np.abs(got - want) / want
            print("%d channel(s) D = %d mix = %s: relative difference %.3g" % (nch, D, mix, rel.max()))
            assert np.all(rel <= 1e-12), (nch, D, mix, rel)
            assert np.all(np.abs(m.total_energy(0) - want) <= 1e-12 * want)
            assert m.tiles(0)[0] == -k.L / (2.0 * D) and m.n_samples[0] == n // D
        some = store.levels(2, None, files=[1])
        assert some is not store.levels(2, None) and len(some) == 1
        assert np.array_equal(some.energy[0], store.levels(2, None).energy[1])


# ------------------------------------------------------------------ 5: damage
@pytest.mark.parametrize("D", [1, 4])
def test_damage_names_file_and_byte_as_a_window_over_the_block_does(kitchen, D):
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
    with PacStore(k.h, [k.files[0], bytes(bad), k.files[2 % len(k.files)]]) as store:
        with pytest.raises(MrcError, match=r"file 1: chunk at byte %d: %s" % (at - 4, reason)) as w:
            store.decode_window([1], [(pj - L) // D], 3, channels=2, rate_divisor=D)
        for mix in MIXES:
            with pytest.raises(MrcError, match=r"%s: file 1: chunk at byte %d: %s" % (FN, at - 4, reason)) as e:
                store.block_energy(D, mix)
            assert e.value.code == -1 and _words(e.value) == _words(w.value)                # the window's words
            with pytest.raises(MrcError, match=r"%s: file 1: chunk at byte %d" % (FN, at - 4)):
                store.block_energy(D, mix, [2, 1])                   # the file's index in the store, not in the selection
            # the store still serves the other files
            o, _, e2 = store.block_energy(D, mix, [0, 2])
            assert _same(e2[o[0]:o[1]], k.store.block_energy(D, mix, [0])[2])
            assert _same(e2[o[1]:o[2]], k.store.block_energy(D, mix, [2 % len(k.files)])[2])


def _words(err):
    """an error's text behind the name of the entry point"""
    return re.sub(r"^.*?mrc_pac_store_\w+: ", "", str(err))


# ------------------------------------------------------------------ 6: capacity and refusals
def test_entry_cap_too_small_fills_the_offsets_and_nothing_else(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    want = k.store.block_energy(1, None)[0]
    for cap in (0, int(want[-1]) - 1):
        rc, off, blk, e = _raw(k.store, 1, _lib.MRC_MIX_EACH, None, cap)
        assert rc == _lib.MRC_ERR_NOMEM and np.array_equal(off, want)
        assert bool((e == 77.0).all()) and bool((blk == 77).all())
        assert "entry_cap" in _lib.lib.mrc_last_error(k.h._h).decode()
        st = k.store.stats()
        assert st["chunks_parsed"] == 0 and st["slabs"] == 0 and st["decode_launches"] == 0
    rc, off, blk, e = _raw(k.store, 1, _lib.MRC_MIX_EACH, None, int(want[-1]))
    assert rc == 0 and not bool((e[:want[-1]] == 77.0).all())


def test_refusals(kitchen):
    from mrcaudiocodec_amd import _lib
    k = kitchen
    cap = 1 << 12

    def refused(D, mix, files, *words):
        rc, off, blk, e = _raw(k.store, D, mix, files, cap)
        text = _lib.lib.mrc_last_error(k.h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and bool((e == 77.0).all()) and bool((blk == 77).all()), (D, mix, files)
        assert FN in text and all(w in text for w in words), text
        assert k.store.stats()["chunks_parsed"] == 0

    for mix in (1, 2, 4, -1):
        refused(1, mix, None, "mix %d" % mix)
    for D in (0, 3, 8, -2):
        refused(D, _lib.MRC_MIX_MID, None, "rate_divisor %d" % D)
    nf = len(k.files)
    refused(1, _lib.MRC_MIX_EACH, [0, nf], "file[1] = %d" % nf, "outside the store's %d files" % nf)
    refused(1, _lib.MRC_MIX_EACH, [-1], "file[0] = -1")
    # Python side: before any library call
    with pytest.raises(ValueError, match="column of mix=None"):
        k.store.levels(mix="left")
    with pytest.raises(ValueError, match="rate_divisor"):
        k.store.levels(rate_divisor=3)
    with pytest.raises(ValueError, match="indices into the store"):
        k.store.levels(files=[nf])
    # no selection: offsets alone
    rc, off, blk, e = _raw(k.store, 1, _lib.MRC_MIX_EACH, [], 0)
    assert rc == 0 and off.tolist() == [0]


def test_quarter_rate_is_refused_where_a_shape_has_no_quarter():
    """(324, 108): D = 4 is refused with the text of mrc_pac_store_decode_window_reduced, D = 2 runs"""
    from mrcaudiocodec_amd import Handle, MrcError
    from mrcaudiocodec_amd.store import PacStore
    L, S = 324, 108
    h = Handle(device_id=0, n_mdct_lines=L, n_short=S)
    try:
        buf = MR.default_stereo_file(9, L, S)
        with PacStore(h, [buf]) as store:
            with pytest.raises(MrcError, match=r"rate_divisor 4: block shape \(%d,%d\)" % (L, L)) as w:
                store.decode_window([0], [0], 16, dtype=torch.float64, rate_divisor=4)
            for mix in MIXES:
                with pytest.raises(MrcError, match=r"%s: rate_divisor 4: block shape \(%d,%d\)" % (FN, L, L)) as e:
                    store.block_energy(4, mix)
                assert e.value.code == -1 and _words(e.value) == _words(w.value)
                assert store.stats()["chunks_parsed"] == 0
                _, blocks, want, _ = LR.block_energies(buf, S, (1, 1), 2, mix == "mid")
                assert np.array_equal(store.block_energy(2, mix)[2].reshape(want.shape), want)
    finally:
        h.close()


# ------------------------------------------------------------------ 7: the command line
def test_cli_prints_the_levels_of_each_file(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd.store import PacStore
    k = _kitchen("default")
    bufs = [LR.silent_ends_file(2, 23), LR.silent_ends_file(1, 22)]
    paths = [str(tmp_path / "s.pac"), str(tmp_path / "m.pac")]
    for p, b in zip(paths, bufs):
        with open(p, "wb") as f:
            f.write(b)
    for argv, D, mix, window in (([], 1, None, 48000), (["--levels-window", "2048"], 1, None, 2048),
                                 (["--rate-divisor", "2", "--mix", "mid", "--levels-window", "1000"], 2, "mid", 1000)):
        capsys.readouterr()
        cli.main(["--levels"] + paths + argv)
        lines = [json.loads(l) for l in capsys.readouterr().out.strip().split("\n")]
        assert len(lines) == 2
        with PacStore(k.h, bufs) as store:
            m = store.levels(D, mix)
            for f, r in enumerate(lines):
                nch = 1 if mix == "mid" else int(store.n_channels[f])
                n = int(store.n_samples[f]) // D
                assert (r["file"], r["channels"], r["samples"], r["window"]) == (paths[f], nch, n, window)
                assert r["rms_db"] == [float(v) for v in m.window_rms_db([f], [0], n)[0, :nch]]
                starts, db = m.grid_levels(f, window)
                if window > n:
                    assert starts.size == 0 and r["loudest_db"] is None and r["quietest_start"] is None
                else:
                    assert starts[1] - starts[0] == k.S // D
                    assert (r["loudest_db"], r["loudest_start"]) == (float(db.max()), int(starts[np.argmax(db)]))
                    assert (r["quietest_db"], r["quietest_start"]) == (float(db.min()), int(starts[np.argmin(db)]))
                    assert r["loudest_db"] > r["quietest_db"] and -30 < r["loudest_db"] < 0
