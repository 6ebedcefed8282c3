"""
GPU tests of the constant-quality VBR kernels on crafted blocks (tests/vbr_cases.py) through their stage entries:

  mrc_dev_vbr_alloc    vbr_alloc_kernel (vbr_walk<false>)
  mrc_dev_vbr_profile  vbr_profile_kernel (vbr_walk<true>): the record of the walk without a ceiling
  mrc_dev_vbr_pick     vbr_pick_kernel: the allocation for one ceiling per block from such a record

Two yardsticks.  The NumPy restatement (tests/vbr_restatement.py) for everything that is bit-defined -- the states a walk
passes, the streams an M/S band raises, and at the cases' own ceilings (no edge candidate: tests/test_vbr_cases_cpu.py) every
integer; its ratios differ from the device's by the two pow() of the masks only (1e-9 relative, the bar of
chain_kit.check_nmr_against_restatement).  And the rule itself (`rule`, below) applied to the DEVICE's record, which needs no
pow and therefore holds at any ceiling, a recorded ratio itself and its two neighbours included.
"""
import math

import numpy as np
import pytest

import vbr_cases as vc
from test_gpu_stages import _dev, _full, _ptr

pytestmark = pytest.mark.gpu

CANARY = -31000
R_CANARY = -7.0                                              # no ratio is negative
COUNTS = [1, 63, 64, 65]
EXTRA_CEILINGS = [3.7e-5, 0.02, 1.0, 47.0, 2.5e4]            # besides the cases' own
N_TIES = 12
_BASE = {}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def handles():
    from mrcaudiocodec_amd import Handle
    hs = {s: Handle(device_id=0, **kw) for s, kw in vc.SETTINGS.items()}
    yield hs
    for hd in hs.values():
        hd.close()


class Dev:
    """the device planes of the blocks `idx` of a configuration and the three entries on them; every output plane is
    followed by a canary"""

    def __init__(self, torch, hd, cfg, idx):
        from mrcaudiocodec_amd import Handle
        cs, lay = vc.cases(cfg), vc.layout(cfg)
        self.torch, self.h, self.cfg, self.lay, self.joint = torch, hd, cfg, lay, cfg[2]
        self.idx, self.n = np.asarray(idx), len(idx)
        self.W = Handle.vbr_record_width(self.joint)
        i32 = torch.int32
        self.lines = _dev(torch, cs["lines"][self.idx])
        self.osc = _dev(torch, cs["overall_scale"][self.idx], i32)
        self.ms = _dev(torch, cs["ms_switch"][self.idx], i32) if self.joint else None
        self.X = _dev(torch, cs["X"][:, self.idx])
        self.T = _dev(torch, cs["T"][:, self.idx])
        self.rec = None

    def _out(self):
        t, lay, n = self.torch, self.lay, self.n
        nb, ns, half = lay["nb"], lay["ns"], lay["half"]
        self.size = dict(ba=n * ns * nb, sf=n * ns * nb, mant=n * ns * half, stat=n * ns * 2, capped=n * ns)
        dt = dict(ba=t.int32, sf=t.int32, mant=t.int16, stat=t.float64, capped=t.int32)
        return {k: _full(t, v + 64, dt[k], math.nan if k == "stat" else CANARY) for k, v in self.size.items()}

    def _read(self, o, what):
        lay, n = self.lay, self.n
        nb, ns, half = lay["nb"], lay["ns"], lay["half"]
        self.torch.cuda.synchronize()
        out = {}
        for k, v in o.items():
            x = v.cpu().numpy()
            tail = x[self.size[k]:]
            assert np.isnan(tail).all() if k == "stat" else (tail == CANARY).all(), "%s: %s written beyond its end" % (what, k)
            x = x[:self.size[k]]
            out[k] = x.view(np.uint16).astype(np.int64) if k == "mant" else x.astype(np.int64) if k != "stat" else x
        cap = out["capped"].reshape(n, ns)
        assert (cap[:, 1:] == 0).all(), what + ": capped bands counted at a block's second entry"
        return dict(bit_alloc=out["ba"].reshape(n, ns, nb), scale_factor=out["sf"].reshape(n, ns, nb),
                    mantissa=out["mant"].reshape(n, ns, half), stat=out["stat"].reshape(n, ns, 2), capped=cap[:, 0])

    def alloc(self, c, what="alloc"):
        o = self._out()
        a, b = self.cfg[:2]
        self.h.dev_vbr_alloc(a, b, self.n, self.joint, c, _ptr(self.lines), _ptr(self.osc), _ptr(self.ms), _ptr(self.X),
                             _ptr(self.T), _ptr(o["ba"]), _ptr(o["sf"]), _ptr(o["mant"]), _ptr(o["stat"]), _ptr(o["capped"]))
        return self._read(o, what)

    def profile(self, what="profile"):
        """-> ratios [n][nb][W], picks [n][nb]; the device copies are kept for pick()"""
        t, n, nb, W = self.torch, self.n, self.lay["nb"], self.W
        rat = _full(t, n * nb * W + 64, t.float64, R_CANARY)
        picks = _full(t, n * nb + 64, t.int32, CANARY)
        a, b = self.cfg[:2]
        self.h.dev_vbr_profile(a, b, n, self.joint, _ptr(self.lines), _ptr(self.osc), _ptr(self.ms), _ptr(self.X), _ptr(self.T),
                               _ptr(rat), _ptr(picks) if self.joint else None)
        t.cuda.synchronize()
        r, p = rat.cpu().numpy(), picks.cpu().numpy()
        assert (r[n * nb * W:] == R_CANARY).all() and (p[n * nb if self.joint else 0:] == CANARY).all(), what + ": written beyond its end"
        r = r[:n * nb * W].reshape(n, nb, W)
        assert (np.isnan(r) | (r >= 0)).all(), what + ": the record was not filled with NaN first"
        self.rec = (rat, picks)
        p = p[:n * nb].view(np.uint32).astype(np.int64).reshape(n, nb) if self.joint else np.zeros((n, nb), np.int64)
        return r, p

    def pick(self, ceilings, what="pick"):
        if self.rec is None:
            self.profile()
        o = self._out()
        a, b = self.cfg[:2]
        c = _dev(self.torch, np.array(np.broadcast_to(np.asarray(ceilings, np.float64), (self.n,))))
        self.h.dev_vbr_pick(a, b, self.n, self.joint, _ptr(c), _ptr(self.lines), _ptr(self.osc), _ptr(self.ms), _ptr(self.rec[0]),
                            _ptr(self.rec[1]) if self.joint else None, _ptr(o["ba"]), _ptr(o["sf"]), _ptr(o["mant"]),
                            _ptr(o["stat"]), _ptr(o["capped"]))
        return self._read(o, what)


def _base(torch, handles, cfg):
    """all blocks of the configuration on the device, with the device's record of them"""
    if cfg not in _BASE:
        d = Dev(torch, handles[cfg[3]], cfg, np.arange(vc.N_BLOCKS))
        rat, picks = d.profile(vc.config_id(cfg) + " profile")
        _BASE[cfg] = (d, rat, picks)
    return _BASE[cfg]


def _same(got, want, what, keys=("bit_alloc", "scale_factor", "mantissa", "capped", "stat")):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
        assert bad.size == 0, "%s %s: %d mismatching entries, first at %s (got %s, want %s)" % (
            what, k, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


INTS = ("bit_alloc", "scale_factor", "mantissa", "capped")


# ------------------------------------------------------------------ the rule, on a record
def rule(cfg, rat, picks, ms, ceilings, b):
    """DESIGN.md section 12 on a record: per band the first recorded state with r <= c (both ratios in an M/S band, which
    follows the recorded picks), else the last one, capped -- per stream in an L/R band, once in an M/S band.  -> bit_alloc
    [n][ns][nb], capped [n], stat [n][ns][2] (fmax from 0, the running sum in band order, b * (sum / nb)), state [n][ns][nb]
    (the index of the stopping state; an M/S band: its step)."""
    lay = vc.layout(cfg)
    nb, ns, mb, joint = lay["nb"], lay["ns"], lay["max_bits"], cfg[2]
    cand = [0] + list(range(2, mb + 1))
    n, W = rat.shape[0], rat.shape[2]
    bits = np.zeros((n, ns, nb), np.int64)
    state = np.zeros((n, ns, nb), np.int64)
    r = np.full((n, ns, nb), np.nan)
    cap = np.zeros(n, np.int64)
    ceilings = np.broadcast_to(np.asarray(ceilings, np.float64), (n,))
    for i in range(n):
        c = ceilings[i]
        for j in range(nb):
            if lay["n_lines"][j] == 0:
                continue                                     # no bits; its ratios 0 / 0
            if joint and ms[i, j] == 1:
                nn, step = [0, 0], 0
                while True:
                    r0, r1 = rat[i, j, 2 * step], rat[i, j, 2 * step + 1]
                    if r0 <= c and r1 <= c:
                        break
                    if nn[0] >= mb and nn[1] >= mb:
                        cap[i] += 1
                        break
                    s = (int(picks[i, j]) >> step) & 1
                    nn[s] = nn[s] + 1 if nn[s] else 2
                    step += 1
                bits[i, :, j], r[i, :, j], state[i, :, j] = nn, (r0, r1), step
                continue
            for s in range(ns):
                off = s * (W // 2) if joint else 0
                for k, nbits in enumerate(cand):
                    if rat[i, j, off + k] <= c:
                        break
                else:
                    cap[i] += 1
                bits[i, s, j], r[i, s, j], state[i, s, j] = nbits, rat[i, j, off + k], k
    stat = np.empty((n, ns, 2))
    stat[:, :, 0] = np.fmax.reduce(np.concatenate([np.zeros((n, ns, 1)), r], axis=2), axis=2)
    stat[:, :, 1] = float(b) * (np.cumsum(r, axis=2)[:, :, -1] / float(nb))
    return dict(bit_alloc=bits, capped=cap, stat=stat, state=state)


# ------------------------------------------------------------------ 1. the record against NumPy
@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_record_against_restatement(torch, handles, cfg):
    d, rat, picks = _base(torch, handles, cfg)
    want, want_picks = vc.record(cfg, d.W)
    what = vc.config_id(cfg)
    bad = np.argwhere(np.isnan(rat) != np.isnan(want))
    assert bad.size == 0, "%s: the states written differ in %d entries, first at %s" % (what, len(bad), bad[0])
    bad = np.argwhere(picks != want_picks)
    assert bad.size == 0, "%s: the streams raised differ in %d bands, first at %s" % (what, len(bad), bad[0])
    zero = want == 0.0                                       # an infinite mask (or no noise at all): exactly 0
    assert (rat[zero] == 0.0).all(), what + ": a ratio under an infinite mask, or of no noise, is not exactly 0"
    fin = ~np.isnan(want) & ~zero
    assert np.isfinite(rat[fin]).all() and np.isfinite(want[fin]).all()
    dev = np.abs(rat[fin] - want[fin]) / np.abs(want[fin])
    print("%s: %d recorded ratios, largest relative deviation from the restatement %.3g" % (what, fin.sum(), dev.max()))
    assert dev.max() <= 1e-9, what


# ------------------------------------------------------------------ 2. alloc against NumPy at the cases' ceilings
@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_alloc_against_restatement(torch, handles, cfg):
    cs, ref = vc.cases(cfg), vc.reference(cfg)
    assert ref["edges"] == 0
    for k, c in enumerate(ref["ceilings"]):
        idx = np.flatnonzero(cs["ceiling"] == k)
        got = Dev(torch, handles[cfg[3]], cfg, idx).alloc(c)
        _same(got, {key: ref[key][idx] for key in INTS}, "%s c=%g vs restatement" % (vc.config_id(cfg), c), INTS)
        if math.isinf(c):
            assert not got["bit_alloc"].any() and not got["mantissa"].any() and not got["capped"].any()
    # one pick launch with every block at its own ceiling: the same integers from the record
    d, rat, picks = _base(torch, handles, cfg)
    got = d.pick(ref["ceilings"][cs["ceiling"]])
    _same(got, ref, vc.config_id(cfg) + " pick, a ceiling per block, vs restatement", INTS)


# ------------------------------------------------------------------ 3. alloc == the rule on the device's record == pick
@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_alloc_and_pick_follow_the_rule_on_the_device_record(torch, handles, cfg):
    d, rat, picks = _base(torch, handles, cfg)
    cs, ref = vc.cases(cfg), vc.reference(cfg)
    for c in list(ref["ceilings"]) + EXTRA_CEILINGS:
        what = "%s c=%g" % (vc.config_id(cfg), c)
        want = rule(cfg, rat, picks, cs["ms_switch"], c, cfg[1])
        got = d.alloc(c)
        _same(got, want, what + " alloc vs the rule on the record", ("bit_alloc", "capped", "stat"))
        _same(d.pick(c), got, what + " pick vs alloc")
    c = np.random.default_rng(5).permutation(np.resize(list(ref["ceilings"]) + EXTRA_CEILINGS, vc.N_BLOCKS))
    _same(d.pick(c), rule(cfg, rat, picks, cs["ms_switch"], c, cfg[1]), vc.config_id(cfg) + " pick, ceilings mixed",
          ("bit_alloc", "capped", "stat"))


# ------------------------------------------------------------------ 4. ties: a ceiling that IS a recorded ratio
def _tie_sample(cfg, rat, picks, ms):
    """(block, band, stream, state index, r): recorded states whose deciding ratio (an M/S step: the larger of its two) is
    positive, finite and below that of every earlier state of the band -- so that c = r stops the band exactly there"""
    lay = vc.layout(cfg)
    nb, ns, joint, W = lay["nb"], lay["ns"], cfg[2], rat.shape[2]
    rng = np.random.default_rng(vc._seed(cfg, 9))
    out, tries = [], 0
    while len(out) < N_TIES and tries < 5000:
        tries += 1
        i, j = int(rng.integers(0, rat.shape[0])), int(rng.integers(0, nb))
        if lay["n_lines"][j] == 0:
            continue
        is_ms = bool(joint and ms[i, j] == 1)
        if joint and is_ms != (len(out) % 2 == 1) and tries < 2500:
            continue                                         # (M/S steps and L/R states in turn)
        if is_ms:
            seq, s = np.fmax(rat[i, j, 0::2], rat[i, j, 1::2]), 0
        else:
            s = int(rng.integers(0, ns))
            seq = rat[i, j, s * (W // 2):(s + 1) * (W // 2)] if joint else rat[i, j]
        seq = seq[~np.isnan(seq)]
        k = int(rng.integers(0, len(seq)))
        if not (np.isfinite(seq[k]) and seq[k] > 0.0 and (seq[:k] > seq[k]).all()):
            continue
        out.append((i, j, s, k, float(seq[k])))
    assert len(out) == N_TIES, vc.config_id(cfg)
    return out


@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_ties_with_a_recorded_ratio(torch, handles, cfg):
    d, rat, picks = _base(torch, handles, cfg)
    cs = vc.cases(cfg)
    ms = cs["ms_switch"]
    sample = _tie_sample(cfg, rat, picks, ms)
    blocks = np.repeat([t[0] for t in sample], 3)
    ceil = np.concatenate([[r, np.nextafter(r, -math.inf), np.nextafter(r, math.inf)] for (_, _, _, _, r) in sample])
    sub = Dev(torch, handles[cfg[3]], cfg, blocks)
    sub.profile()
    want = rule(cfg, rat[blocks], picks[blocks], ms[blocks] if cfg[2] else None, ceil, cfg[1])
    for q, (i, j, s, k, r) in enumerate(sample):             # the rule itself: at c == r there, one ulp below further on
        assert want["state"][3 * q, s, j] == k and want["state"][3 * q + 2, s, j] == k, (i, j, s, k)
        assert want["state"][3 * q + 1, s, j] > k or want["capped"][3 * q + 1] > want["capped"][3 * q], (i, j, s, k)
    by_pick = sub.pick(ceil)
    _same(by_pick, want, vc.config_id(cfg) + " ties through the pick entry", ("bit_alloc", "capped", "stat"))
    for q, (i, j, s, k, r) in enumerate(sample):
        one = Dev(torch, handles[cfg[3]], cfg, [i])
        for v in range(3):
            got = one.alloc(ceil[3 * q + v])
            row = {key: by_pick[key][3 * q + v:3 * q + v + 1] for key in by_pick}
            _same(got, row, "%s block %d band %d stream %d state %d, c = r %+d ulp: alloc vs pick" % (
                vc.config_id(cfg), i, j, s, k, (0, -1, 1)[v]))


# ------------------------------------------------------------------ 5. launch independence
@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_launch_independence(torch, handles, cfg):
    d, rat, picks = _base(torch, handles, cfg)
    c = float(vc.reference(cfg)["ceilings"][3])
    what = vc.config_id(cfg)
    base = d.alloc(c)
    _same(d.alloc(c), base, what + " alloc, repeated")
    base_pick = d.pick(c)
    _same(d.pick(c), base_pick, what + " pick, repeated")
    rat2, picks2 = d.profile()
    _same(dict(r=rat2, p=picks2), dict(r=rat, p=picks), what + " profile, repeated", ("r", "p"))
    order = np.random.default_rng(11).permutation(vc.N_BLOCKS)
    for idx in [order] + [order[:n] for n in COUNTS] + [np.arange(n) for n in COUNTS]:
        sub = Dev(torch, handles[cfg[3]], cfg, idx)
        w = "%s %d blocks" % (what, len(idx))
        r, p = sub.profile()
        _same(dict(r=r, p=p), dict(r=rat[idx], p=picks[idx]), w + " profile", ("r", "p"))
        _same(sub.alloc(c), {k: base[k][idx] for k in base}, w + " alloc")
        _same(sub.pick(c), {k: base_pick[k][idx] for k in base}, w + " pick")


# ------------------------------------------------------------------ 6. refusals
def test_refusals(torch, handles):
    from mrcaudiocodec_amd import Handle, MrcError
    for cfg in [(128, 128, False, "default"), (128, 128, True, "default")]:
        a, b, joint, _ = cfg
        hd = handles["default"]
        d = Dev(torch, hd, cfg, np.arange(4))
        rat, picks = d.profile()
        base = d.alloc(1.0)
        o = d._out()
        ceil = _dev(torch, np.ones(4))
        rec_r = _full(torch, 4 * d.lay["nb"] * d.W, torch.float64, R_CANARY)
        rec_p = _full(torch, 4 * d.lay["nb"], torch.int32, CANARY)
        common = dict(a=a, b=b, n=4, lines=_ptr(d.lines), osc=_ptr(d.osc), ms=_ptr(d.ms))
        outs = dict(ba=_ptr(o["ba"]), sf=_ptr(o["sf"]), mant=_ptr(o["mant"]), stat=_ptr(o["stat"]), capped=_ptr(o["capped"]))

        def alloc(**kw):
            k = dict(common, X=_ptr(d.X), T=_ptr(d.T), **outs)
            k.update(kw)
            hd.dev_vbr_alloc(k["a"], k["b"], k["n"], joint, 1.0, k["lines"], k["osc"], k["ms"], k["X"], k["T"], k["ba"], k["sf"],
                             k["mant"], k["stat"], k["capped"])

        def profile(**kw):
            k = dict(common, X=_ptr(d.X), T=_ptr(d.T), rat=_ptr(rec_r), picks=_ptr(rec_p) if joint else None)
            k.update(kw)
            hd.dev_vbr_profile(k["a"], k["b"], k["n"], joint, k["lines"], k["osc"], k["ms"], k["X"], k["T"], k["rat"], k["picks"])

        def pick(**kw):
            k = dict(common, ceil=_ptr(ceil), rat=_ptr(d.rec[0]), picks=_ptr(d.rec[1]) if joint else None, **outs)
            k.update(kw)
            hd.dev_vbr_pick(k["a"], k["b"], k["n"], joint, k["ceil"], k["lines"], k["osc"], k["ms"], k["rat"], k["picks"], k["ba"],
                            k["sf"], k["mant"], k["stat"], k["capped"])

        shape = [dict(n=-1), dict(a=1152, b=1152), dict(a=1536, b=1536), dict(a=162, b=162)]   # the handle / the chained back end refuses them
        nulls = {alloc: ["lines", "osc", "X", "T", "ba", "sf", "mant", "stat", "capped"], profile: ["lines", "osc", "X", "T", "rat"],
                 pick: ["ceil", "lines", "osc", "rat", "ba", "sf", "mant", "stat", "capped"]}
        for call, names in nulls.items():
            call(n=0)                                        # no blocks: nothing to do, and OK
            bad = shape + [{k: None} for k in names] + ([dict(ms=None)] if joint else [])
            if joint and call is not alloc:
                bad.append(dict(picks=None))
            for kw in bad:
                with pytest.raises(MrcError) as e:
                    call(**kw)
                assert e.value.code == -1 and not str(e.value).endswith("?"), (call.__name__, kw)   # MRC_ERR_INVALID, with a message
                arg = next(iter(kw))
                if kw[arg] is None:
                    assert "null" in str(e.value), (call.__name__, kw, str(e.value))
            torch.cuda.synchronize()
            for k, v in o.items():                           # nothing was written by any of them
                x = v.cpu().numpy()
                assert np.isnan(x).all() if k == "stat" else (x == CANARY).all(), (call.__name__, k)
            assert (rec_r.cpu().numpy() == R_CANARY).all() and (rec_p.cpu().numpy() == CANARY).all(), call.__name__
            _same(d.alloc(1.0), base, "the handle after the refusals of " + call.__name__)   # ... and the handle still works
    # The launches refuse a walk of more than 60 KB of LDS: a joint block of more than 1182 lines per channel.  No handle
    # hands out such a shape (1123 lines at the most; (1536, 1536) above is refused with the shape), so the entries' own
    # check cannot be reached from here.  The largest joint blocks there are do fit: the long block (52 KB, every
    # configuration above) and the joint transition block of 1536 coded lines of settings-matrix row D (39 KB):
    hd = Handle(device_id=0, n_mdct_lines=1024, n_short=512)
    try:
        nb, half = len(hd.bands(1024, 512)), 768
        z = _full(torch, 4 * half, torch.float64, 0.0)
        zi = _full(torch, 4 * half, torch.int32, 0)
        ba, sf, mant = (_full(torch, 2 * half + 64, t, CANARY) for t in (torch.int32, torch.int32, torch.int16))
        stat = _full(torch, 4 + 64, torch.float64, math.nan)
        capped = _full(torch, 2 + 64, torch.int32, CANARY)
        hd.dev_vbr_alloc(1024, 512, 1, True, 0.0, _ptr(z), _ptr(zi), _ptr(zi), _ptr(z), _ptr(z), _ptr(ba), _ptr(sf), _ptr(mant),
                         _ptr(stat), _ptr(capped))
        torch.cuda.synchronize()
        ba, mant, stat, capped = (v.cpu().numpy() for v in (ba, mant, stat, capped))
        assert not ba[:2 * nb].any() and (ba[2 * nb:] == CANARY).all()         # silence against silence: no noise, no bits
        assert not mant[:2 * half].any() and (mant[2 * half:] == CANARY).all()
        assert (stat[:4] == 0.0).all() and np.isnan(stat[4:]).all() and not capped[:2].any() and (capped[2:] == CANARY).all()
    finally:
        hd.close()
