"""
GPU tests of the bit-allocation back ends on crafted SMRs, budgets and lines (tests/alloc_cases.py): ties, values an ulp
from a 6 dB boundary, budgets around zero and beyond what fills every band -- what SMRs computed from audio never are.

  mrc_dev_alloc_quant          bitalloc_lane<9 | 18> + quantize_kernel (short and transition blocks), alloc_quant_long_kernel
                               <25 | 50> (long blocks), bitalloc_kernel<0> (long blocks, planes offset by 8 bytes)
  mrc_dev_alloc_quant_chained  chain_prep_kernel + chain_phase_b_kernel at 256, 512 and 1024 threads, with and without the
                               forced repair of the candidate order; as streams with the reservoir carried on the device,
                               with and without Huffman pricing
  Handle.bitalloc              bitalloc_cases_kernel (the generic instantiation), with the running SMRs it leaves

The yardstick is the oracle (oracle.bitalloc.BitAlloc, oracle.fast._quantise_batch, fast.ms_switch_batch; the host packer
for the Huffman savings).  Every output is an integer and every comparison exact equality; every output plane is followed
by a canary.
"""
import numpy as np
import pytest

import alloc_cases as ac
from test_gpu_stages import _dev, _full, _ptr

pytestmark = pytest.mark.gpu

CANARY = -31000                                              # fits the uint16 plane too; no output takes this value
OPT_FORCE_REPAIR, OPT_CHAIN_THREADS = 3, 4
COUNTS = [1, 63, 64, 65, None]                               # None: all cases
OFFSET = [(1024, 1024, False, 2.86, "offset8"), (1024, 1024, True, 2.86, "offset8")]   # -> bitalloc_kernel<0>
_OUT = {}                                                    # mrc_dev_alloc_quant on all cases, per configuration


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def handles():
    from mrcaudiocodec_amd import Handle
    hs = {t: Handle(device_id=0, target_bits_per_sample=t) for t in ac.TBPS}
    yield hs
    for hd in hs.values():
        hd.close()


def _id(cfg):
    return ac.config_id(cfg[:4]) + ("-" + cfg[4] if len(cfg) > 4 else "")


class Run:
    """the device buffers of one call on the first n blocks of `c` (every output plane followed by a canary), and the call"""

    def __init__(self, torch, hd, cfg, c, n, chained, offset8=False, index=None):
        lay = ac.layout(cfg)
        self.torch, self.h, self.cfg, self.lay, self.n, self.chained = torch, hd, cfg, lay, n, chained
        self.joint = cfg[2]
        nb, ns, half, nsig = lay["nb"], lay["ns"], lay["half"], lay["nsig"]
        pick = (lambda x: x[:n]) if index is None else (lambda x: x[index])
        i32 = torch.int32
        lines = pick(c["lines"])
        if offset8:
            buf = _full(torch, lines.size + 2, torch.float64, float("nan"))
            self.lines = buf[1:1 + lines.size]
            self.lines.copy_(_dev(torch, lines))
            assert self.lines.data_ptr() % 16 == 8
        else:
            self.lines = _dev(torch, lines)
        self.osc = _dev(torch, pick(c["overall_scale"]), i32)
        self.smr = _dev(torch, pick(c["smr"]))
        one = dict(sw=nb, ba=ns * nb, sf=ns * nb, mant=ns * half, ro=1, table=ns, trace=1)
        self.size = {k: n * v for k, v in one.items()}
        self.t = {}
        for k, v in one.items():
            dtype = torch.int16 if (k == "mant" and chained) else i32
            pad = 2 if (k == "mant" and offset8) else 0
            whole = _full(torch, pad + self.size[k] + v, dtype, CANARY)
            self.t[k] = whole[pad:]
            if pad:
                assert self.t[k].data_ptr() % 16 == 8
                self.front = whole[:pad]

    def call(self, res, bps=1, huff=0):
        t, n = self.t, self.n
        self.n_streams = n // bps
        self.size["ro"] = self.n_streams
        r = _dev(self.torch, res, self.torch.int32)
        a, b = self.cfg[:2]
        sw = _ptr(t["sw"]) if self.joint else None
        if self.chained:
            self.h.dev_alloc_quant_chained(a, b, n, self.joint, bps, huff, _ptr(self.lines), _ptr(self.osc), _ptr(self.smr),
                                           _ptr(r), sw, _ptr(t["ba"]), _ptr(t["sf"]), _ptr(t["mant"]), _ptr(t["table"]),
                                           _ptr(t["ro"]), _ptr(t["trace"]))
        else:
            assert bps == 1 and not huff
            self.h.dev_alloc_quant(a, b, n, self.joint, _ptr(self.lines), _ptr(self.osc), _ptr(self.smr), _ptr(r), sw,
                                   _ptr(t["ba"]), _ptr(t["sf"]), _ptr(t["mant"]), _ptr(t["ro"]))
        self.torch.cuda.synchronize()
        return self

    def _host(self, k):
        x = self.t[k].cpu().numpy()
        if x.dtype == np.int16:
            x = x.view(np.uint16)
        return x.astype(np.int64)

    def ints(self, what):
        """the outputs, after the canaries behind (and in front of) them have been found intact"""
        lay, n = self.lay, self.n
        used = ["ba", "sf", "mant", "ro"] + (["sw"] if self.joint else []) + (["table", "trace"] if self.chained else [])
        out = {}
        for k in self.t:
            x = self._host(k)
            size = self.size[k] if k in used else 0
            want = CANARY & 0xffff if (k == "mant" and self.chained) else CANARY
            assert (x[size:] == want).all(), "%s: %s written beyond its last entry" % (what, k)
            out[k] = x[:size]
        if hasattr(self, "front"):
            assert (self.front.cpu().numpy() == CANARY).all(), what + ": mantissa written in front of the plane"
        nb, ns, half = lay["nb"], lay["ns"], lay["half"]
        res = dict(bit_alloc=out["ba"].reshape(n, ns, nb), scale_factor=out["sf"].reshape(n, ns, nb),
                   mantissa=out["mant"].reshape(n, ns, half), reservoir_out=out["ro"])
        if self.joint:
            res["ms_switch"] = out["sw"].reshape(n, nb)
        if self.chained:
            res["table"], res["trace"] = out["table"].reshape(n, ns), out["trace"]
        return res


def _assert_equal(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, "%s %s: %d mismatching entries, first at %s (got %s, want %s)" % (
            what, k, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def _keys(joint):
    return ("bit_alloc", "reservoir_out", "scale_factor", "mantissa") + (("ms_switch",) if joint else ())


def _want(cfg, n):
    c, ref = ac.cases(cfg), ac.reference(cfg)
    want = {k: ref[k][:n] for k in ("bit_alloc", "reservoir_out", "scale_factor", "mantissa")}
    if cfg[2]:
        want["ms_switch"] = c["ms_switch"][:n]
    return want


def _independent(torch, hd, cfg, n, chained, offset8=False):
    c = ac.cases(cfg)
    n = len(c["reservoir"]) if n is None else n
    what = "%s n=%d %s" % (ac.config_id(cfg), n, "chained" if chained else "dev_alloc_quant")
    got = Run(torch, hd, cfg, c, n, chained, offset8).call(c["reservoir"][:n]).ints(what)
    _assert_equal(got, _want(cfg, n), _keys(cfg[2]), what + " vs oracle")
    if chained:                                              # no pricing: raw everywhere; the trace of one-block streams
        assert (got["table"] == 15).all() and np.array_equal(got["trace"], got["reservoir_out"]), what
    return got


def _batch_out(torch, handles, cfg):
    if cfg not in _OUT:
        _OUT[cfg] = _independent(torch, handles[cfg[3]], cfg, None, False)
    return _OUT[cfg]


# ------------------------------------------------------------------ 1. independent blocks, the batch back end
@pytest.mark.parametrize("cfg", ac.CONFIGS + OFFSET, ids=_id)
def test_independent_blocks_batch_back_end(torch, handles, cfg):
    offset8, cfg = len(cfg) > 4, cfg[:4]
    for n in COUNTS:
        got = _independent(torch, handles[cfg[3]], cfg, n, False, offset8)
        if n is None:
            if offset8:                                      # bitalloc_kernel<0> + quantize_kernel against the fused kernel
                _assert_equal(got, _batch_out(torch, handles, cfg), _keys(cfg[2]), _id(cfg) + " offset vs aligned")
            else:
                _OUT[cfg] = got


# ------------------------------------------------------------------ 2. independent blocks, the chained back end
@pytest.mark.parametrize("cfg", ac.CONFIGS, ids=ac.config_id)
def test_independent_blocks_chained_back_end(torch, handles, cfg):
    hd = handles[cfg[3]]
    batch = _batch_out(torch, handles, cfg)
    try:
        for threads in (0, 256, 512, 1024):
            hd.set_option(OPT_CHAIN_THREADS, threads)
            got = _independent(torch, hd, cfg, None, True)
            _assert_equal(got, batch, _keys(cfg[2]), "%s threads=%d: the two device back ends" % (ac.config_id(cfg), threads))
        hd.set_option(OPT_CHAIN_THREADS, 0)
        for n in COUNTS[:-1]:
            _independent(torch, hd, cfg, n, True)
        hd.set_option(OPT_FORCE_REPAIR, 1)
        repaired = _independent(torch, hd, cfg, None, True)
        _assert_equal(repaired, got, _keys(cfg[2]) + ("table", "trace"), ac.config_id(cfg) + " forced repair")
    finally:
        hd.set_option(OPT_FORCE_REPAIR, 0)
        hd.set_option(OPT_CHAIN_THREADS, 0)


# ------------------------------------------------------------------ 3. bitalloc_cases_kernel
@pytest.mark.parametrize("cfg", ac.CONFIGS, ids=ac.config_id)
def test_bitalloc_cases_kernel(handles, cfg):
    lay, c, ref = ac.layout(cfg), ac.cases(cfg), ac.reference(cfg)
    bits, left, after = handles[cfg[3]].bitalloc(c["budget"], ac.MAX_MANT, lay["n_lines"], c["vectors"], want_smr_after=True)
    n = len(left)
    got = dict(bit_alloc=bits.astype(np.int64).reshape(n, lay["ns"], lay["nb"]), reservoir_out=left.astype(np.int64))
    _assert_equal(got, ref, ("bit_alloc", "reservoir_out"), ac.config_id(cfg) + " Handle.bitalloc")
    bad = np.argwhere(after != ref["smr_after"])
    assert bad.size == 0, "%s: running SMRs differ in %d entries, first at %s" % (ac.config_id(cfg), len(bad), bad[0])


# ------------------------------------------------------------------ 4. streams: the reservoir carried on the device
def _stream_run(torch, hd, cfg, streams, huff):
    c = ac.stream_cases(cfg)
    idx = np.concatenate([np.arange(s * ac.STREAM_BLOCKS, (s + 1) * ac.STREAM_BLOCKS) for s in streams])
    what = "%s streams huffman=%d" % (ac.config_id(cfg), huff)
    run = Run(torch, hd, cfg, c, len(idx), True, index=idx).call(c["reservoir"][list(streams)], ac.STREAM_BLOCKS, huff)
    return run.ints(what), idx, what


@pytest.mark.parametrize("cfg", ac.STREAM_CONFIGS, ids=ac.config_id)
def test_streams_carry_the_reservoir(torch, handles, cfg):
    got, idx, what = _stream_run(torch, handles[cfg[3]], cfg, range(ac.N_STREAMS), 0)
    ref = ac.stream_reference(cfg)
    assert np.array_equal(ref["index"], idx)
    want = dict(ref, reservoir_out=ref["trace"][ac.STREAM_BLOCKS - 1::ac.STREAM_BLOCKS])
    if cfg[2]:
        want["ms_switch"] = ac.stream_cases(cfg)["ms_switch"][idx]
    _assert_equal(got, want, _keys(cfg[2]) + ("trace", "table"), what)
    full = got["bit_alloc"].reshape(ac.N_STREAMS, ac.STREAM_BLOCKS, -1)[3]      # the stream that starts with 10^6 bits
    lay = ac.layout(cfg)
    drained = (lay["fill"] - lay["base"]) * ac.STREAM_BLOCKS > 10 ** 6          # (a short block spends too little for that)
    assert (full[0] == ac.MAX_MANT).all() and (full[-1] == ac.MAX_MANT).all() != drained


@pytest.mark.parametrize("cfg", ac.STREAM_CONFIGS, ids=ac.config_id)
def test_streams_with_huffman_pricing(torch, handles, cfg):
    """the reservoir also takes what the cheapest table saves (codecThem.py:224,274): the host packer prices every block of
    the reference.  The stream that starts with 10^6 bits codes 16-bit mantissas, far past every table's escape value."""
    from mrcaudiocodec_amd import pacfile as ppac
    a, b, joint, tbps = cfg
    c, lay = ac.stream_cases(cfg), ac.layout(cfg)
    pcfg = ppac.make_config(target_bits_per_sample=tbps)

    def saved_of(i, bits, sf, mant):
        osc = c["overall_scale"][i][None]
        if joint:
            _, _, table, saved = ppac.pack_joint_blocks(pcfg, a, b, osc, c["ms_switch"][i][None], sf[None], bits[None],
                                                        mant[None].astype(np.int32), True)
        else:
            _, _, table, saved = ppac.pack_blocks(pcfg, a, b, osc, sf[None], bits[None], mant[None].astype(np.int32), True)
        return int(np.asarray(saved).sum()), np.asarray(table).reshape(-1)

    streams = [0, 1, 3, 5]
    got, idx, what = _stream_run(torch, handles[tbps], cfg, streams, 1)
    ref = ac.stream_reference(cfg, streams, saved_of)
    want = dict(ref, reservoir_out=ref["trace"][ac.STREAM_BLOCKS - 1::ac.STREAM_BLOCKS])
    if joint:
        want["ms_switch"] = c["ms_switch"][idx]
    _assert_equal(got, want, _keys(joint) + ("trace", "table"), what)
    assert got["mantissa"].max() > 1 << 12 and len(set(got["table"].ravel().tolist())) >= 3, what
    plain = ac.stream_reference(cfg, streams)
    assert not np.array_equal(plain["trace"], ref["trace"])                    # the savings do move the reservoir


# ------------------------------------------------------------------ 5. refusals of the chained entry
def test_chained_entry_refusals(torch, handles):
    from mrcaudiocodec_amd import MrcError
    hd = handles[2.86]
    for cfg in [(1024, 1024, False, 2.86), (1024, 1024, True, 2.86)]:
        a, b, joint, _ = cfg
        c = ac.cases(cfg)
        r = Run(torch, hd, cfg, c, 4, True)
        t = r.t
        res = _dev(torch, c["reservoir"][:4], torch.int32)
        sw = _ptr(t["sw"]) if joint else None

        def call(a=a, b=b, n=4, bps=1, lines=_ptr(r.lines), osc=_ptr(r.osc), smr=_ptr(r.smr), sw=sw, ba=_ptr(t["ba"]),
                 sf=_ptr(t["sf"]), mant=_ptr(t["mant"]), ro=_ptr(t["ro"])):
            hd.dev_alloc_quant_chained(a, b, n, joint, bps, 0, lines, osc, smr, _ptr(res), sw, ba, sf, mant, _ptr(t["table"]),
                                       ro, _ptr(t["trace"]))

        call(n=0)                                            # no frames: nothing to do, and OK
        bad = [dict(lines=None), dict(osc=None), dict(smr=None), dict(ba=None), dict(sf=None), dict(mant=None), dict(ro=None),
               dict(n=-1), dict(bps=0), dict(bps=-1), dict(bps=3), dict(bps=8),
               dict(lines=_ptr(r.lines) + 8), dict(mant=_ptr(t["mant"]) + 2),
               dict(a=162, b=162),                           # lines no multiple of four: outside the chained back end
               dict(a=1152, b=1152)]                         # a shape the handle refuses
        if joint:
            bad.append(dict(sw=None))
        for kw in bad:
            with pytest.raises(MrcError) as e:
                call(**kw)
            assert e.value.code == -1 and not str(e.value).endswith("?"), kw   # MRC_ERR_INVALID, with a message
        torch.cuda.synchronize()
        for k in t:
            assert (t[k].cpu().numpy() == CANARY).all(), k   # nothing was written by any of them
