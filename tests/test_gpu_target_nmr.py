"""
GPU tests of the encode to a target noise-to-mask ratio (mrc_encode_chained_target_nmr_pac, Handle.encode_chained_pac_target_nmr,
pacfile.encode_stream_target_nmr, cli --target-nmr).

The yardstick is always the existing pair, never the new code: Handle.encode_chained_pac_ladder for the bytes of every rung
and pacfile.measure_nmr (mrc_pac_nmr) on those bytes for the numbers.  Every comparison is equality: the same doubles, the
same counts, the same bytes.  The rule is applied to the yardstick's values in this file.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import HOP, handle as _handle, handles_closed_after_module as _close_handles  # noqa: F401

pytestmark = pytest.mark.gpu
RATES = (1.5, 2.86, 4.0, 8.0)


def _kinds(hops, mono):
    """loud noise, a quiet tone pair, digital silence, a click train"""
    from mrcaudiocodec_amd import synth
    n = (hops + 1) * HOP
    nch = 1 if mono else 2
    noise = np.stack([synth.c2_noise(hops, seed=5 + c, sigma=0.25) for c in range(nch)])
    tones = np.stack([synth.c1_sine(hops, freq=523.0 + 100 * c, amp=0.004) + synth.c1_sine(hops, freq=659.0, amp=0.003)
                      for c in range(nch)])
    return [kit.to_pcm(noise), kit.to_pcm(tones), np.zeros((nch, n), np.int16), kit.clicks(hops, 31, mono, period=5)]


class Case:
    """streams (int16 [nCh][n] each, equal n), their shapes, and the yardstick: files[r][s], nmr[r][s]"""

    def __init__(self, h, pcms, use_huffman=True, rates=RATES):
        from mrcaudiocodec_amd import pacfile
        self.h, self.pcms, self.rates, self.huff = h, pcms, rates, use_huffman
        self.mono = pcms[0].shape[0] == 1
        self.shapes = [kit.shapes_to_last_long(h, p) for p in pcms]
        self.ns = [len(sh) * HOP for sh in self.shapes]
        self.left = np.stack([p[0] for p in pcms])
        self.right = None if self.mono else np.stack([p[1] for p in pcms])
        rs = h.encode_chained_pac_ladder(self.left, self.right, self.shapes, rates, use_huffman=use_huffman, num_samples=self.ns)
        self.files = [[r["bytes"][r["stream_offset"][s]:r["stream_offset"][s + 1]].tobytes() for s in range(len(pcms))] for r in rs]
        self.nmr = []
        for r in range(len(rates)):
            srcs = []
            for p, sh in zip(pcms, self.shapes):
                end = int(sh[-1][0] + sh[-1][1] + sh[-1][2])
                srcs.append(np.ascontiguousarray(p[:, HOP:end]))
            self.nmr.append(pacfile.measure_nmr(h, self.files[r], srcs))

    def totals(self, s):
        return [self.nmr[r][s]["nmr_total_db"] for r in range(len(self.rates))]

    def run(self, target, **kw):
        return self.h.encode_chained_pac_target_nmr(self.left, self.right, self.shapes, self.rates, target,
                                                    use_huffman=self.huff, num_samples=self.ns, **kw)


def _rule(vals, target):
    for r, v in enumerate(vals):
        if v <= target:
            return r, True
    return len(vals) - 1, False


def _check(case, got, target):
    assert len(got) == len(case.pcms)
    for s, g in enumerate(got):
        for r in range(len(case.rates)):
            w = case.nmr[r][s]
            assert g["nmr_total_db"][r] == w["nmr_total_db"], (s, r, g["nmr_total_db"][r], w["nmr_total_db"])
            assert g["nmr_max_db"][r] == w["nmr_max_db"], (s, r, g["nmr_max_db"][r], w["nmr_max_db"])
            assert g["disturbed_blocks"][r] == w["disturbed_blocks"], (s, r)
            assert g["n_blocks"] == w["n_blocks"], (s, r)
        chosen, met = _rule(case.totals(s), target)
        assert (g["chosen"], g["met"]) == (chosen, met), (s, g["chosen"], g["met"], chosen, met, case.totals(s), target)
        assert g["rate"] == case.rates[chosen]
        assert g["data"] == case.files[chosen][s], (s, chosen, len(g["data"]), len(case.files[chosen][s]))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["data"] == y["data"] and (x["chosen"], x["met"], x["n_blocks"]) == (y["chosen"], y["met"], y["n_blocks"])
        for k in ("nmr_total_db", "nmr_max_db", "disturbed_blocks"):
            assert np.array_equal(x[k], y[k]), k


_CASES = {}


def _case(mono, huff=True, exact=False):
    key = (mono, huff, exact)
    if key not in _CASES:
        h = _handle(exact)
        pcm = kit.clicks(30, 11, mono, period=6)
        c = Case(h, [pcm], use_huffman=huff)
        assert len({(int(a), int(b)) for (_, a, b) in c.shapes[0]}) == 4, "all four block shapes"
        assert all(w["n_blocks"] == len(c.shapes[0]) + 1 for w in (c.nmr[r][0] for r in range(4))), "Close()'s block"
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("huff", [True, False])
@pytest.mark.parametrize("mono", [False, True])
def test_numbers_equal_the_ladder_measured(mono, huff):
    c = _case(mono, huff)
    _check(c, c.run(-3.0), -3.0)


def test_silence_is_minus_infinity():
    h = _handle()
    c = Case(h, [np.zeros((2, 25 * HOP), np.int16)])
    assert all(v == -math.inf for v in c.totals(0))
    got = c.run(-200.0)
    _check(c, got, -200.0)
    assert got[0]["nmr_total_db"][0] == -math.inf and got[0]["chosen"] == 0 and got[0]["met"]


@pytest.mark.parametrize("mono", [False, True])
def test_rule_and_bytes(mono):
    c = _case(mono)
    tot = c.totals(0)
    targets = [-math.inf, math.inf, min(tot) - 1.0] + [0.5 * (a + b) for a, b in zip(tot, tot[1:])] + list(tot)
    for t in targets:
        _check(c, c.run(t), t)
    got = c.run(min(tot) - 1.0)[0]
    assert not got["met"] and got["chosen"] == len(RATES) - 1
    got = c.run(tot[1])[0]                              # <= is inclusive
    assert got["met"] and got["chosen"] == _rule(tot, tot[1])[0] <= 1
    assert c.run(math.inf)[0]["chosen"] == 0


@pytest.mark.parametrize("mono", [False, True])
def test_many_streams_choose_different_rungs(mono):
    h = _handle()
    c = Case(h, _kinds(24, mono))
    # a target between the values of one stream's rungs: picked so that three rungs or more are chosen over the streams
    cands = sorted({v for s in range(4) for v in c.totals(s) if math.isfinite(v)})
    best = max(cands, key=lambda t: len({_rule(c.totals(s), t)[0] for s in range(4)}))
    assert len({_rule(c.totals(s), best)[0] for s in range(4)}) >= 3, [c.totals(s) for s in range(4)]
    got = c.run(best)
    _check(c, got, best)
    assert len({g["chosen"] for g in got}) >= 3
    _same(got, c.run(best))
    for s in range(4):
        one = h.encode_chained_pac_target_nmr(c.left[s:s + 1], None if mono else c.right[s:s + 1], [c.shapes[s]], RATES, best,
                                              num_samples=[c.ns[s]])
        _same(one, got[s:s + 1])


def test_slabs_do_not_change_anything():
    h = _handle()
    try:
        long = Case(h, [kit.clicks(40, 17, False, period=6)])
        tot = long.totals(0)
        t = 0.5 * (tot[1] + tot[2])
        want = long.run(t)
        _check(long, want, t)
        assert len(long.shapes[0]) > 2 * 12
        h.set_option(6, 12)                              # <= 12 blocks per slab: three time slabs or more
        _same(long.run(t), want)
        h.set_option(6, 131072)
        from mrcaudiocodec_amd import synth
        short = Case(h, [kit.to_pcm(np.stack([synth.c2_noise(8, seed=70 + 2 * s + c, sigma=0.02 * (s + 1)) for c in range(2)]))
                         for s in range(6)])
        cands = sorted(v for s in range(6) for v in short.totals(s))
        t = cands[len(cands) // 2]
        want = short.run(t)
        _check(short, want, t)
        assert sum(len(sh) for sh in short.shapes) > 20 >= max(len(sh) for sh in short.shapes)
        h.set_option(6, 20)                              # whole streams, several slabs
        _same(short.run(t), want)
    finally:
        h.set_option(6, 131072)


def test_exact_spreading_mode():
    c = _case(False, True, exact=True)
    tot = c.totals(0)
    t = 0.5 * (tot[0] + tot[1])
    _check(c, c.run(t), t)


@pytest.mark.parametrize("mono", [False, True])
def test_device_entry_point(mono):
    import torch
    c = _case(mono)
    h = c.h
    tot = c.totals(0)
    t = 0.5 * (tot[1] + tot[2])
    want = c.run(t)
    dev = torch.device("cuda", 0)
    left = torch.from_numpy(c.left).to(dev)
    right = None if mono else torch.from_numpy(c.right).to(dev)
    cap = len(want[0]["data"]) + 64
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    got = h.encode_chained_pac_target_nmr(None, None, c.shapes, RATES, t, num_samples=c.ns,
                                          device=(left.data_ptr(), None if mono else right.data_ptr(), left.shape[1],
                                                  out.data_ptr(), cap))
    host = out.cpu().numpy()
    for g in got:
        lo, hi = g["data"]
        g["data"] = host[lo:hi].tobytes()
    _same(got, want)
    assert not host[len(want[0]["data"]):].any()


def test_second_batch_of_one_shape_equals_single_batch_slabs():
    """Inside a slab the blocks of one shape are analysed 16384 at a time.  4096-block slabs: time slabs of one batch each,
    the path of every other test; the default slab: one slab whose (S,S) group is a full batch and a batch of five."""
    h = _handle()
    pcm, shapes, ns = kit.long_short_run(period=6)
    rates = (2.86, 8.0)
    run = lambda: h.encode_chained_pac_target_nmr(pcm, None, [shapes], rates, 0.0, num_samples=[ns])
    try:
        h.set_option(6, 4096)
        want = run()
        h.set_option(6, 131072)
        got = run()
    finally:
        h.set_option(6, 131072)
    assert want[0]["n_blocks"] == len(shapes) + 1 and len(want[0]["data"]) > 0
    _same(got, want)
    assert got[0]["rate"] == want[0]["rate"]


def _raw(h, c, rates, target, out_cap=None, num_samples=True, start=None, off=None, a=None, b=None):
    """the C entry point itself -> (rc, out, total, results...)"""
    from mrcaudiocodec_amd import _lib
    s0, o0, a0, b0 = h._chain_schedule(c.shapes)
    start = s0 if start is None else np.ascontiguousarray(start, np.int64)
    off = o0 if off is None else np.ascontiguousarray(off, np.int64)
    a = a0 if a is None else np.ascontiguousarray(a, np.int32)
    b = b0 if b is None else np.ascontiguousarray(b, np.int32)
    n = len(start) - 1
    rates = np.ascontiguousarray(rates, np.float64)
    R = max(len(rates), 1)
    ns = np.ascontiguousarray(c.ns, np.uint32)
    cap = h.chain_out_bound(s0, a0, b0, True, True, 1 if c.mono else 2) if out_cap is None else out_cap
    out = np.full(max(cap, 1) + 32, 0xEE, np.uint8)
    res = dict(s_off=np.zeros(n + 1, np.int64), chosen=np.full(n, -7, np.int32), met=np.full(n, -7, np.int32),
               tot=np.full((R, n), np.nan), mx=np.full((R, n), np.nan), dist=np.full((R, n), -7, np.int64),
               nblk=np.full(n, -7, np.int64), total=np.full(1, -7, np.int64))
    p = lambda arr: arr.ctypes.data
    rc = _lib.lib.mrc_encode_chained_target_nmr_pac(
        h._h, len(rates), p(rates), float(target), n, c.left.ctypes.data_as(C.c_void_p),
        None if c.mono else c.right.ctypes.data_as(C.c_void_p), c.left.shape[1], p(start), p(off), p(a), p(b), 1,
        ns.ctypes.data_as(C.c_void_p) if num_samples else None, out.ctypes.data_as(C.c_void_p), cap, p(res["s_off"]),
        p(res["chosen"]), p(res["met"]), p(res["tot"]), p(res["mx"]), p(res["dist"]), p(res["nblk"]), p(res["total"]))
    return rc, out, res


def test_out_cap_too_small():
    from mrcaudiocodec_amd import _lib
    c = _case(False)
    h = c.h
    tot = c.totals(0)
    t = 0.5 * (tot[1] + tot[2])
    chosen = _rule(tot, t)[0]
    want = c.files[chosen][0]
    rc, out, res = _raw(h, c, RATES, t, out_cap=len(want) - 1)
    assert rc == _lib.MRC_ERR_NOMEM
    assert np.all(out == 0xEE), "nothing is written when the bytes do not fit"
    assert int(res["total"][0]) == len(want) and list(res["s_off"]) == [0, len(want)]
    assert int(res["chosen"][0]) == chosen and int(res["met"][0]) == 1 and int(res["nblk"][0]) == c.nmr[0][0]["n_blocks"]
    for r in range(4):
        assert res["tot"][r, 0] == c.nmr[r][0]["nmr_total_db"] and res["mx"][r, 0] == c.nmr[r][0]["nmr_max_db"]
        assert res["dist"][r, 0] == c.nmr[r][0]["disturbed_blocks"]
    buf = np.zeros(len(want), np.uint8)
    total = np.zeros(1, np.int64)
    assert _lib.lib.mrc_chain_fetch_output(h._h, buf.ctypes.data_as(C.c_void_p), buf.size, total.ctypes.data) == 0
    assert buf.tobytes() == want and int(total[0]) == len(want)
    # the binding does the same on its own
    assert c.run(t, out_cap=16)[0]["data"] == want
    # and a buffer of exactly the size is enough
    rc, out, res = _raw(h, c, RATES, t, out_cap=len(want))
    assert rc == 0 and out[:len(want)].tobytes() == want and np.all(out[len(want):] == 0xEE)


def test_refusals_name_the_argument():
    from mrcaudiocodec_amd import _lib
    c = _case(False)
    h = c.h
    start, off, a, b = h._chain_schedule(c.shapes)

    def refused(word, **kw):
        rates = kw.pop("rates", RATES)
        target = kw.pop("target", 0.0)
        rc, out, _ = _raw(h, c, rates, target, **kw)
        msg = _lib.lib.mrc_last_error(h._h).decode()
        assert rc == _lib.MRC_ERR_INVALID and word in msg, (rc, msg)
        assert np.all(out == 0xEE)

    refused("n_rates", rates=[])
    refused("n_rates", rates=np.linspace(1, 9, 17))
    refused("target_bits_per_sample[1]", rates=[1.5, math.nan])
    refused("target_bits_per_sample[1]", rates=[1.5, math.inf])
    refused("target_bits_per_sample[0]", rates=[0.0, 2.0])
    refused("target_bits_per_sample[1]", rates=[1.5, 65.0])
    refused("ascending", rates=[1.5, 4.0, 2.86])
    refused("ascending", rates=[1.5, 1.5])
    refused("target_nmr_total_db", target=math.nan)
    refused("num_samples", num_samples=False)
    h.set_option(5, 1)
    try:
        refused("MRC_OPT_SENSITIVITY")
    finally:
        h.set_option(5, 0)
    first_short = a.copy()
    first_short[0] = 128
    refused("first block", a=first_short)
    shifted = off.copy()
    shifted[3] += 64
    refused("block_offset[3]", off=shifted)
    ends_short = b.copy()
    ends_short[-1] = 128
    refused("last block", b=ends_short)
    _check(c, c.run(0.0), 0.0)                           # the handle still works


def test_cli_target_nmr(tmp_path, capsys):
    from mrcaudiocodec_amd import cli
    from mrcaudiocodec_amd import synth
    # the file ends in long blocks and in two silent hops: mrc_pac_nmr measures Close()'s block against the samples that
    # follow the last coded block, the call against the zeros Close() coded -- the same thing when the WAV ends in silence
    tail = kit.to_pcm(np.stack([synth.c1_sine(3, freq=440.0, amp=0.05)] * 2))[:, HOP:]
    pcm = np.concatenate([kit.clicks(22, 23, False, period=6)[:, HOP:], tail, np.zeros((2, 2 * HOP), np.int16)], axis=1)
    wav = kit.write_wav(tmp_path / "in.wav", pcm)
    lad = cli.encode_wav(wav, None, bits_per_sample="1.5,2.86,4,8")
    dst = str(tmp_path / "out.pac")
    probe = cli.encode_wav_target_nmr(wav, None, "1.5,2.86,4,8", "inf")
    tot = [float(v) for v in probe["nmr_total_db"]]
    t = 0.5 * (tot[1] + tot[2])
    capsys.readouterr()
    cli.main([wav, dst, "--bits-per-sample", "1.5,2.86,4,8", "--target-nmr", repr(t)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    k = [1.5, 2.86, 4.0, 8.0].index(line["chosen_bits_per_sample"])
    assert k == _rule(tot, t)[0] and line["met"] is True
    data = open(dst, "rb").read()
    assert data == lad[k] == cli.encode_wav(wav, None, bits_per_sample=str(line["chosen_bits_per_sample"]))
    cli.main([wav, dst, "--measure"])
    meas = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert meas["nmr_total_db"] == line["nmr_total_db"][k] and meas["nmr_max_db"] == line["nmr_max_db"][k]
    assert meas["disturbed_blocks"] == line["disturbed_blocks"][k] and meas["n_blocks"] == line["n_blocks"]
    for extra in (["-d"], ["--certify"], ["--measure"]):
        with pytest.raises(SystemExit):
            cli.main([wav, dst, "--bits-per-sample", "1.5,4", "--target-nmr", "0"] + extra)
    for argv in (["--bits-per-sample", "4", "--target-nmr", "0"], ["--target-nmr", "0"],
                 ["--bits-per-sample", "4,1.5", "--target-nmr", "0"], ["--bits-per-sample", "1.5,4", "--target-nmr", "nan"]):
        with pytest.raises(SystemExit):
            cli.main([wav, dst] + argv)
    with pytest.raises(SystemExit):
        cli.main([wav, str(tmp_path / "out_{bps}.pac"), "--bits-per-sample", "1.5,4", "--target-nmr", "0"])
    capsys.readouterr()
