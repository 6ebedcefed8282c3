#!/usr/bin/env python3
"""
Golden vectors at sample rates other than 48 and 44.1 kHz, from the reference's OWN code executed through
tests/golden/py2harness.py (as make_golden_ref.py, make_golden_pac.py and make_golden_mono.py do):

    python tests/golden/make_golden_rates.py [/root/reference]   ->  tests/golden/ref_rates.npz, ref_rates_smr.npz,
                                                                    ref_pac_rates.npz

ref_rates.npz      Thresh / Intensity(Thresh) / SPL on the line grids of 1024, 576 and 128 lines at 32, 88.2, 96 and 192 kHz
                   (psychoac.py:8-25; from ~80 kHz on Intensity(Thresh(f)) of the top lines is +inf -- recorded as such);
                   band tables at those rates, and whether AssignMDCTLinesFromFreqLimits (psychoac.py:86-105) accepts or
                   raises on either side of the lowest rate each block shape is defined at; EncodeSingleChannel /
                   JointEncodeChannels chains (codecThem.py:136-354, 359-574) with the reservoir carried, at 96 and
                   32 kHz, long-only and switched
ref_rates_smr.npz  getMaskedThreshold / CalcSMRs (psychoac.py:134-219) of the four reference shapes at the four rates, on
                   content with energy above 20 kHz (no CalcSMRs for (128,128) at 192 kHz: two of its bands are empty, and
                   the reference's band maximum raises ValueError there)
ref_pac_rates.npz  the reference CLI (pacfileThem.py run as a script) on short stereo WAVs at 32 and 96 kHz: .pac bytes
                   (Huffman tables present) and the WAV its decode direction wrote; one mono 96 kHz file through the mono
                   harness of make_golden_mono.py.  At 96 kHz the reference's transient filter (cheby2(20, 40, 9000/fs)
                   as tf2sos) is unstable and codes the stream almost entirely as short blocks: reference behaviour.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

import py2harness as H                          # noqa: E402
from oracle import huffman_tables as HT          # noqa: E402   (table data)
import make_golden_mono as GM                    # noqa: E402   (the mono harness; its driver does not run on import)
import mono_oracle as MO                         # noqa: E402   (WAV bytes)

R = H.load_reference(REF)
rw, rmdct, rq, rp, rc = R["window"], R["mdct"], R["quantize"], R["psychoac"], R["codecThem"]
rng = np.random.default_rng(20261016)
SHORT_LIMITS = [300, 630, 1080, 1720, 2700, 4400, 7700, 15500, 24000]      # pacfileThem.py:643
SHAPES = [(1024, 1024), (1024, 128), (128, 128), (128, 1024)]
RATES = (32000, 88200, 96000, 192000)
# the lowest integer rate each shape is defined at (the centre of its last line >= 15500 Hz): (a, b) -> rate
LOWEST = {(1024, 1024): 31016, (1024, 128): 31027, (576, 576): 31027, (162, 162): 31096, (128, 128): 31122}


def pcm_to_float(pcm):
    """pcmfile.py:91-100 through the reference's own vDequantizeUniform."""
    codes = np.asarray([int(v) for v in pcm])
    signs = np.signbit(codes)
    codes[signs] *= -1
    temp = rq.vDequantizeUniform(codes, 16)
    temp[signs] *= -1.
    return temp


def gauss_pcm(n, sigma):
    return np.clip(np.rint(rng.normal(0, sigma * 32767, n)), -32767, 32767).astype(np.int16)


def limits_of(a, b):
    return None if a + b == 2048 else SHORT_LIMITS


def bands(a, b, fs):
    half = (a + b) // 2
    lim = limits_of(a, b)
    nl = rp.AssignMDCTLinesFromFreqLimits(half, fs) if lim is None else rp.AssignMDCTLinesFromFreqLimits(half, fs, lim)
    return rp.ScaleFactorBands(nl)


def grid(half, fs):
    return (np.arange(half) + 0.5) * ((float(fs) / half) / 2.)


def first_inf_freq(half, fs):
    """centre of the first line of the grid whose quiet threshold overflows, or None"""
    with np.errstate(over="ignore"):
        q = rp.Intensity(rp.Thresh(grid(half, fs)))
    k = np.flatnonzero(np.isinf(q))
    return None if not len(k) else grid(half, fs)[k[0]]


def rate_blocks(N, fs):
    """16-bit content of N samples whose peaks and maskers reach the region where the quiet threshold overflows:
    white noise up to Nyquist, tones at 30 / 40 / 45 kHz (those below Nyquist; 14 kHz at 32 kHz) in one block, a tone just below the first line whose
    quiet threshold is +inf (the top line where none is), digital silence"""
    t = np.arange(N)
    rows = [gauss_pcm(N, 0.1)]
    x = sum(6000 * np.sin(2 * np.pi * f / fs * t + 0.3) for f in (30000.0, 40000.0, 45000.0, 14000.0) if f < 0.45 * fs)
    rows.append(np.clip(np.rint(x + rng.normal(0, 30, N)), -32767, 32767).astype(np.int16))
    f0 = first_inf_freq(N // 2, fs)
    f0 = (f0 if f0 is not None else grid(N // 2, fs)[-1]) - 0.75 * fs / N
    x = 9000 * np.sin(2 * np.pi * f0 / fs * t) + 3000 * np.sin(2 * np.pi * 1000.0 / fs * t + 1) + rng.normal(0, 20, N)
    rows.append(np.clip(np.rint(x), -32767, 32767).astype(np.int16))
    rows.append(np.zeros(N, np.int16))
    return np.array(rows)


def params(fs, nch):
    cp = types.SimpleNamespace()           # audiofile.py:51-53 is an empty attribute bag
    cp.sampleRate, cp.nChannels, cp.nMDCTLines = fs, nch, 1024
    cp.nScaleBits, cp.nMantSizeBits, cp.targetBitsPerSample = 4, 4, 2.86
    cp.nSamplesPerBlock, cp.bitReservoir, cp.nSamplesShort = 1024, 0, 128
    cp.a = cp.b = 1024
    cp.blkswBitA = cp.blkswBitB = 1
    return cp


def shape_cycle(n_hops, transient_hops):
    """block shapes as the reference CLI produces them (pacfileThem.py:1192-1210)"""
    shapes, a = [], 1024
    for h in range(n_hops):
        if h in transient_hops:
            for _ in range(8):
                shapes.append((a, 128)); a = 128
        else:
            shapes.append((a, 1024)); a = 1024
    return shapes


def stereo_pcm(n_hops, fs):
    """noise with level steps, half the hops correlated, and a 30 kHz tone where the rate has one"""
    n = n_hops * 1024
    g1, g2 = gauss_pcm(n, 0.1).astype(np.float64), gauss_pcm(n, 0.1).astype(np.float64)
    t = np.arange(n)
    hop = t // 1024
    tone = 4000 * np.sin(2 * np.pi * 30000.0 / fs * t) if fs > 64000 else 4000 * np.sin(2 * np.pi * 12000.0 / fs * t)
    right = np.where(hop % 2 == 0, 0.8 * g1 + 0.2 * g2, 0.1 * g2)
    lvl = 10.0 ** (-1.5 * (hop % 5 == 3))
    pcm = np.stack([g1 * lvl + tone, right * lvl + 0.5 * tone])
    return np.clip(np.rint(pcm), -32767, 32767).astype(np.int16)


def dense(m, ba, nlines):
    out = np.zeros(int(np.sum(nlines)), dtype=np.int64)
    lo = np.cumsum(nlines) - nlines
    i = 0
    for k in range(len(nlines)):
        if ba[k]:
            out[lo[k]:lo[k] + nlines[k]] = m[i:i + nlines[k]]
            i += nlines[k]
    assert i == len(m)
    return out


def run_chain(e, tag, pcm, shapes, fs, joint):
    """EncodeSingleChannel (channel 0) / JointEncodeChannels over consecutive blocks framed as WriteDataBlock /
    JointWriteDataBlock frame them (pacfileThem.py:628-645, 799-816), the reservoir carried in cp; stored in the layout
    of make_golden_ref.py's chains (tests/refgold.py check_chain reads it)."""
    cp = params(fs, 2 if joint else 1)
    x = np.array([pcm_to_float(ch) for ch in pcm])
    nch = x.shape[0]
    prior = np.zeros((nch, 1024))
    pos, res_in, res_out = 0, [], []
    for i, (a, b) in enumerate(shapes):
        new = x[:, pos:pos + b]
        pos += b
        full = [np.concatenate((prior[c][-a:], new[c])) for c in range(nch)]
        prior = new
        cp.a, cp.b, cp.sfBands = a, b, bands(a, b, fs)
        res_in.append(cp.bitReservoir)
        k = "%s_%d" % (tag, i)
        nl = cp.sfBands.nLines
        if joint:
            sf, ba, mant, osf, ms = rc.JointEncodeChannels(full[0].copy(), full[1].copy(), cp)
            e[k + "_ms"] = np.array(ms, dtype=np.int64)
        else:
            s1, b1, m1, o1 = rc.EncodeSingleChannel(full[0].copy(), cp)
            sf, ba, mant, osf = [s1], [b1], [m1], [o1]
        res_out.append(cp.bitReservoir)
        e[k + "_sf"], e[k + "_ba"] = np.array(sf, dtype=np.int64), np.array(ba, dtype=np.int64)
        e[k + "_os"], e[k + "_table"] = np.array(osf, dtype=np.int64), np.array([15] * len(sf), dtype=np.int64)
        for c in range(len(sf)):
            e[k + "_mant%d" % c] = dense(np.asarray(mant[c]), np.asarray(ba[c]), nl)
    e[tag + "_pcm"] = pcm if joint else pcm[:1]
    e[tag + "_shapes"] = np.array(shapes)
    e[tag + "_res_in"], e[tag + "_res_out"] = np.array(res_in), np.array(res_out)
    e[tag + "_params"] = np.array([fs, cp.nChannels, cp.nScaleBits, cp.nMantSizeBits, cp.targetBitsPerSample])


# ------------------------------------------------------------------------------------------------ ref_rates.npz
r = {"rates": np.array(RATES)}
with np.errstate(over="ignore", divide="ignore"):
    for fs in RATES:
        for half in (1024, 576, 128):
            key = "%d_%d" % (half, fs)
            f = grid(half, fs)
            r["thresh_" + key] = rp.Thresh(f)
            r["quiet_" + key] = rp.Intensity(rp.Thresh(f))
            r["spl_quiet_" + key] = rp.SPL(rp.Intensity(rp.Thresh(f)))
        for half, kind in ((1024, "cb"), (576, "short"), (128, "short")):
            nl = rp.AssignMDCTLinesFromFreqLimits(half, fs) if kind == "cb" else \
                rp.AssignMDCTLinesFromFreqLimits(half, fs, SHORT_LIMITS)
            r["bt_nlines_%d_%d_%s" % (half, fs, kind)] = rp.ScaleFactorBands(nl).nLines
# the band loop's domain: 1 = accepted, 0 = IndexError, at r* - 1 and r* for each shape (and two rates far below)
dom = []
for (a, b), lo in LOWEST.items():
    lim = SHORT_LIMITS if (a, b) != (1024, 1024) else None
    for fs in (22050, 31000, lo - 1, lo, lo + 1):
        try:
            if lim is None:
                rp.AssignMDCTLinesFromFreqLimits((a + b) // 2, fs)
            else:
                rp.AssignMDCTLinesFromFreqLimits((a + b) // 2, fs, lim)
            ok = 1
        except IndexError:
            ok = 0
        dom.append((a, b, fs, ok))
r["domain"] = np.array(dom)
for fs in RATES:
    for (a, b) in SHAPES:
        N = a + b
        sfb = bands(a, b, fs)
        pcm = rate_blocks(N, fs)
        thr, smr, scl = [], [], []
        with np.errstate(over="ignore", divide="ignore"):
            for row in pcm:
                x = pcm_to_float(row)
                X = rmdct.MDCT(rw.TransitionWindow(x, a, b), a, b)[:N // 2]
                sc = rq.ScaleFactor(np.max(np.abs(X)), 4)
                X = X * (1 << sc)
                thr.append(rp.getMaskedThreshold(x, X, sc, fs, sfb))
                if min(sfb.nLines) > 0:             # (an empty band: np.amax of nothing raises, psychoac.py:217)
                    smr.append(rp.CalcSMRs(x, X, sc, fs, sfb))
                scl.append(sc)
        key = "%d_%d_%d" % (a, b, fs)
        r["pcm_" + key], r["thr_" + key], r["scale_" + key] = pcm, np.array(thr), np.array(scl)
        if smr:
            r["smr_" + key] = np.array(smr)
with np.errstate(over="ignore", divide="ignore"):
    for fs in (96000, 32000):
        k = fs // 1000
        run_chain(r, "r%dlong" % k, stereo_pcm(3, fs), shape_cycle(3, set()), fs, False)
        run_chain(r, "r%dsingle" % k, stereo_pcm(3, fs), shape_cycle(3, {1}), fs, False)
        run_chain(r, "r%djointch" % k, stereo_pcm(4, fs), shape_cycle(4, {2}), fs, True)
        run_chain(r, "r%djointlong" % k, stereo_pcm(3, fs), shape_cycle(3, set()), fs, True)
smr_keys = [k for k in r if k.startswith(("pcm_", "thr_", "smr_", "scale_"))]
np.savez_compressed(os.path.join(HERE, "ref_rates_smr.npz"), **{k: r.pop(k) for k in smr_keys})
np.savez_compressed(os.path.join(HERE, "ref_rates.npz"), **r)


# ------------------------------------------------------------------------------------------------ ref_pac_rates.npz
def wav_content(seed, n, rate, burst_at):
    g = np.random.default_rng(seed)
    t = np.arange(n)
    g1, g2 = g.normal(0, 0.1 * 32767, n), g.normal(0, 0.1 * 32767, n)
    hop = t // 1024
    lvl = 10.0 ** (-1.5 * (hop % 5 == 3))
    tone = np.sin(2 * np.pi * (30000.0 if rate > 64000 else 440.0) / rate * t) * (hop > 4)
    left = g1 * lvl + 3000 * tone
    right = np.where(hop % 2 == 0, 0.8 * g1 + 0.2 * g2, 0.1 * g2) * lvl + 2000 * tone
    pcm = np.clip(np.rint(np.stack([left, right])), -32767, 32767).astype(np.int16)
    for p in burst_at:
        pcm[:, p:p + 128] = np.clip(g.normal(0, 0.5 * 32767, (2, 128)), -32767, 32767).astype(np.int16)
    return pcm


CASES = {
    "s32": (32000, wav_content(21, 10 * 1024 - 200, 32000, [4200])),      # long / transition / short blocks at 32 kHz
    # the degenerate all-short schedule.  The file ends in three silent hops: a stream whose last hop is coded short
    # cannot be written by the reference at all (Close() frames a long block around it and raises in MDCT)
    "s96": (96000, wav_content(22, 10 * 1024, 96000, [])),
}
CASES["s96"][1][:, 7 * 1024:] = 0
CASES["s32"][1][:, 8 * 1024:] = 0
out = {}
cwd = os.getcwd()
for name, (rate, pcm) in CASES.items():
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open("in.wav", "wb") as f:
                f.write(MO.wav_bytes(pcm, rate))
            H.load_file_layer(REF)
            H.write_huffman_files("./training_data/", HT.TABLES, HT.TABLE_ORDER)
            err = H.run_pacfile_main("in.wav", REF)
            if err is not None:
                raise err
            pac = np.frombuffer(open("in.pac", "rb").read(), dtype=np.uint8)
            w = open("in_decoded.wav", "rb").read()
            dec = np.frombuffer(w[44:], dtype="<i2").reshape(-1, 2).T.astype(np.int16)
        finally:
            os.chdir(cwd)
    out[name + "_pcm"], out[name + "_rate"], out[name + "_pac"], out[name + "_decoded"] = pcm, np.array(rate), pac, dec
# mono, 96 kHz, through the mono harness (WriteDataBlock for JointWriteDataBlock)
pcm = np.clip(np.rint(np.random.default_rng(23).normal(0, 0.05 * 32767, 7 * 1024 - 100)), -32767, 32767).astype(np.int16)[None]
pcm[:, 4 * 1024:] = 0                   # (ends long, as above)
with tempfile.TemporaryDirectory() as tmp:
    os.chdir(tmp)
    try:
        with open("in.wav", "wb") as f:
            f.write(MO.wav_bytes(pcm, 96000))
        H.load_file_layer(REF)
        H.write_huffman_files("./training_data/", HT.TABLES, HT.TABLE_ORDER)
        P = GM.load_pacfile_module(REF)
        GM.encode_mono_wav(P, sys.modules["pcmfile"], "in.wav", "in.pac")
        pac = np.frombuffer(open("in.pac", "rb").read(), dtype=np.uint8)
    finally:
        os.chdir(cwd)
out["m96_pcm"], out["m96_rate"], out["m96_pac"] = pcm, np.array(96000), pac
out["cases"] = np.array(sorted(CASES))
np.savez_compressed(os.path.join(HERE, "ref_pac_rates.npz"), **out)
for f in ("ref_rates", "ref_rates_smr", "ref_pac_rates"):
    print(f, os.path.getsize(os.path.join(HERE, f + ".npz")) // 1024, "KiB")
