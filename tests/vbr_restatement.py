"""
The constant-quality VBR rule of mrc_encode_vbr_nmr_pac restated in NumPy from the oracle (no tests
of its own).  Built on oracle.codec / oracle.quantize / oracle.decode for the transform, the quantiser and the file, and on
tests/nmr_restatement.py for the measure: X, T, mask_j, noise_j and r_j are mrc_pac_nmr's.

Per band the candidates n = 0, 2, 3, .., maxMantBits are tried in that order and the first with r_j(n) <= c is taken (a band
without lines takes 0; a band that never meets c keeps maxMantBits and is CAPPED).  In a joint block an L/R band is first-fit
per coded stream against its own channel; an M/S band starts at (0, 0) and, while max(r_L, r_R) > c, raises (0 -> 2, else
+ 1) the stream whose own error energy sum (x - x^)^2 (overall scale removed) is larger -- a tie: stream 0 -- or the other
one when that stream is at maxMantBits; both there: capped, counted once.

EDGE candidates: evaluated candidates whose decision could flip with the last bits of the arithmetic -- |r / c - 1| < 1e-6
for a ratio that is compared with c, |e0 / e1 - 1| < 1e-6 for two unequal error energies that are compared.  A test
that wants exact equality with the device picks inputs for which encode(...)["edges"] == 0.
"""
import math

import numpy as np

from oracle import codec, decode as odec, pacfile as opac
from oracle.huffman_tables import RAW_TABLE_ID
from oracle.mdct import MDCT
from oracle.ms_stereo import MSSwitchSFBands
from oracle.quantize import ScaleFactor, vMantissa
from oracle.window import TransitionWindow

import nmr_restatement as nmr

EDGE = 1e-6


def ceiling_ratio(ceiling_db):
    """c as the library forms it: one pow on the host (+inf -> inf, -inf -> 0)"""
    if ceiling_db == math.inf:
        return math.inf
    if ceiling_db == -math.inf:
        return 0.0
    return math.pow(10.0, ceiling_db / 10.0)


def candidates(max_bits):
    return [0] + list(range(2, max_bits + 1))


def _near(a, b):
    if not (math.isfinite(a) and math.isfinite(b)) or b == 0.0:
        return False
    return abs(a / b - 1.0) < EDGE


class _Band:
    """one coded stream's band: its scaled lines, the overall scale level, the quantiser at n bits"""

    def __init__(self, scaled, level, n_scale_bits):
        self.x, self.level, self.nsb = np.asarray(scaled, np.float64), float(level), n_scale_bits
        self.peak = np.max(np.abs(self.x)) if len(self.x) else 0.0

    def decoded(self, n):
        """the band's decoded lines with the overall scale removed (zeros at n = 0)"""
        if not n or not len(self.x):
            return np.zeros(len(self.x))
        sf = ScaleFactor(self.peak, self.nsb, n)
        m = vMantissa(self.x, sf, self.nsb, n)
        return odec.vDequantize(sf, m, self.nsb, n) / self.level

    def error(self, n):
        d = self.x / self.level - self.decoded(n)
        e = 0.0
        for v in d * d:                                   # line order
            e += float(v)
        return e


def _ratio(X, Xhat, mask):
    d = X - Xhat
    noise = 0.0
    for v in 4.0 * (d * d):                               # line order
        noise += float(v)
    if math.isinf(mask):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(noise) / np.float64(mask))


def _masks(T, edges):
    with np.errstate(over="ignore"):
        line = 10.0 ** ((np.asarray(T, np.float64) - 96.0) / 10.0)
    out = []
    for j in range(len(edges) - 1):
        m = 0.0
        for v in line[edges[j]:edges[j + 1]]:
            m += float(v)
        out.append(m)
    return out


def _first_fit(band, X, mask, c, max_bits, st, trail):
    """-> (n, r at n, capped)"""
    if not len(band.x):
        return 0, math.nan, 0                              # (0 / 0 in the measure, too)
    r = math.nan
    for n in candidates(max_bits):
        r = _ratio(X, band.decoded(n), mask)
        st["edges"] += _near(r, c)
        trail.append((n, r))
        if r <= c:
            return n, r, 0
    return max_bits, r, 1


def _lines(seg, a, b):
    return MDCT(TransitionWindow(np.asarray(seg, np.float64), a, b), a, b)[:(a + b) // 2]


def _edges(sfb):
    return np.concatenate([[0], np.cumsum(sfb.nLines)]).astype(int)


def block_mono(seg, cp, c, rate, st):
    """one non-joint channel: -> dict(ba, r, trail, os, scaled)"""
    sfb, nsb = cp.sfBands, cp.nScaleBits
    max_bits = codec._max_mant_bits(cp)
    X, T = nmr.source_analysis(seg, cp.a, cp.b, rate)
    lines = _lines(seg, cp.a, cp.b)
    osc = ScaleFactor(np.max(np.abs(lines)), nsb)
    scaled = lines * (1 << osc)
    e = _edges(sfb)
    masks = _masks(T, e)
    ba, rr, trails = [], [], []
    for j in range(sfb.nBands):
        lo, hi = e[j], e[j + 1]
        trail = []
        n, r, cap = _first_fit(_Band(scaled[lo:hi], 1 << osc, nsb), X[lo:hi], masks[j], c, max_bits, st, trail)
        st["capped"] += cap
        ba.append(n); rr.append(r); trails.append(trail)
    return dict(ba=[np.array(ba, int)], r=[np.array(rr)], trail=[trails], os=[osc], scaled=[scaled], ms=None)


def block_joint(segL, segR, cp, c, rate, st):
    sfb, nsb = cp.sfBands, cp.nScaleBits
    max_bits = codec._max_mant_bits(cp)
    segL, segR = np.asarray(segL, np.float64), np.asarray(segR, np.float64)
    time = [segL, segR, (segL + segR) / 2.0, (segL - segR) / 2.0]
    lines = [_lines(x, cp.a, cp.b) for x in time]
    ms = np.asarray(MSSwitchSFBands(lines[0], lines[1], sfb), int)
    osc = []
    for X in lines:
        s = ScaleFactor(np.max(np.abs(X)), nsb)
        X *= (1 << s)
        osc.append(s)
    src = [nmr.source_analysis(x, cp.a, cp.b, rate) for x in (segL, segR)]
    e = _edges(sfb)
    masks = [_masks(src[ch][1], e) for ch in range(2)]
    ba = np.zeros((2, sfb.nBands), int)
    rr = np.zeros((2, sfb.nBands))
    trails = [[[] for _ in range(sfb.nBands)] for _ in range(2)]
    for j in range(sfb.nBands):
        lo, hi = e[j], e[j + 1]
        if ms[j] != 1:
            for s in range(2):
                band = _Band(lines[s][lo:hi], 1 << osc[s], nsb)
                n, r, cap = _first_fit(band, src[s][0][lo:hi], masks[s][j], c, max_bits, st, trails[s][j])
                st["capped"] += cap
                ba[s, j], rr[s, j] = n, r
            continue
        bands = [_Band(lines[2 + s][lo:hi], 1 << osc[2 + s], nsb) for s in range(2)]
        n = [0, 0]
        while True:
            d = [bands[s].decoded(n[s]) for s in range(2)]
            r = [_ratio(src[0][0][lo:hi], d[0] + d[1], masks[0][j]), _ratio(src[1][0][lo:hi], d[0] - d[1], masks[1][j])]
            trails[0][j].append((tuple(n), r[0], r[1]))
            if hi == lo:
                r = [math.nan, math.nan]
                break
            st["edges"] += _near(r[0], c) + _near(r[1], c)
            if r[0] <= c and r[1] <= c:
                break
            err = [bands[s].error(n[s]) for s in range(2)]
            st["edges"] += err[0] != err[1] and _near(err[0], err[1])
            pick = 1 if err[1] > err[0] else 0
            if n[pick] >= max_bits:
                pick ^= 1
            if n[pick] >= max_bits:
                st["capped"] += 1
                break
            n[pick] = n[pick] + 1 if n[pick] else 2
        ba[:, j], rr[:, j] = n, r
    return dict(ba=[ba[0], ba[1]], r=[rr[0], rr[1]], trail=trails, os=osc, scaled=lines, ms=ms)


def _huff(m, ba, cp, huffman):
    if not huffman:
        return RAW_TABLE_ID, m
    t, codes, _ = codec.calculateHuffmanGain(m, ba, cp)
    return t, codes


def encode(pcm, shapes, c, sample_rate=48000, huffman=True, num_samples=None, cp=None):
    """pcm int16 [nCh][n], every row starting with its zero prior hop; shapes [(offset, a, b)] ending in a long block; c the
    linear ceiling -> dict(data = the `.pac` bytes, capped, edges, blocks = [dict per block, Close()'s blocks (one per
    channel) last]).  cp: the oracle CodingParams of another codec setting (block lengths, field widths; its rate and
    channel count are used), else the defaults at sample_rate."""
    pcm = np.atleast_2d(pcm)
    nch = pcm.shape[0]
    x = nmr.pcm_to_float(pcm)
    if cp is None:
        cp = codec.default_params(sampleRate=sample_rate, nChannels=nch)
    sample_rate = cp.sampleRate
    assert cp.nChannels == nch
    L = cp.nMDCTLines
    shapes = [(int(o), int(a), int(b)) for (o, a, b) in shapes]
    assert shapes[-1][2] == L and shapes[0][1] == L
    st = dict(capped=0, edges=0)
    out = opac.file_header(cp, sum(b for (_, _, b) in shapes) if num_samples is None else int(num_samples))
    blocks = []
    half = lambda: (cp.a + cp.b) / 2.

    def one_channel_block(segs):
        sf, ba, mm, osc, tabs, infos = [], [], [], [], [], []
        for seg in segs:
            info = block_mono(seg, cp, c, sample_rate, st)
            s, m = codec._quantise_stream(lambda i: info["scaled"][0], info["ba"][0], cp.sfBands, cp.nScaleBits, half())
            t, m = _huff(m, info["ba"][0], cp, huffman)
            sf.append(s); ba.append(info["ba"][0]); mm.append(m); osc.append(info["os"][0]); tabs.append(t); infos.append(info)
        return opac.pack_block(sf, ba, mm, osc, tabs, cp), infos

    for (off, a, b) in shapes:
        cp.a, cp.b = a, b
        cp.sfBands = codec.bands_for_block(a, b, L, sample_rate)
        if nch == 1:
            data, infos = one_channel_block([x[0, off:off + a + b]])
            blocks.append(infos[0])
        else:
            info = block_joint(x[0, off:off + a + b], x[1, off:off + a + b], cp, c, sample_rate, st)
            sf, mm, tabs = [], [], []
            for s in range(2):
                pick = lambda i, s=s: info["scaled"][2 + s] if info["ms"][i] == 1 else info["scaled"][s]
                f, m = codec._quantise_stream(pick, info["ba"][s], cp.sfBands, cp.nScaleBits, half())
                t, m = _huff(m, info["ba"][s], cp, huffman)
                sf.append(f); mm.append(m); tabs.append(t)
            data = opac.pack_joint_block(sf, info["ba"], mm, info["os"], info["ms"], tabs, cp)
            blocks.append(info)
        out += data
    off, a, b = shapes[-1]
    cp.a = cp.b = L
    cp.sfBands = codec.bands_for_block(L, L, L, sample_rate)
    data, infos = one_channel_block([np.concatenate([x[ch, off + a:off + a + b], np.zeros(L)]) for ch in range(nch)])
    blocks.extend(infos)
    return dict(data=out + data, capped=st["capped"], edges=st["edges"], blocks=blocks, nch=nch)


def coded_bits(data, nch):
    """payload bits of a file: 8 x (its bytes - the header - 4 per chunk)"""
    cp, off = odec.read_header(data)
    chunks = odec.split_chunks(data, off)
    return 8 * (len(data) - off - 4 * len(chunks))


def source_of(pcm, shapes, hop=1024):
    """what mrc_pac_nmr measures a stream's file against: the row from the prior hop's end to the end of its last block"""
    o, a, b = (int(v) for v in shapes[-1])
    return np.ascontiguousarray(np.atleast_2d(pcm)[:, hop:o + a + b])
