"""
The constant-quality VBR rule of mrc_encode_vbr_nmr_pac restated in NumPy from the oracle (no tests
of its own).  Built on oracle.codec / oracle.quantize / oracle.decode for the transform, the quantiser and the file, and on
tests/nmr_restatement.py for the measure: X, T, mask_j, noise_j and r_j are mrc_pac_nmr's.

Per band the candidates n = 0, 2, 3, .., maxMantBits are tried in that order and the first with r_j(n) <= c is taken (a band
without lines takes 0; a band that never meets c keeps maxMantBits and is CAPPED).  In a joint block an L/R band is first-fit
per coded stream against its own channel; an M/S band starts at (0, 0) and, while max(r_L, r_R) > c, raises (0 -> 2, else
+ 1) the stream whose own error energy sum (x - x^)^2 (overall scale removed) is larger -- a tie: stream 0 -- or the other
one when that stream is at maxMantBits; both there: capped, counted once.

The rule itself is walk_mono / walk_joint, on planes: block_mono / block_joint hand them the planes of audio, block_crafted
planes of the caller's making (tests/vbr_cases.py), as the stage entries mrc_dev_vbr_alloc / _profile take them.  A walk with
c = None stops nowhere: vbr_profile_kernel's.

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


def _sum(v):
    """v[0] + v[1] + .. in line order (np.cumsum adds one term after the other; np.sum pairs them up)"""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


class _Band:
    """one coded stream's band: its scaled lines, the overall scale level, the quantiser at n bits"""

    def __init__(self, scaled, level, n_scale_bits):
        self.x, self.level, self.nsb = np.asarray(scaled, np.float64), float(level), n_scale_bits
        self.peak = np.max(np.abs(self.x)) if len(self.x) else 0.0
        self._dec, self._err = {}, {}

    def decoded(self, n):
        """the band's decoded lines with the overall scale removed (zeros at n = 0)"""
        if n not in self._dec:
            if not n or not len(self.x):
                self._dec[n] = np.zeros(len(self.x))
            else:
                sf = ScaleFactor(self.peak, self.nsb, n)
                m = vMantissa(self.x, sf, self.nsb, n)
                self._dec[n] = odec.vDequantize(sf, m, self.nsb, n) / self.level
        return self._dec[n]

    def error(self, n):
        if n not in self._err:
            d = self.x / self.level - self.decoded(n)
            self._err[n] = _sum(d * d)                        # line order
        return self._err[n]


def _ratio(X, Xhat, mask):
    d = X - Xhat
    noise = _sum(4.0 * (d * d))                               # line order
    if math.isinf(mask):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(noise) / np.float64(mask))


def _masks(T, edges):
    with np.errstate(over="ignore"):
        line = 10.0 ** ((np.asarray(T, np.float64) - 96.0) / 10.0)
    return [_sum(line[edges[j]:edges[j + 1]]) for j in range(len(edges) - 1)]


def _fits(r, c):
    """c None: no ceiling -- the walk of vbr_profile_kernel, which no state stops"""
    return c is not None and r <= c


def _first_fit(band, X, mask, c, max_bits, st, trail):
    """-> (n, r at n, capped)"""
    if not len(band.x):
        return 0, math.nan, 0                              # (0 / 0 in the measure, too)
    r = math.nan
    for n in candidates(max_bits):
        r = _ratio(X, band.decoded(n), mask)
        st["edges"] += c is not None and _near(r, c)
        trail.append((n, r))
        if _fits(r, c):
            return n, r, 0
    return max_bits, r, 1


def _lines(seg, a, b):
    return MDCT(TransitionWindow(np.asarray(seg, np.float64), a, b), a, b)[:(a + b) // 2]


def _edges(sfb):
    return np.concatenate([[0], np.cumsum(sfb.nLines)]).astype(int)


def walk_mono(scaled, level, X, T, c, sfb, nsb, max_bits, st, bands=None):
    """The rule on one non-joint channel's planes: its scaled lines and overall scale level, the source analysis X and T,
    the linear ceiling c (None: none) -> (ba, r, trails, capped flag per band).  bands: the _Band objects of an earlier
    walk over the same planes (their quantiser results are kept), else None."""
    e = _edges(sfb)
    masks = _masks(T, e)
    if bands is None:
        bands = [_Band(scaled[e[j]:e[j + 1]], level, nsb) for j in range(sfb.nBands)]
    ba, rr, trails, caps = [], [], [], []
    for j in range(sfb.nBands):
        trail = []
        n, r, cap = _first_fit(bands[j], X[e[j]:e[j + 1]], masks[j], c, max_bits, st, trail)
        st["capped"] += cap
        ba.append(n); rr.append(r); trails.append(trail); caps.append(cap)
    return np.array(ba, int), np.array(rr), trails, np.array(caps, int), masks, bands


def block_mono(seg, cp, c, rate, st):
    """one non-joint channel: -> dict(ba, r, trail, os, scaled)"""
    sfb, nsb = cp.sfBands, cp.nScaleBits
    X, T = nmr.source_analysis(seg, cp.a, cp.b, rate)
    lines = _lines(seg, cp.a, cp.b)
    osc = ScaleFactor(np.max(np.abs(lines)), nsb)
    scaled = lines * (1 << osc)
    ba, rr, trails, _, _, _ = walk_mono(scaled, 1 << osc, X, T, c, sfb, nsb, codec._max_mant_bits(cp), st)
    return dict(ba=[ba], r=[rr], trail=[trails], os=[osc], scaled=[scaled], ms=None)


def walk_joint(lines, osc, ms, src, c, sfb, nsb, max_bits, st, bands=None):
    """The rule on a joint block's planes: lines [4] the SCALED L, R, M, S lines, osc [4] their overall scales, ms [nBands]
    the switch, src [2] = (X, T) of the left and the right source, c the linear ceiling (None: none) -> dict(ba [2][nb], r
    [2][nb], trail, caps [2][nb] (an M/S band's cap at stream 0), raised {band: the streams its M/S walk raised, in order},
    steps {band: per step that a raise or the cap follows, (e0, e1, the stream with the larger error, the stream taken
    or None where the band is capped)}, masks, bands)."""
    e = _edges(sfb)
    masks = [_masks(src[ch][1], e) for ch in range(2)]
    nb = sfb.nBands
    if bands is None:
        bands = [[_Band(lines[sig][e[j]:e[j + 1]], 1 << osc[sig], nsb) for j in range(nb)] for sig in range(4)]
    ba = np.zeros((2, nb), int)
    rr = np.zeros((2, nb))
    caps = np.zeros((2, nb), int)
    trails = [[[] for _ in range(nb)] for _ in range(2)]
    raised, steps = {}, {}
    for j in range(nb):
        lo, hi = e[j], e[j + 1]
        if ms[j] != 1:
            for s in range(2):
                n, r, cap = _first_fit(bands[s][j], src[s][0][lo:hi], masks[s][j], c, max_bits, st, trails[s][j])
                st["capped"] += cap
                ba[s, j], rr[s, j], caps[s, j] = n, r, cap
            continue
        pair = [bands[2][j], bands[3][j]]
        n = [0, 0]
        raised[j], steps[j] = [], []
        while True:
            d = [pair[s].decoded(n[s]) for s in range(2)]
            r = [_ratio(src[0][0][lo:hi], d[0] + d[1], masks[0][j]), _ratio(src[1][0][lo:hi], d[0] - d[1], masks[1][j])]
            trails[0][j].append((tuple(n), r[0], r[1]))
            if hi == lo:
                r = [math.nan, math.nan]
                break
            if c is not None:
                st["edges"] += _near(r[0], c) + _near(r[1], c)
            if _fits(r[0], c) and _fits(r[1], c):
                break
            err = [pair[s].error(n[s]) for s in range(2)]
            st["edges"] += err[0] != err[1] and _near(err[0], err[1])
            larger = pick = 1 if err[1] > err[0] else 0
            if n[pick] >= max_bits:
                pick ^= 1
            if n[pick] >= max_bits:
                st["capped"] += 1
                caps[0, j] = 1
                steps[j].append((err[0], err[1], larger, None))
                break
            steps[j].append((err[0], err[1], larger, pick))
            raised[j].append(pick)
            n[pick] = n[pick] + 1 if n[pick] else 2
        ba[:, j], rr[:, j] = n, r
    return dict(ba=ba, r=rr, trail=trails, caps=caps, raised=raised, steps=steps, masks=masks, bands=bands)


def block_joint(segL, segR, cp, c, rate, st):
    sfb, nsb = cp.sfBands, cp.nScaleBits
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
    w = walk_joint(lines, osc, ms, src, c, sfb, nsb, codec._max_mant_bits(cp), st)
    return dict(ba=[w["ba"][0], w["ba"][1]], r=[w["r"][0], w["r"][1]], trail=w["trail"], os=osc, scaled=lines, ms=ms)


def quantise_dense(pick, ba, sfb, nsb, half):
    """codec._quantise_stream with the mantissas on their lines (0 where a band has no bits) -> scale_factor [nb], mantissa
    [half].  A band table with bands without lines (192 kHz) is outside what _quantise_stream takes (the peak of no lines);
    its bands go through the same two calls one by one, the empty ones with peak 0."""
    e = _edges(sfb)
    mant = np.zeros(half, np.int64)
    if (np.asarray(sfb.nLines) > 0).all():
        sf, compact = codec._quantise_stream(pick, ba, sfb, nsb, half)
        i = 0
        for j in range(sfb.nBands):
            if ba[j]:
                mant[e[j]:e[j + 1]] = compact[i:i + e[j + 1] - e[j]]
                i += e[j + 1] - e[j]
        return np.asarray(sf, np.int64), mant
    sf = np.zeros(sfb.nBands, np.int64)
    for j in range(sfb.nBands):
        x = pick(j)[e[j]:e[j + 1]]
        sf[j] = ScaleFactor(np.max(np.abs(x)) if len(x) else 0.0, nsb, ba[j])
        if ba[j] and len(x):
            mant[e[j]:e[j + 1]] = vMantissa(x, sf[j], nsb, ba[j])
    return sf, mant


def block_crafted(lines, osc, ms, X, T, c, sfb, nsb, max_bits, profile=True):
    """The rule on caller-made planes, as mrc_dev_vbr_alloc / _profile take them: lines [nsig][half] phase A's UNSCALED lines
    (a joint block: L, R, M, S), osc [nsig], ms [nBands] (None: a non-joint block), X and T [ns][half] per output channel,
    c the linear ceiling -> dict: bit_alloc / scale_factor [ns][nb], mantissa [ns][half] (dense), ratio [ns][nb] at the
    stopping states, capped and edges (counts of the block; edges: of both walks), caps [ns][nb], trail (the states tried with their ratios),
    raised / steps (M/S bands, walk_joint), masks [ns][nb], and with `profile` the walk without a ceiling under
    "profile" (trail, raised and steps of every state of every band)."""
    joint = ms is not None
    half = len(lines[0])
    scaled = [np.ldexp(np.asarray(lines[i], np.float64), int(osc[i])) for i in range(len(lines))]
    st, pst = dict(capped=0, edges=0), dict(capped=0, edges=0)   # pst: the walk without a ceiling (its error energies)
    out = {}
    if not joint:
        prof = None
        bands = None
        if profile:
            _, _, ptrail, _, _, bands = walk_mono(scaled[0], 1 << int(osc[0]), X[0], T[0], None, sfb, nsb, max_bits, pst)
            prof = dict(trail=[ptrail], raised={}, steps={})
        ba, rr, trails, caps, masks, _ = walk_mono(scaled[0], 1 << int(osc[0]), X[0], T[0], c, sfb, nsb, max_bits, st, bands)
        ba, rr, caps, masks, trails = ba[None], rr[None], caps[None], [masks], [trails]
        raised, steps = {}, {}
        pick = [lambda j: scaled[0]]
    else:
        src = [(X[0], T[0]), (X[1], T[1])]
        prof = None
        bands = None
        if profile:
            prof = walk_joint(scaled, osc, ms, src, None, sfb, nsb, max_bits, pst)
            bands = prof["bands"]
        w = walk_joint(scaled, osc, ms, src, c, sfb, nsb, max_bits, st, bands)
        ba, rr, caps, masks, trails, raised, steps = w["ba"], w["r"], w["caps"], w["masks"], w["trail"], w["raised"], w["steps"]
        pick = [lambda j, s=s: scaled[2 + s] if ms[j] == 1 else scaled[s] for s in range(2)]
    q = [quantise_dense(pick[s], ba[s], sfb, nsb, half) for s in range(len(pick))]
    out.update(bit_alloc=np.asarray(ba), scale_factor=np.stack([v[0] for v in q]), mantissa=np.stack([v[1] for v in q]),
               ratio=np.asarray(rr), capped=st["capped"], edges=st["edges"] + pst["edges"], caps=np.asarray(caps), trail=trails,
               raised=raised, steps=steps, masks=np.asarray(masks, np.float64), profile=prof)
    return out


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
