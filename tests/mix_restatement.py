"""
The mid (L + R) / 2 of a stereo `.pac` file as mrc_pac_store_decode_window_mix defines it -- on the MDCT lines, before the
inverse transform -- restated in NumPy from the oracle's own functions, and the files the mix tests run on
(tests/test_store_mix_cpu.py, tests/test_gpu_store_mix.py).  A plain module.

With l1, l2 the two streams' dequantised lines of a joint block, each divided by its overall scale level, line k of the mid
is l1 where the band's M/S switch is set (the first stream is the mid; the side stream is not looked at) and
0.5 * (l1 + l2) where it is not; the last block of a stereo file is not joint: 0.5 * (x0 + x1) of its two channels' lines.
One IMDCT, window and overlap-add per block follow (tests/reduced_restatement.synthesise), at 1 / D of the rate like there.
The inverse transform being linear, the result is 0.5 * (ref[0] + ref[1]) of reduced_restatement.decode up to rounding:
((l1 + l2) + (l1 - l2)) / 2 against l1.
"""
import numpy as np

import reduced_restatement as RR
import settings_kit as SK
from oracle import codec as ocodec, decode as odec, pacfile as opac

KIT_SIDS = ("B", "C", "D", "K")
DIVISORS = (1, 2, 4)


def mid_blocks(buf, n_short, blksw_bits):
    """a stereo file -> (cp, [dict(start, a, b, joint, lines (the mid's, (a + b) / 2), ms (the switches or None))])"""
    cp, off = odec.read_header(buf, n_short, blksw_bits)
    if cp.nChannels != 2:
        raise ValueError("the mid of a stereo file was asked of a file of %d channels" % cp.nChannels)
    chunks = odec.split_chunks(buf, off)
    if len(chunks) % 2:
        raise ValueError("chunk count is not a multiple of the channel count")
    n, out, start = len(chunks) // 2, [], 0
    for blk in range(n):
        joint = blk < n - 1
        if joint:
            p = odec.parse_joint_block(chunks[2 * blk], chunks[2 * blk + 1], cp)
            lvl = [1. * (1 << int(s)) for s in p["overallScale"]]                    # L, R, M, S
            l1 = odec._dequantise_lines(p["scaleFactor"][0], p["bitAlloc"][0], p["mantissa"][0], cp)
            l2 = odec._dequantise_lines(p["scaleFactor"][1], p["bitAlloc"][1], p["mantissa"][1], cp)
            lines = np.zeros_like(l1)
            for iBand in range(cp.sfBands.nBands):
                lo, hi = cp.sfBands.lowerLine[iBand], cp.sfBands.upperLine[iBand] + 1
                if p["ms_switch"][iBand] == 1:
                    lines[lo:hi] = l1[lo:hi] / lvl[2]
                else:
                    lines[lo:hi] = 0.5 * (l1[lo:hi] / lvl[0] + l2[lo:hi] / lvl[1])
            ms = np.array(p["ms_switch"])
        else:
            x = []
            for ch in range(2):
                p = odec.parse_block(chunks[2 * blk + ch], cp)
                x.append(odec._dequantise_lines(p["scaleFactor"], p["bitAlloc"], p["mantissa"], cp) / (1. * (1 << p["overallScale"])))
            lines, ms = 0.5 * (x[0] + x[1]), None
        out.append(dict(start=start, a=int(cp.a), b=int(cp.b), joint=joint, lines=lines, ms=ms))
        start += int(cp.a)
    return cp, out


def mid_decode(buf, n_short, blksw_bits, D):
    """-> float64 [samples / D], the MDCT's delay kept as reduced_restatement.decode keeps it"""
    cp, blks = mid_blocks(buf, n_short, blksw_bits)
    total = blks[-1]["start"] + blks[-1]["a"] + blks[-1]["b"]
    plane = np.zeros(total // D)
    for k in blks:
        at, n = k["start"] // D, (k["a"] + k["b"]) // D
        plane[at:at + n] += RR.synthesise(k["lines"], k["a"], k["b"], D)
    return plane


# ------------------------------------------------------------------ the files
DEFAULT_SEED = 5


def default_stereo_file(seed=DEFAULT_SEED, L=1024, S=128, rate=48000):
    """the default-setting five-hop stereo file of the reduced-rate tests: (L,L), (L,L), (L,S), (S,S).., (S,L), (L,L) and
    Close()'s block from oracle.pacfile.encode_stereo_stream; a tone common to both channels (M/S bands) over independent
    noise (L/R bands)"""
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


def one_block(buf, n_short, blksw_bits):
    """the file's header and its last block alone (a stereo file: the two non-joint chunks Close() wrote, and nothing else)"""
    cp, off = odec.read_header(buf, n_short, blksw_bits)
    last = off
    for _ in range(len(odec.split_chunks(buf, off)) - cp.nChannels):            # a chunk: its byte count in 4 bytes, its bytes
        last += 4 + int.from_bytes(buf[last:last + 4], "little")
    return buf[:off] + buf[last:]


def one_block_stereo_file(sid):
    """a ONE-BLOCK STEREO file of a kit setting: the header and Close()'s two non-joint chunks of the oracle's file of the
    setting's first, loud hop (the zero prior hop, then tone and independent noise: the two channels differ audibly, which
    the quiet end of the kit's five-hop stream does not promise)"""
    L, S = SK.lengths(sid)
    buf = opac.encode_stereo_stream(SK.to_float(SK.stream(sid)[:, :2 * L]), [(0, L, L)], SK.coding_params(sid, 2), huffman=True)
    return one_block(buf, S, SK.blksw(sid))


_FILES = {}


def files(sid):
    """the mix tests' files of a setting (a KIT_SIDS letter or "default"), built once:
    -> dict(L, S, blksw, files [bytes], nch [per file], full [per file: holds every shape])
    kit setting: stereo Huffman, stereo raw, mono, one-block mono, ONE-BLOCK STEREO; default: the five-hop stereo file."""
    if sid not in _FILES:
        if sid == "default":
            L, S, blksw = 1024, 128, (1, 1)
            bufs, nch, full = [default_stereo_file()], [2], [True]
        else:
            (L, S), blksw = SK.lengths(sid), SK.blksw(sid)
            stereo, mono = SK.oracle_file(sid, 2, True)["data"], SK.oracle_file(sid, 1, True)["data"]
            bufs = [stereo, SK.oracle_file(sid, 2, False)["data"], mono, one_block(mono, S, blksw), one_block_stereo_file(sid)]
            nch, full = [2, 2, 1, 1, 2], [True, True, True, False, False]
        _FILES[sid] = dict(L=L, S=S, blksw=blksw, files=bufs, nch=nch, full=full)
    return _FILES[sid]
