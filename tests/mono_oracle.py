"""
The oracle's mono `.pac` writer, composed from oracle pieces: the reference CLI's encode loop (pacfileThem.py:1159-1214)
with WriteDataBlock (622-790) in place of JointWriteDataBlock, then Close() (973-984) -- one non-joint chunk per block,
codingParams.bitReservoir carried from block to block through codec.Encode's Huffman savings (codecThem.py:205-231).
Shared by tests/test_mono_golden.py (against the reference's own bytes) and tests/test_gpu_mono.py.
"""
import struct

import numpy as np

from oracle import codec, pacfile, transient


def read_wav_codes(wav):
    """16-bit PCM WAV bytes -> (rate, nCh, numSamples, int16 [nCh][n])."""
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    _, _, n_ch, rate, _, _, _ = struct.unpack("<LHHLLHH", wav[16:36])
    n = struct.unpack("<L", wav[40:44])[0] // (2 * n_ch)
    codes = np.frombuffer(wav[44:44 + 2 * n * n_ch], dtype="<i2").reshape(-1, n_ch).T.astype(np.int16)
    return rate, n_ch, n, codes


def wav_bytes(pcm, rate):
    pcm = np.atleast_2d(pcm)
    data = np.ascontiguousarray(pcm.T).astype("<i2").tobytes()
    nch = pcm.shape[0]
    return (b"RIFF" + struct.pack("<L", 36 + len(data)) + b"WAVE" + b"fmt " +
            struct.pack("<LHHLLHH", 16, 1, nch, rate, rate * nch * 2, nch * 2, 16) + b"data" +
            struct.pack("<L", len(data)) + data)


def to_float(codes):
    """pcmfile.py:91-100: int16 code c -> sign(c) 2|c| / 65535 (-32768 -> 0)."""
    c = np.asarray(codes, dtype=np.float64)
    mag = np.abs(c)
    return np.where(mag >= 32768, 0.0, np.sign(c) * 2.0 * mag / 65535)


def stream_of(codes, hop=1024):
    """the WAV's codes [n] -> the float stream [1][(nHops + 1) * hop] the encode loop reads: zero prior hop, last hop
    zero padded."""
    codes = np.asarray(codes).reshape(-1)
    n_hops = -(-len(codes) // hop)
    x = np.zeros(n_hops * hop)
    x[:len(codes)] = to_float(codes)
    return np.concatenate([np.zeros(hop), x])[None, :]


def encode_mono_stream(stream, shapes, cp=None, huffman=True, num_samples=None, trace=None):
    """stream [1][samples] starting with the zero prior hop, shapes [(offset, a, b)] ending with a long block -> .pac bytes.
    trace (a list) receives codingParams.bitReservoir after every item (Close()'s included)."""
    cp = cp or codec.default_params(nChannels=1)
    cp.bitReservoir = 0 if getattr(cp, "bitReservoir", None) is None else cp.bitReservoir
    x = np.asarray(stream, dtype=np.float64).reshape(-1)
    L = cp.nMDCTLines
    if shapes[-1][2] != L:
        raise ValueError("the stream must end with a long block")
    out = pacfile.file_header(cp, sum(b for (_, _, b) in shapes) if num_samples is None else num_samples)
    enc = codec.Encode if huffman else codec.EncodeNoHuff
    blocks = [(a, b, x[off:off + a + b].copy()) for (off, a, b) in shapes]
    off, a, b = shapes[-1]
    blocks.append((L, L, np.concatenate([x[off + a:off + a + b], np.zeros(L)])))     # Close(): last hop + zeros
    for (a, b, blk) in blocks:
        cp.a, cp.b = a, b
        cp.sfBands = codec.bands_for_block(a, b, L, cp.sampleRate)
        r = enc([blk], cp)
        out += pacfile.pack_block(r[0], r[1], r[2], r[3], r[4], cp)
        if trace is not None:
            trace.append(int(cp.bitReservoir))
    return out


def encode_wav_mono(wav, huffman=True):
    """The whole mono encode loop on WAV bytes: ingest, the detector with one hop of look-ahead on the one channel,
    blocks, Close()."""
    rate, n_ch, n, codes = read_wav_codes(wav)
    assert n_ch == 1
    cp = codec.default_params(sampleRate=rate, nChannels=1)
    stream = stream_of(codes[0], cp.nMDCTLines)
    shapes = transient.block_shapes(stream, cp)
    cp.bitReservoir = 0
    return encode_mono_stream(stream, shapes, cp, huffman, num_samples=n)
