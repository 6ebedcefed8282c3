#!/usr/bin/env python3
"""
Mono file-level golden data from the reference's OWN file layer.  The reference's command line only writes stereo
files (its loop hard-codes JointWriteDataBlock; the WriteDataBlock call is left commented out, pacfileThem.py:1218), but
its library encodes any channel count.  This generator loads pacfileThem.py as a MODULE through tests/golden/py2harness.py
(the same uniform Python-2 pass, the script's driver not run) and drives it as the command line does, with
WriteDataBlock in place of JointWriteDataBlock:

    PCMFile.OpenForReading / JointReadDataBlock       pcmfile.py (the CLI's reader, any channel count)
    the CLI's codingParams                            pacfileThem.py:1105-1131
    PACFile.OpenForWriting                            header with nChannels = 1
    TransientDetector + one hop of look-ahead         pacfileThem.py:1025-1056, 1159-1214
    PACFile.WriteDataBlock per block                  pacfileThem.py:622-790
    PACFile.Close                                     pacfileThem.py:973-984 (WriteDataBlock reads only data[0])

on synthetic 16-bit mono WAV files.  Recorded, as data:

    tests/golden/ref_pac_mono.npz   <case>_pcm      int16 [1][n]   the WAV's samples
                                    <case>_rate     sample rate
                                    <case>_pac      uint8 []       the .pac file, Huffman tables present
                                    <case>_pac_raw  uint8 []       the same with every block raw (EncodeNoHuff, id 15)

The Huffman files under ./training_data are written by the harness from this repo's table data, as for ref_pac.npz.
Raw files: the reference's WriteDataBlock calls self.Encode, which prices the Huffman tables whenever it finds them;
with no ./training_data it finds none and writes every block raw, which is what EncodeNoHuff writes.
"""
import ast
import builtins
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
from oracle import transient as otr, codec as ocodec   # noqa: E402   (only to ASSERT the cases contain short blocks)
import mono_oracle as MO                         # noqa: E402   (WAV bytes, the float stream)


def load_pacfile_module(ref_dir):
    """pacfileThem.py executed as a module named `pacfileThem` (its `__main__` driver does not run), with the harness's
    pass and namespace helpers exactly as run_pacfile_main applies them to the script."""
    H.load_file_layer(ref_dir)
    path = os.path.join(ref_dir, "pacfileThem.py")
    with builtins.open(path, encoding="utf-8-sig") as f:
        text = H._print_fixed(f.read(), "pacfileThem")
    tree = H._Pass().visit(ast.parse(text, filename=path))
    ast.fix_missing_locations(tree)

    class _Globals(dict):
        def __setitem__(self, k, v):
            if k == "np":
                v = H._Np()
            elif k == "range":
                v = H.py2range
            elif k in ("pack", "unpack", "calcsize"):
                v = H._struct_helpers()[k]
            elif k == "open":
                v = H._open_binary
            dict.__setitem__(self, k, v)

    ns = _Globals(__name__="pacfileThem", __file__=path, __py2div__=H.py2div, __py2idiv__=H.py2idiv,
                  __py2idx__=H.py2idx, range=H.py2range, xrange=H.py2range)
    exec(compile(tree, path, "exec"), ns)
    mod = types.SimpleNamespace(**ns)
    return mod


def encode_mono_wav(P, pcm_mod, wav_path, pac_path):
    """The reference CLI's encode direction with WriteDataBlock for JointWriteDataBlock."""
    inFile = pcm_mod.PCMFile(wav_path)
    outFile = P.PACFile(pac_path)
    cp = inFile.OpenForReading()
    assert cp.nChannels == 1
    cp.nMDCTLines = 1024
    cp.nScaleBits = 4
    cp.nMantSizeBits = 4
    cp.targetBitsPerSample = 2.86
    cp.nSamplesPerBlock = cp.nMDCTLines
    cp.bitReservoir = 0
    cp.nSamplesShort = 128
    cp.a = cp.nMDCTLines
    cp.b = cp.nMDCTLines
    cp.blkswBitA = 1
    cp.blkswBitB = 1
    outFile.OpenForWriting(cp)
    b, a = P.signal.cheby2(20, 40, 9000. / cp.sampleRate, 'high')
    sos = P.signal.tf2sos(b, a)
    nSub = cp.nSamplesPerBlock // cp.nSamplesShort
    cp.P = np.zeros((cp.nChannels, 1 + nSub))
    T = np.array([0.1, 0.075])
    blocky = 0
    mem = None
    while True:
        data = inFile.JointReadDataBlock(cp, blocky)
        if not data:
            break
        data = np.vstack(data)
        blksw = P.TransientDetector(data, cp, sos, T)
        if mem is None:                                  # one hop of look-ahead
            mem, memSw = data, blksw
            continue
        if np.sum(memSw) > 1 or any(blksw == 1):
            for i in range(nSub):
                cp.b = cp.nSamplesShort
                outFile.WriteDataBlock(mem[:, cp.b * i:cp.b * (i + 1)], cp, blocky)
                cp.a = cp.b
                blocky += 1
        else:
            cp.b = cp.nSamplesPerBlock
            outFile.WriteDataBlock(mem, cp, blocky)
            cp.a = cp.b
            blocky += 1
        mem, memSw = data, blksw
    inFile.Close(cp)
    outFile.Close(cp)
    return blocky


def content(seed, n, kind, burst_at=()):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    hop = t // 1024
    if kind == "noise":
        lvl = 10.0 ** (-1.5 * (hop % 5 == 3)) * 10.0 ** (-2.2 * (hop % 7 == 5))
        x = rng.normal(0, 0.1 * 32767, n) * lvl
    elif kind == "tone":
        x = 9000 * np.sin(2 * np.pi * 440.0 / 48000 * t) + 800 * np.sin(2 * np.pi * 1500.0 / 48000 * t)
    else:                                                # near-silence: a few codes of dither
        x = rng.normal(0, 2.0, n)
    pcm = np.clip(np.rint(x), -32767, 32767).astype(np.int16)[None, :]
    for p in burst_at:
        pcm[0, p:p + 128] = np.clip(rng.normal(0, 0.5 * 32767, 128), -32767, 32767).astype(np.int16)
    return pcm


CASES = {
    # noise with bursts, ragged length: long / transition / short blocks
    "noise48": (48000, content(11, 14 * 1024 - 300, "noise", [6200, 9000])),
    # a tone at 44.1 kHz (its band tables), length an exact multiple of the block size (the header's padding rule)
    "tone44": (44100, content(12, 12 * 1024, "tone")),
    # near-silence
    "quiet48": (48000, content(13, 10 * 1024 + 17, "quiet")),
    # bursts at 44.1 kHz, a multiple of 1024 samples, full-scale negative code
    "burst44": (44100, content(14, 11 * 1024, "noise", [3100, 4500])),
}
CASES["burst44"][1][0, 100] = -32768

if __name__ == "__main__":
    out = {}
    cwd = os.getcwd()
    for name, (rate, pcm) in CASES.items():
        for with_tables in (True, False):
            with tempfile.TemporaryDirectory() as tmp:
                os.chdir(tmp)
                try:
                    with open("in.wav", "wb") as f:
                        f.write(MO.wav_bytes(pcm, rate))
                    H.load_file_layer(REF)
                    if with_tables:
                        H.write_huffman_files("./training_data/", HT.TABLES, HT.TABLE_ORDER)
                    P = load_pacfile_module(REF)
                    encode_mono_wav(P, sys.modules["pcmfile"], "in.wav", "in.pac")
                    pac = np.frombuffer(open("in.pac", "rb").read(), dtype=np.uint8)
                finally:
                    os.chdir(cwd)
            out[name + ("_pac" if with_tables else "_pac_raw")] = pac
        out[name + "_pcm"], out[name + "_rate"] = pcm, np.array(rate)
        cp = ocodec.default_params(sampleRate=rate, nChannels=1)
        shapes = otr.block_shapes(MO.stream_of(pcm[0]), cp)
        print(name, "blocks", len(shapes), "short", sum(b == 128 for (_o, _a, b) in shapes), "bytes", out[name + "_pac"].size,
              out[name + "_pac_raw"].size)
        if name.startswith(("noise", "burst")):
            assert any(b == 128 for (_o, _a, b) in shapes), "case %s has no short blocks" % name
        if name != "quiet48":
            assert not np.array_equal(out[name + "_pac"], out[name + "_pac_raw"]), "no Huffman-coded block in " + name
    out["cases"] = np.array(sorted(CASES))
    np.savez_compressed(os.path.join(HERE, "ref_pac_mono.npz"), **out)
    print("ref_pac_mono.npz", os.path.getsize(os.path.join(HERE, "ref_pac_mono.npz")) // 1024, "KiB")
