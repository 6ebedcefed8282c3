"""
CPU test of the portable chunk parser (mrcaudiocodec_amd/csrc/mrc_unpack.hpp), the code the device unpack kernel runs:
tests/unpack_check.cpp compiles it for the host -- with AddressSanitizer and UndefinedBehaviorSanitizer where g++ has
them -- and parses the corpus of tests/unpack_corpus.py in the layout of mrc_unpack_blocks.  Every accept / reject
decision and every integer must equal the host parser's (pacfile.unpack_blocks), the sanitizers must stay silent.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import unpack_corpus as UC
from mrcaudiocodec_amd import pacfile as ppac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _compile(tmp):
    src = os.path.join(ROOT, "tests", "unpack_check.cpp")
    inc = ["-I", os.path.join(ROOT, "mrcaudiocodec_amd", "csrc")]
    exe = os.path.join(tmp, "unpack_check")
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.path.join(tmp, "probe")] + SAN,
                           input=b"int main() { return 0; }\n", capture_output=True)
    flags = SAN if probe.returncode == 0 else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + inc + [src, "-o", exe])
    return exe, bool(flags)


def _write_input(path, cases):
    lut, esc = UC.decode_tables()
    with open(path, "wb") as f:
        f.write(lut.astype("<u2").tobytes())
        f.write(esc.astype("<i4").tobytes())
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            cfg = c["cfg"]
            f.write(struct.pack("<6i", cfg.n_scale_bits, cfg.n_mant_size_bits, cfg.blksw_bits_a, cfg.blksw_bits_b,
                                cfg.n_short, cfg.n_mdct_lines))
            tabs = [ppac.band_table(cfg, a, b) for (a, b) in UC.SHAPES(cfg)]
            f.write(struct.pack("<4i", *[len(t) for t in tabs]))
            f.write(struct.pack("<4i", *[(a + b) // 2 for (a, b) in UC.SHAPES(cfg)]))
            for t in tabs:
                f.write(np.asarray(t, "<i4").tobytes())
            offs = np.asarray(c["offsets"], "<i8")
            f.write(struct.pack("<3iq", len(offs) // c["nch"], c["nch"], int(c["joint"]), len(c["buf"])))
            f.write(c["buf"])
            f.write(offs.tobytes())


def _read_output(path, cases):
    raw = np.fromfile(path, dtype="<i4")
    pos, res = 0, []
    keys = ("a", "b", "huff_table", "overall_scale", "ms_switch", "scale_factor", "bit_alloc", "mantissa")
    for c in cases:
        status = int(raw[pos])
        pos += 1
        if status:
            res.append(status)
            continue
        n, nch, L = len(c["offsets"]) // c["nch"], c["nch"], c["cfg"].n_mdct_lines
        shapes = [(n,), (n,), (n, nch), (n, 4 if c["joint"] else nch), (n, 32), (n, nch, 32), (n, nch, 32), (n, nch, L)]
        got = {}
        for k, shp in zip(keys, shapes):
            size = int(np.prod(shp))
            got[k] = raw[pos:pos + size].reshape(shp)
            pos += size
        res.append(got)
    assert pos == raw.size
    return res


def _check(cases, tmp_path):
    exe, sanitized = _compile(str(tmp_path))
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    _write_input(src, cases)
    run = subprocess.run([exe, src, dst], capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-3000:]
    got = _read_output(dst, cases)
    n_acc = n_rej = 0
    for c, g in zip(cases, got):
        want = UC.host_parse(c)
        if want is None:
            assert not isinstance(g, dict), "%s: the host parser refuses, the portable parser accepts" % c["label"]
            n_rej += 1
            continue
        assert isinstance(g, dict), "%s: the host parser accepts, the portable parser refuses (status %d)" % (c["label"], g)
        for k, v in want.items():
            if k == "ms_switch" and not c["joint"]:
                continue                          # (mrc_unpack_blocks leaves it alone for independent channels)
            assert np.array_equal(g[k], v), "%s: %s differs" % (c["label"], k)
        n_acc += 1
    return n_acc, n_rej, sanitized


def test_portable_parser_equals_host_parser_on_corpus(tmp_path):
    bases = UC.base_cases()
    n_acc, n_rej, _ = _check(bases, tmp_path)
    assert n_rej == 0 and n_acc == len(bases) >= 144
    labels = " ".join(c["label"] for c in bases)
    for part in ("ref_a48_pac", "ref_b44_pac_raw", "switched_huff1", "mono_", "table3_", "jtable0_", "_m5_", "crafted_default_full_2ch/joint",
                 "crafted_default_main_2ch_huffman/flush", "crafted_E_one_line_1ch_huffman", "crafted_E_main_2ch/joint"):
        assert part in labels


def test_portable_parser_agrees_on_damaged_chunks(tmp_path):
    damaged = UC.corruptions(UC.base_cases(), n=2000)
    n_acc, n_rej, sanitized = _check(damaged, tmp_path)
    kinds = {c["label"].split(":")[1].split("@")[0] for c in damaged}
    assert kinds == {"flip", "table", "alloc", "short", "offset"}
    assert n_rej >= 500 and n_acc >= 100, (n_acc, n_rej)      # both outcomes well represented
    print("damaged chunk sets: %d accepted, %d refused by both parsers; sanitizers %s" %
          (n_acc, n_rej, "on" if sanitized else "not available"))
