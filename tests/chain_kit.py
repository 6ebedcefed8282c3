"""
What the tests of the chained encodes share (test_gpu_ladder / _nmr / _mono / _target_nmr / _vbr / _vbr_size and their
*_cpu.py companions): a cache of handles, the signal generators, the stream and WAV plumbing, and the check of the ctypes
binding against include/mrc_hip.h.

The seeds the GPU tests pass to the generators were picked so that the NumPy restatements meet no edge candidate; a change
to what a generator returns for given arguments changes what those tests run on.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 1024
_HANDLES = {}


# ------------------------------------------------------------------ handles
def handle(exact=False, rate=48000, **cfg):
    """a handle on device 0 at sample rate `rate` (cfg: further arguments of Handle), with MRC_OPT_EXACT_SPREAD if `exact`;
    kept until close_handles()"""
    from mrcaudiocodec_amd import Handle
    key = (exact, int(rate), tuple(sorted(cfg.items())))
    if key not in _HANDLES:
        _HANDLES[key] = Handle(sample_rate=int(rate), device_id=0, **cfg)
        if exact:
            _HANDLES[key].set_option(1, 1)
    return _HANDLES[key]


def close_handles():
    for hd in _HANDLES.values():
        hd.close()
    _HANDLES.clear()


@pytest.fixture(scope="module", autouse=True)
def handles_closed_after_module():
    """imported by a test module: the handles it took are closed when its last test is done"""
    yield
    close_handles()


# ------------------------------------------------------------------ signals
def to_pcm(x):
    pcm = np.clip(np.rint(np.atleast_2d(x) * 32767.5), -32767, 32767).astype(np.int16)
    pcm[:, :HOP] = 0
    return pcm


def clicks(hops, seed, mono, period, fs=48000):
    """config C4 content -- noise floor + bursts every `period`-th hop (synth.c4_transients, a seed per channel) -- and a tone
    common to the channels, so that M/S bands occur beside L/R bands: int16 [nCh][(hops + 1) * HOP]"""
    from mrcaudiocodec_amd import synth
    chans = [synth.c4_transients(hops, seed=seed + c, period=period)[0] for c in range(1 if mono else 2)]
    tone = synth.c1_sine(hops, freq=440.0 + seed, amp=0.1, fs=fs)[:len(chans[0])]
    return to_pcm(np.stack(chans) + tone)


def noise(hops, seed, fs):
    from mrcaudiocodec_amd import synth
    return to_pcm(np.stack([synth.c2_noise(hops, seed=seed + c, sigma=0.05) for c in range(2)]) +
                  synth.c1_sine(hops, freq=3000.0, amp=0.2, fs=fs))


def shapes_to_last_long(h, pcm):
    """the detector's block shapes [n][3] up to the last long block (Close() needs one)"""
    from mrcaudiocodec_amd import transient
    shapes = transient.block_shape_array(h, pcm)
    last = np.nonzero(shapes[:, 2] == HOP)[0][-1]
    return shapes[:last + 1]


def long_short_run(period):
    """one mono stream whose (S,S) blocks do not fit one batch of the source analysis (16384 blocks of one shape):
    (L,S), 16384 + 5 x (S,S), (S,L) -- int16 [1][n], its shapes, its sample count"""
    S, n_ss = 128, 16384 + 5
    a = np.array([HOP] + [S] * (n_ss + 1), np.int64)
    b = np.array([S] * (n_ss + 1) + [HOP], np.int64)
    off = np.concatenate([[0], np.cumsum(a)[:-1]])
    shapes = np.stack([off, a, b], axis=1)
    hops = -(-int(off[-1] + a[-1] + b[-1]) // HOP)
    return clicks(hops, 11, True, period), shapes, int(b.sum())


# ------------------------------------------------------------------ plumbing
def rows(pcms):
    """int16 [nCh][n_s] streams of one channel count, padded to one stride -> (left [nS][stride], right or None, stride)"""
    stride = max(p.shape[1] for p in pcms)
    mono = pcms[0].shape[0] == 1
    left = np.zeros((len(pcms), stride), np.int16)
    right = None if mono else np.zeros((len(pcms), stride), np.int16)
    for i, p in enumerate(pcms):
        left[i, :p.shape[1]] = p[0]
        if not mono:
            right[i, :p.shape[1]] = p[1]
    return left, right, stride


def write_wav(path, pcm, rate=48000):
    """int16 [nCh][n] as a 16-bit PCM WAV file -> str(path)"""
    from mrcaudiocodec_amd import cli
    with open(str(path), "wb") as f:
        f.write(cli.wav_bytes(pcm, rate))
    return str(path)


# ------------------------------------------------------------------ the binding against the header
_SCALAR = {"double": C.c_double, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t,
           "uint32_t": C.c_uint32}
_RETURN = dict(_SCALAR, **{"void": None, "const char*": C.c_char_p})


def header_text(comments=False):
    text = open(os.path.join(ROOT, "include", "mrc_hip.h")).read()
    return text if comments else re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_declarations():
    """every function include/mrc_hip.h declares: name -> (return type, [argument declarations]), white space squeezed"""
    found = re.findall(r"\b(const\s+char\s*\*|void|int|int64_t)\s+(mrc_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", header_text())
    squeeze = lambda t: " ".join(t.split())
    return {name: (squeeze(ret).replace(" *", "*"), [] if squeeze(args) == "void" else [squeeze(a) for a in args.split(",")])
            for ret, name, args in found}


def header_args(name):
    return header_declarations()[name][1]


def check_binding(names):
    """the ctypes prototype of each name against its declaration: the return type, the argument count, and per argument a
    pointer type for a `*`, else exactly the scalar's ctypes counterpart"""
    from mrcaudiocodec_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    decls = header_declarations()
    for name in names:
        assert hasattr(raw, name) and name in _lib.EXPORTS and name in decls, name
        fn = getattr(_lib.lib, name)
        ret, args = decls[name]
        assert fn.restype is _RETURN[ret], (name, ret, fn.restype)
        assert len(fn.argtypes) == len(args), (name, len(fn.argtypes), len(args))
        for decl, typ in zip(args, fn.argtypes):
            if "*" in decl:
                assert typ is C.c_void_p or issubclass(typ, C._Pointer), (name, decl, typ)
            else:
                words = [w for w in decl.split() if w != "const"]
                assert len(words) == 2 and typ is _SCALAR.get(words[0]), (name, decl, typ)
