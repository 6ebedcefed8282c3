"""
The frames of tests/test_gpu_smr_overflow.py and test_smr_overflow_cpu.py (and of tools/record_smr_overflow.py, which records
their fixture): long blocks (N = 2048) around the masker table's second round -- smr_kernel (csrc/mrc_smr_body.hpp) builds a
table entry per thread, 256 a round; wave 0 makes the entries of the maskers from 256 on in a round of its own.

One int16 stereo stream holds every source back to back, a zero hop in front of each: the left channel is the mono input, the
right one follows it by smr_content's "mix" relation.  FRAMES names the start of every frame of the tests in it:

  c2-<i>    frame i of BASELINE config C2 (synth.c2_noise, seed 1234; the benchmark's content): 255, 256, 257, 258 maskers
            (frames 13, 8, 3, 11: either side of the round's edge) and 273 (frame 205: the most among the first 400)
  comb      a second round of more than a wave's worth (> 320 maskers), more than the nodes take
  comb6     the same from partials spread over 6 dB
  step      slope nodes, contenders that fail the bound (chunks sent back to the sorted sweep)
  silence   a silent frame (no masker) and a half-silent one; sparse: an impulse pair -- lines on the SPL floor, < 32 maskers
  softtone  a soft tone over a low floor: nodes, few contenders
  lsb       an impulse pair of one least significant bit in silence: a few maskers, every one below the intensity at which an
            SPL reaches its -30 dB floor (the table entry's level sits on the floor)

STREAMED: nine consecutive frames of C2 (3 .. 11; 257, 256 and 258 maskers among them) for the hop-overlapped batches.
"""
import numpy as np

import smr_content as C

HOP = 1024
N = 2 * HOP
C2_HOPS = 207                                          # frames 0 .. 205
C2_FRAMES = (13, 8, 3, 11, 205)
C2_MASKERS = {13: 255, 8: 256, 3: 257, 11: 258, 205: 273}
CONTENT_FRAMES = (("comb", 4), ("comb6", 4), ("step", 4), ("silence", 1), ("silence", 2), ("sparse", 4), ("softtone", 4),
                  ("lsb", 0))
STREAM_FIRST, STREAM_COUNT = 3, 9

_cache = {}


def _c2_pair():
    from mrcaudiocodec_amd import synth
    left = np.concatenate([np.zeros(HOP), synth._gauss_pcm(1234, (C2_HOPS - 1) * HOP, 0.1)])
    other = np.concatenate([np.zeros(HOP), synth._gauss_pcm(5678, (C2_HOPS - 1) * HOP, 0.1)])
    return np.stack([left.astype(np.int16), C.RELATIONS["mix"](left, other)])


def _lsb_pair():
    left, other = np.zeros(3 * HOP), np.zeros(3 * HOP)
    left[[HOP + 300, HOP + 340]] = 1, -1
    other[[HOP + 517, HOP + 585]] = 2, -2
    return np.stack([left.astype(np.int16), C.RELATIONS["mix"](left, other)])


def stream():
    """-> (int16 [2][samples], {label: first sample of the frame}), read-only, made once"""
    if "stream" not in _cache:
        parts, frames, at = [_c2_pair()], {}, 0
        for i in C2_FRAMES:
            frames["c2-%d" % i] = i * HOP
        for i in range(STREAM_FIRST, STREAM_FIRST + STREAM_COUNT):
            frames.setdefault("c2-%d" % i, i * HOP)
        at = parts[0].shape[1]
        names = []
        for name, _ in CONTENT_FRAMES:
            if name not in names:
                names.append(name)
        base = {}
        for name in names:
            pcm = _lsb_pair() if name == "lsb" else C.stereo(name, "mix", N)
            base[name] = at
            parts.append(pcm)
            at += pcm.shape[1]
        for name, f in CONTENT_FRAMES:
            frames["%s-%d" % (name, f)] = base[name] + f * HOP
        pcm = np.ascontiguousarray(np.concatenate(parts, axis=1))
        assert pcm.dtype == np.int16
        pcm.setflags(write=False)
        _cache["stream"] = (pcm, frames)
    return _cache["stream"]


def labels():
    """the frames the batches by offsets[] draw from (the tests' inputs proper), in a fixed order"""
    return ["c2-%d" % i for i in C2_FRAMES] + ["%s-%d" % nf for nf in CONTENT_FRAMES]


def streamed_labels():
    return ["c2-%d" % i for i in range(STREAM_FIRST, STREAM_FIRST + STREAM_COUNT)]


def all_labels():
    out = labels()
    return out + [lab for lab in streamed_labels() if lab not in out]


def blocks(labs):
    """float64 (left, right) blocks [len(labs)][N] of the named frames, as the library maps int16 codes"""
    from mrcaudiocodec_amd import synth
    pcm, frames = stream()
    x = synth.pcm_to_float(pcm)
    return (np.stack([x[0, frames[lab]:frames[lab] + N] for lab in labs]),
            np.stack([x[1, frames[lab]:frames[lab] + N] for lab in labs]))


class Device:
    """The stream on the GPU (int16 codes and the float64 fractions they stand for) and the masking stage of the encode run on
    frames of it: Handle.dev_masking, i.e. the kernels an encode launches, with smr_kernel's own outputs handed out."""

    def __init__(self, torch, handle):
        from mrcaudiocodec_amd import synth
        self.torch, self.h = torch, handle
        pcm, self.frames = stream()
        self.pcm = {"int16": torch.from_numpy(pcm.copy()).to("cuda:0"),
                    "float64": torch.from_numpy(synth.pcm_to_float(pcm)).to("cuda:0")}
        self.nb = len(handle.bands(HOP, HOP))

    def masking(self, joint, dtype, n, first=0, stride=0, offsets=None):
        """n frames at first + stride i, or at offsets[] -> dict(smr, band_peak [n][nsig][nb] (NaN where the kernel writes
        nothing: joint units no band selects), ms_switch (joint)) as host arrays"""
        torch = self.torch
        nsig = 4 if joint else 1
        f64 = dict(dtype=torch.float64, device="cuda:0")
        i32 = dict(dtype=torch.int32, device="cuda:0")
        ch = self.pcm[dtype]
        left, right = ch[0, first:], (ch[1, first:] if joint else None)
        off = None if offsets is None else torch.tensor(np.asarray(offsets, dtype=np.int64), device="cuda:0")
        lines = torch.empty((n, nsig, HOP), **f64)
        scale = torch.empty((n, nsig), **i32)
        sw = torch.empty((n, self.nb), **i32) if joint else None
        smr = torch.full((n, nsig, self.nb), float("nan"), **f64)
        peak = torch.full((n, nsig, self.nb), float("nan"), **f64)
        self.h.dev_masking(HOP, HOP, n, left.data_ptr(), right.data_ptr() if joint else None, 1 if dtype == "int16" else 0,
                           stride, None if off is None else off.data_ptr(), lines.data_ptr(), scale.data_ptr(),
                           None if sw is None else sw.data_ptr(), smr.data_ptr(), peak.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = dict(smr=smr.cpu().numpy(), band_peak=peak.cpu().numpy(), overall_scale=scale.cpu().numpy())
        if joint:
            out["ms_switch"] = sw.cpu().numpy()
        return out

    def singles(self, joint, dtype, labs):
        """every named frame in a call of its own -> the arrays of masking(), a row per frame"""
        rows = [self.masking(joint, dtype, 1, offsets=[self.frames[lab]]) for lab in labs]
        return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}

    def sent_back(self, labs):
        """MRC_OPT_SENSITIVITY's count of node chunks sent back to the sorted sweep, per named frame (mono, int16)"""
        self.h.set_option(5, 1)
        try:
            out = []
            for lab in labs:
                self.h.sensitivity(reset=True)
                self.masking(False, "int16", 1, offsets=[self.frames[lab]])
                out.append(int(self.h.sensitivity(reset=True)["node_chunks_sent_back"]))
        finally:
            self.h.set_option(5, 0)
        return np.array(out, dtype=np.int64)
