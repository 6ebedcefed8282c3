"""
Seeded int16 contents for the tests of the masking kernels (tests/test_gpu_smr_contenders.py, test_smr_paths_cpu.py,
test_gpu_smr_paths.py): the mono makers, and stereo streams made of them with a relation between the channels, each with
the zero prior hop, cut into blocks of a shape (a, b).  A plain module; streams and blocks are made once per process and
handed out read-only.

What a content is for (asserted by the tests from the restatements, not from this text):
  noise     white noise, sigma 0.1 of full scale: slope nodes everywhere
  step      that noise with a 40 dB step down at 6 kHz: lines above the step live on distant loud maskers, their chunks are
            sent back from the nodes to the sorted sweep
  pink      noise at -3 dB per octave: the slope range of a unit is beyond the nodes' reach (whole-unit sorted sweep)
  softtone  997 Hz at -36 dB over a -60 dB floor; tone: the same at half of full scale
  varied    synth.c6_varied: levels that wander over 60 dB, tones that come and go, silence, clipping
  comb6     a partial on every second FFT bin of the block length, amplitudes spread over 6 dB: more maskers than the nodes take
  comb      the same at equal amplitudes: every second bin a strict peak, the capacity of the masker scans
  sparse    an impulse pair per block: fewer maskers than the nodes need
  silence   hops of digital silence and of noise
"""
import numpy as np

HOP = 1024
N_FRAMES = 8                                         # frames per content and shape in the path tests


def _noise(seed, n, sigma):
    g = np.random.default_rng(seed).normal(0.0, sigma * 32767, n)
    return np.clip(np.rint(g), -32767, 32767)


def content_noise(n_frames=9, seed=77):
    return np.concatenate([np.zeros(HOP), _noise(seed, n_frames * HOP, 0.1)]).astype(np.int16)


def _tone(amp, n_frames=9, seed=5):
    n = np.arange((n_frames + 1) * HOP)
    x = amp * 32767 * np.sin(2 * np.pi * 997.0 * n / 48000.0) + _noise(seed, len(n), 1e-3)
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


def content_tone(n_frames=9, seed=5):
    return _tone(0.5, n_frames, seed)


def content_softtone(n_frames=9, seed=5):
    return _tone(0.015, n_frames, seed)


def _gated(seed, on):
    x = _noise(seed, len(on) * HOP, 0.1)
    x[~np.repeat(np.array(on, dtype=bool), HOP)] = 0
    return x.astype(np.int16)


def content_silence(n_frames=9, seed=11):
    return _gated(seed, [1, 0, 0, 1, 0, 1, 1, 0, 0, 1][:n_frames + 1])


def content_step(n_frames=9, seed=21):
    n = (n_frames + 1) * HOP
    spec = np.fft.rfft(np.random.default_rng(seed).normal(0.0, 0.1 * 32767, n))
    spec[np.fft.rfftfreq(n, 1.0 / 48000.0) >= 6000.0] *= 0.01
    return np.clip(np.rint(np.fft.irfft(spec, n)), -32767, 32767).astype(np.int16)


def content_sparse(n_frames=9, at=(300, 340)):
    x = np.zeros((n_frames + 1) * HOP)
    x[HOP + at[0]::2 * HOP] = 20000                                # (every second hop: a block sees one pair)
    x[HOP + at[1]::2 * HOP] = -12000
    return x.astype(np.int16)


def content_pink(n_frames=9, seed=31):
    n = (n_frames + 1) * HOP
    spec = np.fft.rfft(np.random.default_rng(seed).normal(0.0, 1.0, n))
    spec[1:] /= np.sqrt(np.arange(1, len(spec)))                   # power ~ 1 / f
    spec[0] = 0
    x = np.fft.irfft(spec, n)
    return np.clip(np.rint(x / x.std() * 0.1 * 32767), -32767, 32767).astype(np.int16)


def content_varied(n_frames=9, seed=21):
    from mrcaudiocodec_amd import synth
    return np.rint(synth.c6_varied(n_frames, seed=seed) * 65535.0 / 2.0).astype(np.int16)      # (pcm_to_float, inverted)


def content_comb(N, n_frames=9, seed=41, spread_db=0.0):
    """a partial on every odd FFT bin of an N-sample block up to the last bin searched for peaks, random phases, amplitudes
    uniform in dB over spread_db; periodic in N, so every N-sample block holds whole periods of every partial"""
    rng = np.random.default_rng(seed)
    k = np.arange(1, N // 2 - 101, 2)
    amp = 10.0 ** (rng.uniform(-spread_db, 0.0, len(k)) / 20.0)
    spec = np.zeros(N // 2 + 1, dtype=complex)
    spec[k] = amp * np.exp(2j * np.pi * rng.random(len(k)))
    period = np.fft.irfft(spec, N)
    x = np.tile(period, ((n_frames + 1) * HOP + N - 1) // N)[:(n_frames + 1) * HOP]
    return np.clip(np.rint(x / x.std() * 0.1 * 32767), -32767, 32767).astype(np.int16)


# name -> maker(n_frames, seed, N); the second seed of a content is its first + 100
_MAKERS = dict(
    noise=lambda n, s, N: content_noise(n, 77 + s),
    step=lambda n, s, N: content_step(n, 21 + s),
    pink=lambda n, s, N: content_pink(n, 31 + s),
    softtone=lambda n, s, N: content_softtone(n, 5 + s),
    tone=lambda n, s, N: content_tone(n, 5 + s),
    varied=lambda n, s, N: content_varied(n, 21 + s),
    comb6=lambda n, s, N: content_comb(N, n, 43 + s, 6.0),
    comb=lambda n, s, N: content_comb(N, n, 41 + s, 0.0),
    sparse=lambda n, s, N: content_sparse(n, (300, 340) if s == 0 else (517, 585)),
    silence=lambda n, s, N: content_silence(n, 11 + s),
)
CONTENTS = tuple(_MAKERS)


def _requantise(x):
    return np.clip(np.rint(x), -32767, 32767).astype(np.int16)


# the right channel from the left one and the content's second seed
RELATIONS = dict(
    mix=lambda left, other: _requantise(0.6 * left + 0.4 * other),       # correlated: M/S wins where both are alike
    apart=lambda left, other: _requantise(0.25 * other),                 # unrelated and 12 dB down: L/R wins
    same=lambda left, other: _requantise(left),                          # S = 0: silent units among M/S
    neg=lambda left, other: _requantise(-1.0 * left),                    # M = 0
    rsilent=lambda left, other: _requantise(0.0 * left),                 # R = 0: a silent unit among L/R
)

_cache = {}


def stereo(name, relation, N, n_frames=N_FRAMES):
    """int16 [2][(n_frames + 1) HOP], the first hop zero in both channels (N: the block length, which only the combs use)"""
    key = (name, relation, N if name.startswith("comb") else 0, n_frames)
    if key not in _cache:
        left = _MAKERS[name](n_frames, 0, N).astype(np.float64)
        other = _MAKERS[name](n_frames, 100, N).astype(np.float64)
        pcm = np.stack([_requantise(left), RELATIONS[relation](left, other)])
        assert pcm.dtype == np.int16
        pcm[:, :HOP] = 0
        pcm.setflags(write=False)
        _cache[key] = pcm
    return _cache[key]


def starts_of(a, b, n_frames=N_FRAMES):
    """first sample of each block of shape (a, b): a hop apart (the long block: the hop-overlapped stream), the short block
    (N = 256) 128 apart from the end of the zero hop's last eighth on, so that its first block is half silent"""
    if a + b <= 256:
        return HOP - (a + b) // 2 + np.arange(n_frames) * ((a + b) // 2)
    return np.arange(n_frames) * HOP


def blocks(pcm, a, b, n_frames=N_FRAMES):
    """int16 [2][samples] -> float64 left and right blocks [n_frames][a + b], as the library maps int16 codes"""
    from mrcaudiocodec_amd import synth
    x = synth.pcm_to_float(pcm)
    st = starts_of(a, b, n_frames)
    return np.stack([x[0, s:s + a + b] for s in st]), np.stack([x[1, s:s + a + b] for s in st])


# ---- the corpus of the path tests: (content, relation) pairs, N_FRAMES blocks each, per block shape
# The "mix" makes M/S win nearly every band, so each content whose class of evaluation has to show among the L/R units too comes
# a second time with unrelated channels ("apart"); "same" puts the step and the impulse pair into the M signal and leaves S
# silent, "rsilent" leaves a silent unit among L/R.
PAIRS = (("noise", "mix"), ("step", "apart"), ("step", "same"), ("pink", "mix"), ("pink", "apart"), ("softtone", "neg"),
         ("tone", "rsilent"), ("varied", "mix"), ("varied", "apart"), ("comb6", "mix"), ("comb6", "apart"), ("comb", "mix"),
         ("comb", "apart"), ("sparse", "mix"), ("sparse", "same"), ("silence", "mix"))
LABELS = tuple("%s-%s" % p for p in PAIRS)


def corpus(a, b):
    """every pair's blocks of shape (a, b) -> dict(labels, pcm = {label: int16 [2][samples]}, starts, left, right
    (float64 [len(PAIRS) N_FRAMES][a + b], pair after pair), rows = {label: slice into left / right})"""
    key = ("corpus", a, b)
    if key not in _cache:
        pcm = {lab: stereo(name, rel, a + b) for lab, (name, rel) in zip(LABELS, PAIRS)}
        cut = [blocks(pcm[lab], a, b) for lab in LABELS]
        left, right = np.concatenate([c[0] for c in cut]), np.concatenate([c[1] for c in cut])
        left.setflags(write=False)
        right.setflags(write=False)
        rows = {lab: slice(i * N_FRAMES, (i + 1) * N_FRAMES) for i, lab in enumerate(LABELS)}
        _cache[key] = dict(labels=LABELS, pcm=pcm, starts=starts_of(a, b), left=left, right=right, rows=rows)
    return _cache[key]
