"""
PacStore: `.pac` files resident on the device of a Handle (mrc_pac_store_*), sample windows of them decoded straight into
torch tensors [item][channel][time] on that device.  Upload once, crop for ever: a call parses and synthesises only the
blocks its windows overlap, and no file byte crosses PCIe again.

    with PacStore(handle, bufs) as store:
        x = store.decode_window(files, starts, 48000, dtype=torch.float32)     # [len(files)][channels][48000], on the GPU
        y = store.decode_window(files, starts, 12000, dtype=torch.float32, rate_divisor=4)   # the same second at 1/4 rate
        m = store.decode_window(files, starts, 24000, dtype=torch.float32, rate_divisor=2, mix="mid")   # [len(files)][1][24000]

rate_divisor = 2 or 4 (mrc_pac_store_decode_window_reduced) decodes at half or quarter sample rate straight from the MDCT
lines: the first 1/D of each block's lines through an inverse transform D times shorter.  starts and window then count
reduced samples; reduced sample m is the signal, band-limited to the new Nyquist frequency, at full-rate time
D m + (D - 1) / 2 -- (D - 1) / 2 full-rate samples after full-rate sample D m.

mix = "mid", "left" or "right" (mrc_pac_store_decode_window_mix) gives ONE channel of every file, stereo or mono: left and
right are the bits of that channel of the two-channel call; mid is (L + R) / 2 formed on the MDCT lines, where most bands
of a stereo file hold it already, so that a stereo block costs one inverse transform, one plane and one output row.

resample = (up, down) (mrc_pac_store_decode_window_resampled) gives the window at up / down of the rate_divisor's rate -- any
rational rate, 16 kHz from 48 kHz files among them -- through a polyphase Hann-windowed sinc that reads the float64 planes
on the device; starts and window then count output samples:

        d, up, down = resample_plan(48000, 16000)                              # (2, 2, 3): half-rate synthesis, then 2 / 3
        z = store.decode_window(files, starts, 16000, dtype=torch.float32, rate_divisor=d, resample=(up, down))

levels (mrc_pac_store_block_energy) answers how loud every stretch of every file is without decoding it: the sum of squares
of each block's decoded MDCT lines IS the energy the block adds to the signal (Parseval on the orthogonal lapped transform),
and levels.LevelMap turns those numbers into window levels, admissible crop starts, reproducible draws and gains:

        m = store.levels()                                                     # every file, per channel; cached
        starts = m.sample_starts(files, 48000, -40.0, np.random.default_rng(0))   # crops at or above -40 dB RMS
        x = store.decode_window(files, starts, 48000, dtype=torch.float32)
        x *= torch.from_numpy(m.gains_to(-20.0, files, starts, 48000)).to(x)[:, None, None]

decode_window_sum (mrc_pac_store_decode_window_sum) gives windows that are weighted sums of crops -- speech over noise at a drawn
SNR, an event placed inside a background (a term's start may be negative: it reads zeros there), mixup -- folded from the
float64 planes in one call, every bit defined, no per-term window written:

        g = m.gains_for_snr(10.0, speech, s_starts, noise, n_starts, 48000)   # the noise 10 dB below the speech
        x = store.decode_window_sum(np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1),
                                    np.stack([np.ones_like(g), g], 1), 48000, dtype=torch.float32)

band_gains= (mrc_pac_store_decode_window_shaped) changes the spectrum of a crop, or of a term of a sum, where it is cheapest: one
multiplication per decoded MDCT line, between the dequantiser and the inverse transform that runs anyway -- a telephone band
for the speech term, an EQ tilt per item, frequency masks, a per-item low-pass.  Per-line gains on a lapped transform are not
an LTI filter: smooth curves are clean, a brick-wall edge leaves a small aliasing residue near the edge frequency:

        tilt = gains_from_db(np.linspace(3.0, -9.0, 25))                       # one row for every item, the codec's 25 bands
        x = store.decode_window(files, starts, 48000, dtype=torch.float32, band_gains=tilt)
        masks = band_mask_gains(len(files), 25, np.random.default_rng(0), n_masks=2, max_width=4)
        y = store.decode_window(files, starts, 48000, dtype=torch.float32, band_gains=masks)
        z = store.decode_window(files, starts, 48000, band_gains=[0.0, 1.0, 0.0], band_edges_hz=[0, 300, 3400, 24000])   # telephone band

speed_factors=, speed_index= (mrc_pac_store_decode_window_speeds) read every item, or every term of a sum, at a speed of its own
drawn from a short list -- the speed perturbation of speech recipes (0.9x, 1.0x, 1.1x per utterance) in one call, one plan and
one output kernel, each unit bit for bit what decode_window(resample=its ratio) gives.  Speech at a drawn speed over noise at
speed 1 at a drawn SNR, at 16 kHz from 48 kHz files; source_spans says which stretch of the half-rate signal a sped-up term
lies over, which is what the levels are asked about:

        speeds = [(9, 10), (1, 1), (11, 10)]                                   # the term's ratio: 2 / 3 divided by its speed
        ratios = speed_ratios((2, 3), speeds)                                  # [(20, 27), (2, 3), (20, 33)]
        pick = rng.integers(0, 3, len(speech))
        first, length = store.source_spans(s_starts, 16000, ratios, pick, rate_divisor=2)
        n_first, _ = store.source_spans(n_starts, 16000, [(2, 3)], np.zeros_like(pick), rate_divisor=2)
        m, g = store.levels(2, "mid"), np.ones(len(speech))
        for r in range(3):                                                     # (one window length per question)
            k = pick == r
            g[k] = m.gains_for_snr(rng.uniform(0, 20), speech[k], first[k], noise[k], n_first[k], int(length[k][0])) if k.any() else 1.0
        x = store.decode_window_sum(np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1), np.stack([np.ones_like(g), g], 1),
                                    16000, dtype=torch.float32, rate_divisor=2, mix="mid", resample=(2, 3),
                                    speed_factors=speeds, speed_index=np.stack([pick, np.ones_like(pick)], 1))   # the noise: speed 1

ir_index= (mrc_pac_store_decode_window_reverb) sends an item, or a term of a sum, through a room: the store keeps a bank of impulse
responses (set_impulse_responses; ir_at_rate brings a recorded one to the rate the terms are read at), and a term is convolved
with the response it names, last of all, in float64 overlap-save on the device -- speech through a room over dry noise:

        store.set_impulse_responses([ir_at_rate(h, 48000, 16000) for h in rooms])
        x = store.decode_window_sum(np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1), np.stack([np.ones_like(g), g], 1),
                                    16000, dtype=torch.float32, rate_divisor=2, mix="mid", resample=(2, 3),
                                    ir_index=np.stack([rng.integers(0, len(rooms), len(speech)), np.full(len(speech), -1)], 1))

band_energy_window (mrc_pac_store_band_energy_window) is the time-frequency feature that usually follows a crop, taken from
the same sums split by frequency band and laid on a frame grid -- the coded file already is a time-frequency representation:

        edges = critical_band_edges(48000)                                     # 0, 100, 200, ... 15500, 24000
        e = store.band_energy_window(files, starts, 94, 512, edges)            # [len(files)][channels][25][94], on the GPU
        logspec = torch.log10(e.clamp_min(1e-12))

filterbank_window (mrc_pac_store_filterbank_window) is that call with overlapping triangular filters in place of the
rectangular bands -- a mel front end without a decode or an STFT.  A line's weight in a filter is the triangle's mean over the
line's own frequency interval, so a filter narrower than a short block's line spacing is never empty and the log needs no
-inf guard beyond digital silence:

        points = mel_points(80, 0.0, 24000.0)                                  # 82 points: HTK mel, 80 filters
        e = store.filterbank_window(files, starts, 100, 480, points)           # [len(files)][channels][80][100], on the GPU
        logmel = torch.log(e.clamp_min(1e-10))

stft_window (mrc_pac_store_stft_window) is the STFT itself -- torch.stft's numbers, for a pretrained front end -- of any row
decode_window_sum can make (mixtures, speeds, band gains, rooms), with the caller's frame window and mel matrix, and no
waveform tensor in between:

        bank = mel_bin_weights(400, 16000, mel_points(80, 0.0, 8000.0))        # [80][201], torchaudio's melscale_fbanks rule
        e = store.stft_window(files, starts, 98, 160, 400, bank=bank, output="bank", rate_divisor=2, mix="mid", resample=(2, 3))
        logmel = torch.log(e.clamp_min(1e-10))                                 # [len(files)][1][80][98]

span_first=, span_len=, fade_in=, fade_out= (mrc_pac_store_decode_window_spans) let a term of a sum sound in PART of its row, with a
linear fade at either end; what is parsed and synthesised follows the spans, not the window.  Concatenation -- a row of pieces
laid end to end, eight utterances packed into one 10 s row or pieces of one file in another order, optionally crossfaded --
is one call; concat_spans does the arithmetic (a term's start is the source position that stands at row sample 0):

        lengths = np.full((len(rows), 8), 20000)                               # eight pieces of 1.25 s per row at 16 kHz
        starts, first, length, fin, fout = concat_spans(lengths, piece_starts, crossfade=160)
        x = store.decode_window_sum(piece_files, starts, np.ones(starts.shape), int(first[0, -1] + length[0, -1]), dtype=torch.float32,
                                    rate_divisor=2, mix="mid", resample=(2, 3), span_first=first, span_len=length,
                                    fade_in=fin, fade_out=fout)

A placed, cropped event -- 0.5 s from source sample p of the event's file at 0.3 s into a 4 s background, faded over 5 ms; the
event's file is parsed under its 0.5 s only:

        at, n = 4800, 8000
        x = store.decode_window_sum(np.stack([background, event], 1), np.stack([b_starts, p - at], 1), np.stack([np.ones_like(g), g], 1),
                                    64000, dtype=torch.float32, rate_divisor=2, mix="mid", resample=(2, 3),
                                    span_first=np.stack([np.zeros_like(p), np.full_like(p, at)], 1),
                                    span_len=np.stack([np.full_like(p, 64000), np.full_like(p, n)], 1), fade_in=[0, 80], fade_out=[0, 80])
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib

STAT_NAMES = ("chunks_parsed", "decode_launches", "slabs", "plan_bytes_uploaded")
MS_NAMES = ("plan_upload", "unpack", "synthesis", "window_out")
RATE_DIVISORS = (1, 2, 4)
MIXES = {"mid": _lib.MRC_MIX_MID, "left": _lib.MRC_MIX_LEFT, "right": _lib.MRC_MIX_RIGHT}


def check_rate_divisor(rate_divisor, what="decode_window"):
    """rate_divisor as an int in RATE_DIVISORS, else ValueError (a bool or a float is not an int)"""
    if isinstance(rate_divisor, bool) or not isinstance(rate_divisor, (int, np.integer)) or int(rate_divisor) not in RATE_DIVISORS:
        raise ValueError("%s: rate_divisor must be an int in {1, 2, 4}, got %r" % (what, rate_divisor))
    return int(rate_divisor)


def check_mix(mix, channels=None, what="decode_window"):
    """mix (None: no mix) with the channels asked for beside it -> its MRC_MIX_* value or None, else ValueError"""
    if mix is None:
        return None
    if not isinstance(mix, str) or mix not in MIXES:
        raise ValueError('%s: mix must be None, "mid", "left" or "right", got %r' % (what, mix))
    if channels is not None and (isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or int(channels) != 1):
        raise ValueError("%s: mix=%r gives one channel, channels must be None or 1, got %r" % (what, mix, channels))
    return MIXES[mix]


RESAMPLE_ZEROS, RESAMPLE_ROLLOFF = 16, 0.9475     # the defaults of resample_taps
RESAMPLE_MAX_TERM, RESAMPLE_MAX_RATIO, RESAMPLE_MAX_ZEROS = 1024, 8, 64


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_resample(resample, what="decode_window"):
    """resample as (up, down) or (up, down, zeros, rolloff) -> (up, down, zeros, rolloff) with up / down reduced, or None
    for None and for a ratio of 1; else ValueError: mrc_resample_taps' rule, checked before any library call"""
    if resample is None:
        return None
    if not isinstance(resample, (tuple, list)) or len(resample) not in (2, 4):
        raise ValueError("%s: resample must be None, (up, down) or (up, down, zeros, rolloff), got %r" % (what, resample))
    up, down = resample[0], resample[1]
    zeros, rolloff = (RESAMPLE_ZEROS, RESAMPLE_ROLLOFF) if len(resample) == 2 else resample[2:]
    for name, v in (("up", up), ("down", down)):
        if not _is_int(v) or int(v) < 1:
            raise ValueError("%s: resample: %s must be a positive int, got %r" % (what, name, v))
    g = int(np.gcd(int(up), int(down)))
    up, down = int(up) // g, int(down) // g
    for name, v in (("up", up), ("down", down)):
        if v > RESAMPLE_MAX_TERM:
            raise ValueError("%s: resample: %s = %d (of %d / %d, reduced) is above %d" % (what, name, v, up, down, RESAMPLE_MAX_TERM))
    if down > RESAMPLE_MAX_RATIO * up or up > RESAMPLE_MAX_RATIO * down:
        raise ValueError("%s: resample: up / down = %d / %d is outside [1 / %d, %d]" % (what, up, down, RESAMPLE_MAX_RATIO, RESAMPLE_MAX_RATIO))
    if not _is_int(zeros) or not 1 <= int(zeros) <= RESAMPLE_MAX_ZEROS:
        raise ValueError("%s: resample: zeros must be an int in 1..%d, got %r" % (what, RESAMPLE_MAX_ZEROS, zeros))
    if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float, np.integer, np.floating)) or not 0.5 <= float(rolloff) <= 1.0:
        raise ValueError("%s: resample: rolloff must be a number in [0.5, 1], got %r" % (what, rolloff))
    if up == down:
        return None
    return up, down, int(zeros), float(rolloff)


def resample_taps(up, down, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF):
    """mrc_resample_taps -> (W, float64 [up][2 W]) with up / down reduced: the Hann-windowed sinc of
    PacStore.decode_window(resample=), phase p and tap j at d = (j - W + 1) - p / up input samples from the output sample.
    No handle, no GPU.  MrcError where the library refuses."""
    def call(w, taps):
        rc = lib.mrc_resample_taps(int(up), int(down), int(zeros), float(rolloff), w.ctypes.data, taps)
        if rc:
            err = _lib.MrcError("libmrc_hip error %d: %s" % (rc, lib.mrc_last_error(None).decode()))
            err.code = rc
            raise err
    w = np.zeros(1, np.int32)
    call(w, None)
    g = int(np.gcd(int(up), int(down)))
    taps = np.zeros((int(up) // g, 2 * int(w[0])), np.float64)
    call(w, taps.ctypes.data)
    return int(w[0]), taps


def resample_plan(rate_in, rate_out, divisors=RATE_DIVISORS):
    """How to read files of rate_in Hz at rate_out Hz -> (rate_divisor, up, down): the largest divisor D of `divisors` that
    divides rate_in with rate_in / D >= rate_out -- the cheapest synthesis that still holds the band -- and up / down =
    rate_out / (rate_in / D), reduced (1, 1: that divisor alone gives the rate).  48000 -> 16000: (2, 2, 3); 44100 -> 16000:
    (2, 320, 441); a rate_out above rate_in: divisor 1 (44100 -> 48000: (1, 160, 147)).  ValueError for rates that are not
    positive ints and for a fraction outside what decode_window(resample=) takes."""
    for name, v in (("rate_in", rate_in), ("rate_out", rate_out)):
        if not _is_int(v) or int(v) < 1:
            raise ValueError("resample_plan: %s must be a positive int, got %r" % (name, v))
    rate_in, rate_out = int(rate_in), int(rate_out)
    fits = [check_rate_divisor(d, "resample_plan") for d in divisors]
    d = max([d for d in fits if rate_in % d == 0 and rate_in // d >= rate_out] or [1])     # (a rate above the file's: full rate)
    g = int(np.gcd(rate_out, rate_in // d))
    up, down = rate_out // g, rate_in // d // g
    check_resample((up, down), "resample_plan")
    return d, up, down


MAX_RATIOS = 8                           # MRC_MAX_STORE_RATIOS


def _speed_list(resample, speed_factors, what):
    """-> ([(up, down)] reduced, zeros, rolloff): resample's base ratio (None: 1 / 1) divided by every speed; ValueError as
    speed_ratios describes it"""
    checked = check_resample(resample, what)
    zeros, rolloff = (RESAMPLE_ZEROS, RESAMPLE_ROLLOFF) if resample is None or len(resample) == 2 else (int(resample[2]), float(resample[3]))
    base_up, base_down = (1, 1) if resample is None else (int(resample[0]), int(resample[1]))
    if checked is not None:
        base_up, base_down = checked[0], checked[1]
    if not isinstance(speed_factors, (tuple, list)) or not 1 <= len(speed_factors) <= MAX_RATIOS:
        raise ValueError("%s: speed_factors must be a list of 1 to %d (num, den) pairs, got %r" % (what, MAX_RATIOS, speed_factors))
    ratios = []
    for i, f in enumerate(speed_factors):
        if not isinstance(f, (tuple, list)) or len(f) != 2 or not all(_is_int(v) and int(v) >= 1 for v in f):
            raise ValueError("%s: speed_factors[%d] must be a pair of positive ints (num, den), got %r" % (what, i, f))
        num, den = int(f[0]), int(f[1])
        up, down = base_up * den, base_down * num
        g = int(np.gcd(up, down))
        up, down = up // g, down // g
        if max(up, down) >= 1 << 31:
            raise ValueError("%s: speed_factors[%d] = %d / %d: the combined ratio %d / %d does not fit an int" % (what, i, num, den, up, down))
        check_resample((up, down, zeros, rolloff), "%s: speed_factors[%d] = %d / %d on %d / %d" % (what, i, num, den, base_up, base_down))
        ratios.append((up, down))
    return ratios, zeros, rolloff


def speed_ratios(resample, speed_factors):
    """The ratios at which decode_window(resample=, speed_factors=) reads its units -> [(up, down)], reduced, one per factor:
    resample's base ratio (None: 1 / 1) divided by the speed num / den -- a speed above 1 plays faster, so fewer output
    samples cover the same source.  48 kHz files at 16 kHz (rate_divisor 2, resample (2, 3)) at 9/10, 1, 11/10:
    [(20, 27), (2, 3), (20, 33)].  No handle, no GPU.  ValueError for a list that is not 1 to 8 pairs of positive ints and for
    a combined ratio outside what check_resample takes, named with its reduced terms (320 / 441 at 11 / 10 is 3200 / 4851)."""
    return _speed_list(resample, speed_factors, "speed_ratios")[0]


def check_speed_index(speed_index, unit_shape, n_ratios, what="decode_window"):
    """speed_index of a window call -> int32 [units], contiguous, else ValueError: ints, the shape of the call's units, every
    value an index into the list of n_ratios"""
    unit_shape = tuple(int(v) for v in unit_shape)
    try:
        idx = np.asarray(speed_index)
        if idx.dtype == object or idx.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("%s: speed_index must be ints, got %r" % (what, speed_index))
    if idx.shape != unit_shape:
        raise ValueError("%s: speed_index must have shape %s, got %s" % (what, unit_shape, idx.shape))
    idx = idx.reshape(-1)
    bad = np.flatnonzero((idx < 0) | (idx >= n_ratios))
    if bad.size:
        raise ValueError("%s: speed_index must lie in 0..%d (the speed_factors given), got %d at unit %d"
                         % (what, n_ratios - 1, int(idx[bad[0]]), int(bad[0])))
    return np.ascontiguousarray(idx.astype(np.int32))


REVERB_BLOCK = _lib.MRC_STORE_REVERB_BLOCK          # the overlap-save hop B of ir_index= (transforms of 2 B points)
MAX_IR_TAPS = _lib.MRC_MAX_STORE_IR_TAPS


def check_impulse_responses(irs, what="set_impulse_responses"):
    """a bank for PacStore.set_impulse_responses -> (offsets int64 [n + 1], taps float64, back to back), else ValueError: a
    list of 1-D arrays of 1..MAX_IR_TAPS finite numbers each; None or an empty list: no bank, (offsets [0], no taps)"""
    if irs is None:
        irs = []
    if isinstance(irs, np.ndarray) or not isinstance(irs, (tuple, list)):
        raise ValueError("%s: the bank must be a list of 1-D arrays (or None), got %r" % (what, type(irs).__name__))
    rows = []
    for j, ir in enumerate(irs):
        try:
            a = np.asarray(ir)
            if a.dtype == object or a.dtype.kind not in "fiu":
                raise TypeError
            a = a.astype(np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s: impulse response %d must be numbers, got %r" % (what, j, ir))
        if a.ndim != 1 or not 1 <= a.size <= MAX_IR_TAPS:
            raise ValueError("%s: impulse response %d must be 1-D with 1 to %d taps, got shape %s" % (what, j, MAX_IR_TAPS, a.shape))
        bad = np.flatnonzero(~np.isfinite(a))
        if bad.size:
            raise ValueError("%s: impulse response %d must be finite, got %r at tap %d" % (what, j, float(a[bad[0]]), int(bad[0])))
        rows.append(a)
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=offsets[1:])
    taps = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, np.float64)
    return offsets, taps


def check_ir_index(ir_index, unit_shape, n_irs, what="decode_window"):
    """ir_index of a window call -> int32 [units], contiguous, else ValueError: ints, the shape of the call's units, every value
    -1 (not convolved) or an index into the store's bank of n_irs impulse responses"""
    unit_shape = tuple(int(v) for v in unit_shape)
    try:
        idx = np.asarray(ir_index)
        if idx.dtype == object or idx.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("%s: ir_index must be ints, got %r" % (what, ir_index))
    if idx.shape != unit_shape:
        raise ValueError("%s: ir_index must have shape %s, got %s" % (what, unit_shape, idx.shape))
    idx = idx.reshape(-1)
    bad = np.flatnonzero((idx < -1) | (idx >= n_irs))
    if bad.size:
        if n_irs == 0:
            raise ValueError("%s: ir_index names impulse response %d at unit %d, but the store has none (set_impulse_responses)"
                             % (what, int(idx[bad[0]]), int(bad[0])))
        raise ValueError("%s: ir_index must be -1 or lie in 0..%d (the store's impulse responses), got %d at unit %d"
                         % (what, n_irs - 1, int(idx[bad[0]]), int(bad[0])))
    return np.ascontiguousarray(idx.astype(np.int32))


MAX_SPAN = 1 << 40                        # of span_len and of |span_first| (the library's bound on a window)


def check_spans(span_first, span_len, fade_in, fade_out, unit_shape, what="decode_window_sum"):
    """The spans of a call's terms and their fades as int64 arrays of unit_shape, the shape of files -> (span_first, span_len,
    fade_in, fade_out), or None where all four are None.  span_first and span_len go together and have the shape of files; a
    fade is None (0), a scalar (every term) or an array of that shape.  ValueError: one of span_first / span_len without the
    other, a fade without spans, another shape, values that are not whole numbers, span_len outside [0, 2^40], |span_first|
    above 2^40, a negative fade, fade_in + fade_out above the term's span_len."""
    if span_first is None and span_len is None:
        for name, v in (("fade_in", fade_in), ("fade_out", fade_out)):
            if v is not None:
                raise ValueError("%s: %s goes with span_first and span_len" % (what, name))
        return None
    if span_first is None or span_len is None:
        raise ValueError("%s: span_first and span_len go together, got only %s" % (what, "span_len" if span_first is None else "span_first"))
    out = []
    for name, v, scalar_ok in (("span_first", span_first, False), ("span_len", span_len, False), ("fade_in", fade_in, True),
                               ("fade_out", fade_out, True)):
        a = np.asarray(0 if v is None else v)
        if a.dtype.kind not in "iu" or a.dtype == np.bool_:
            if a.dtype.kind != "f" or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
                raise ValueError("%s: %s must hold whole numbers, got %r" % (what, name, v))
        if a.dtype.kind == "f" and a.size and np.max(np.abs(a)) > 2.0 ** 62:
            raise ValueError("%s: %s is out of range, got %r" % (what, name, v))
        a = a.astype(np.int64)
        if scalar_ok and a.ndim == 0:
            a = np.full(unit_shape, int(a), np.int64)
        if a.shape != tuple(unit_shape):
            raise ValueError("%s: %s must have the shape of files %s%s, got %s"
                             % (what, name, tuple(unit_shape), " or be a scalar" if scalar_ok else "", a.shape))
        out.append(np.ascontiguousarray(a.reshape(-1)))
    first, length, fin, fout = out
    for name, bad in (("span_len must lie in [0, 2^40]", (length < 0) | (length > MAX_SPAN)),
                      ("span_first must lie in [-2^40, 2^40]", np.abs(first) > MAX_SPAN),
                      ("fade_in must not be negative", fin < 0), ("fade_out must not be negative", fout < 0),
                      ("fade_in + fade_out must not exceed span_len", fin + fout > length)):
        at = np.flatnonzero(bad)
        if at.size:
            k = int(at[0])
            raise ValueError("%s: %s, got span_first %d, span_len %d, fade_in %d, fade_out %d at term %d"
                             % (what, name, first[k], length[k], fin[k], fout[k], k))
    return first, length, fin, fout


def concat_spans(lengths, source_starts, crossfade=0, item_offsets=None):
    """Rows of pieces laid end to end -> (starts, span_first, span_len, fade_in, fade_out) for decode_window_sum and
    stft_window, each of the shape of lengths.  lengths, source_starts: [n][K], or 1-D [terms] with item_offsets [n + 1] as those
    calls take them; piece k is lengths[k] row samples from source position source_starts[k] of its file (both in output
    samples at the term's ratio).  A row's first piece begins at row sample 0 and every later one `crossfade` samples before
    its predecessor ends; over that overlap the earlier piece fades out and the later one fades in, linearly, their weights
    adding to 1 (crossfade=0: the pieces abut, no fade).  A row's outer ends are not faded.  The row ends at span_first +
    span_len of its last piece.  ValueError: shapes that do not agree, a negative length or crossfade, and a crossfade longer
    than half an inner piece (a piece that fades at both ends) or than a row's first or last piece."""
    lengths, src = np.asarray(lengths, dtype=np.int64), np.asarray(source_starts, dtype=np.int64)
    if lengths.shape != src.shape:
        raise ValueError("concat_spans: lengths and source_starts must have one shape, got %s and %s" % (lengths.shape, src.shape))
    if isinstance(crossfade, (bool, np.bool_)) or not _is_int(crossfade) or crossfade < 0:
        raise ValueError("concat_spans: crossfade must be a whole number >= 0, got %r" % (crossfade,))
    crossfade = int(crossfade)
    if item_offsets is None:
        if lengths.ndim != 2:
            raise ValueError("concat_spans: lengths must be [n][K], or 1-D with item_offsets; got shape %s" % (lengths.shape,))
        offsets = np.arange(lengths.shape[0] + 1, dtype=np.int64) * lengths.shape[1]
    else:
        offsets = np.asarray(item_offsets, dtype=np.int64)
        if lengths.ndim != 1 or offsets.ndim != 1 or offsets.size < 1 or offsets[0] != 0 or np.any(np.diff(offsets) < 0) or \
                offsets[-1] != lengths.size:
            raise ValueError("concat_spans: with item_offsets, lengths must be 1-D and item_offsets [n + 1], start at 0, not "
                             "decrease and end at the number of pieces; got %r" % (item_offsets,))
    shape, flat, src = lengths.shape, lengths.reshape(-1), src.reshape(-1)
    if np.any(flat < 0):
        raise ValueError("concat_spans: lengths must not be negative, got %d at piece %d" % (flat[flat < 0][0], np.flatnonzero(flat < 0)[0]))
    first, fin, fout = np.zeros(flat.size, np.int64), np.zeros(flat.size, np.int64), np.zeros(flat.size, np.int64)
    for i in range(offsets.size - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        at = 0
        for k in range(a, b):
            fin[k] = crossfade if k > a else 0
            fout[k] = crossfade if k < b - 1 else 0
            if fin[k] + fout[k] > flat[k]:
                raise ValueError("concat_spans: crossfade %d does not fit piece %d of %d samples, which fades over %d"
                                 % (crossfade, k, flat[k], fin[k] + fout[k]))
            first[k] = at - fin[k]
            at = first[k] + flat[k]
    return tuple(v.reshape(shape) for v in (src - first, first, flat.copy(), fin, fout))


ROUTE_NONE = _lib.MRC_ROUTE_NONE                      # route_irs: the term does not reach this channel
MAX_ROUTE_CHANNELS = _lib.MRC_MAX_STORE_ROUTE_CHANNELS


def check_routes(route_gains, route_irs, n_terms, n_irs, what="decode_window_routed"):
    """the routes of a routed window call -> (gains float64 [n_terms][C], irs int32 [n_terms][C]), contiguous, else ValueError:
    two arrays of ONE shape, the call's terms (any leading axes with n_terms entries in all) and a last axis of 1 to
    MAX_ROUTE_CHANNELS output channels; gains finite numbers; irs ints, each ROUTE_NONE (the term does not reach the channel),
    -1 (dry) or an index into the store's bank of n_irs impulse responses"""
    try:
        g = np.asarray(route_gains)
        if g.dtype == object or g.dtype.kind not in "fiu":
            raise TypeError
        g = g.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: route_gains must be numbers, got %r" % (what, route_gains))
    try:
        idx = np.asarray(route_irs)
        if idx.dtype == object or idx.dtype.kind not in "iu":
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("%s: route_irs must be ints, got %r" % (what, route_irs))
    n_terms = int(n_terms)
    if g.shape != idx.shape or g.ndim < 2 or not 1 <= g.shape[-1] <= MAX_ROUTE_CHANNELS or \
            int(np.prod(g.shape[:-1], dtype=np.int64)) != n_terms:
        raise ValueError("%s: route_gains and route_irs must have one shape, the %d terms and a last axis of 1 to %d channels, "
                         "got %s and %s" % (what, n_terms, MAX_ROUTE_CHANNELS, g.shape, idx.shape))
    n_ch = g.shape[-1]
    g, idx = g.reshape(n_terms, n_ch), idx.reshape(n_terms, n_ch)
    at = lambda bad: (int(bad[0]) // n_ch, int(bad[0]) % n_ch)
    bad = np.flatnonzero(~np.isfinite(g))
    if bad.size:
        raise ValueError("%s: route_gains must be finite, got %r at term %d, channel %d" % ((what, float(g.flat[bad[0]])) + at(bad)))
    bad = np.flatnonzero(idx < ROUTE_NONE)
    if bad.size:
        raise ValueError("%s: route_irs must be ROUTE_NONE (%d), -1 or an index into the bank, got %d at term %d, channel %d"
                         % ((what, ROUTE_NONE, int(idx.flat[bad[0]])) + at(bad)))
    bad = np.flatnonzero(idx >= n_irs)
    if bad.size:
        if n_irs == 0:
            raise ValueError("%s: route_irs names impulse response %d at term %d, channel %d, but the store has none "
                             "(set_impulse_responses)" % ((what, int(idx.flat[bad[0]])) + at(bad)))
        raise ValueError("%s: route_irs must be ROUTE_NONE (%d), -1 or lie in 0..%d (the store's impulse responses), got %d at "
                         "term %d, channel %d" % ((what, ROUTE_NONE, n_irs - 1, int(idx.flat[bad[0]])) + at(bad)))
    return np.ascontiguousarray(g), np.ascontiguousarray(idx.astype(np.int32))


def array_routes(room_of, n_mics, gains=None):
    """The routes of terms heard by a microphone array -> (route_gains float64, route_irs int32), both of room_of's shape plus a
    last axis [n_mics], for a bank laid out room-major: microphone c of room r is impulse response r * n_mics + c.  room_of:
    ints, the room of every term; -1: the term is dry on every channel.  gains: None (1.0), or numbers of room_of's shape (one
    gain per term, the same on every microphone) or of the result's shape.  ValueError for rooms that are not ints >= -1, an
    n_mics outside 1..MAX_ROUTE_CHANNELS and gains of another shape."""
    what = "array_routes"
    if not _is_int(n_mics) or not 1 <= int(n_mics) <= MAX_ROUTE_CHANNELS:
        raise ValueError("%s: n_mics must be an int in 1..%d, got %r" % (what, MAX_ROUTE_CHANNELS, n_mics))
    n_mics = int(n_mics)
    rooms = np.asarray(room_of)
    if rooms.dtype == object or rooms.dtype.kind not in "iu" or (rooms.size and int(rooms.min()) < -1):
        raise ValueError("%s: room_of must be ints >= -1 (-1: a dry term), got %r" % (what, room_of))
    rooms = rooms.astype(np.int64)
    irs = np.where(rooms[..., None] < 0, -1, rooms[..., None] * n_mics + np.arange(n_mics, dtype=np.int64))
    g = np.ones(irs.shape, np.float64)
    if gains is not None:
        gains = np.asarray(gains, dtype=np.float64)
        if gains.shape == rooms.shape:
            gains = gains[..., None]
        elif gains.shape != irs.shape:
            raise ValueError("%s: gains must have shape %s or %s, got %s" % (what, rooms.shape, irs.shape, gains.shape))
        g = g * gains
    return g, irs.astype(np.int32)


def ir_at_rate(ir, rate_in, rate_out):
    """A recorded room impulse response at the rate the terms are read at -> float64 [ceil(len(ir) * rate_out / rate_in)].  Host
    NumPy over the library's own polyphase filter (resample_taps(up, down), up / down = rate_out / rate_in reduced): output n
    is the fold over j = 0 .. 2 W - 1 of taps[p][j] * ir[q - W + 1 + j] (zero outside the response), q = n down // up and p =
    n down % up -- decode_window(resample=)'s rule -- times down / up, the factor that keeps the DC gain sum(ir) of the
    convolution at the new rate; where that nominal result's sum lies within one half of sum(ir) != 0 it is rescaled so that
    the two sums agree.  Equal rates: a float64 copy.  ValueError for rates that are not positive ints, a response that is not
    1-D finite numbers, and a ratio outside what decode_window(resample=) takes."""
    what = "ir_at_rate"
    for name, v in (("rate_in", rate_in), ("rate_out", rate_out)):
        if not _is_int(v) or int(v) < 1:
            raise ValueError("%s: %s must be a positive int, got %r" % (what, name, v))
    _, taps_in = check_impulse_responses([ir], what)
    g = int(np.gcd(int(rate_in), int(rate_out)))
    up, down = int(rate_out) // g, int(rate_in) // g
    if up == down:
        return taps_in.copy()
    check_resample((up, down), what)
    W, taps = resample_taps(up, down)
    n_out = -((-taps_in.size * up) // down)
    nd = np.arange(n_out, dtype=np.int64) * down
    q, p = nd // up, nd % up
    padded = np.concatenate([np.zeros(W, np.float64), taps_in, np.zeros(W + 1, np.float64)])
    out = np.zeros(n_out, np.float64)
    for j in range(2 * W):                                   # ir[q - W + 1 + j] is padded[q + 1 + j]
        out += taps[p, j] * padded[q + 1 + j]
    out *= down / up
    s_in, s_out = float(taps_in.sum()), float(out.sum())
    if s_in != 0.0 and s_out != 0.0 and abs(s_out - s_in) <= 0.5 * abs(s_in):
        out *= s_in / s_out
    return out


def check_levels_mix(mix, what="levels"):
    """mix of PacStore.levels -> MRC_MIX_EACH (None: every channel) or MRC_MIX_MID, else ValueError"""
    if mix is None:
        return _lib.MRC_MIX_EACH
    if isinstance(mix, str) and mix in ("left", "right"):
        raise ValueError('%s: mix=%r is a column of mix=None (every channel): ask for that and take channel %d'
                         % (what, mix, ("left", "right").index(mix)))
    if not isinstance(mix, str) or mix != "mid":
        raise ValueError('%s: mix must be None or "mid", got %r' % (what, mix))
    return _lib.MRC_MIX_MID


MAX_BANDS = 256                          # MRC_MAX_STORE_BANDS
# the codec's critical-band limits below the last (psychoac.py:82-84; the last band takes what is left, up to Nyquist)
CRITICAL_BAND_LIMITS_HZ = (100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700, 4400,
                           5300, 6400, 7700, 9500, 12000, 15500)


def critical_band_edges(sample_rate):
    """0, the codec's 24 critical-band limits below Nyquist, Nyquist -> float64 [bands + 1]: at 48 kHz the 25 bands of a long
    block's scale-factor table"""
    nyquist = float(sample_rate) / 2.0
    if not np.isfinite(nyquist) or nyquist <= 0:
        raise ValueError("critical_band_edges: sample_rate must be a positive number, got %r" % (sample_rate,))
    return np.array([0.0] + [float(f) for f in CRITICAL_BAND_LIMITS_HZ if f < nyquist] + [nyquist])


def check_band_edges(band_edges_hz, what="band_energy_window"):
    """band edges in Hz -> float64 [bands + 1], else ValueError: 1 to MAX_BANDS bands, finite, from 0 up, strictly increasing"""
    try:
        edges = np.ascontiguousarray(np.asarray(band_edges_hz, dtype=np.float64).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError("%s: band_edges_hz must be a sequence of frequencies in Hz, got %r" % (what, band_edges_hz))
    if not 2 <= edges.size <= MAX_BANDS + 1:
        raise ValueError("%s: band_edges_hz must hold 2 to %d edges (1 to %d bands), got %d" % (what, MAX_BANDS + 1, MAX_BANDS, edges.size))
    if not np.all(np.isfinite(edges)):
        raise ValueError("%s: band_edges_hz must be finite, got %r" % (what, band_edges_hz))
    if edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("%s: band_edges_hz must start at or above 0 and increase strictly, got %r" % (what, band_edges_hz))
    return edges


def check_band_gains(band_gains, unit_shape, n_bands, what="decode_window", band_edges_hz=None):
    """band_gains of decode_window / decode_window_sum -> float64 [units][n_bands], contiguous (None: None), else ValueError:
    unit_shape is the shape of the call's units ((n,) items, or the shape of decode_window_sum's files), band_gains that shape
    plus a last axis [n_bands], or [n_bands] alone for every unit; numbers, finite (zero and negative gains are allowed).
    band_edges_hz is looked at only to refuse it without band_gains."""
    if band_gains is None:
        if band_edges_hz is not None:
            raise ValueError("%s: band_edges_hz is given without band_gains" % what)
        return None
    unit_shape = tuple(int(v) for v in unit_shape)
    try:
        g = np.asarray(band_gains)
        if g.dtype == object or g.dtype.kind not in "fiu":
            raise TypeError
        g = g.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: band_gains must be numbers, got %r" % (what, band_gains))
    if g.shape == (n_bands,):
        g = np.broadcast_to(g, unit_shape + (n_bands,))
    if g.shape != unit_shape + (n_bands,):
        raise ValueError("%s: band_gains must have shape %s or (%d,) (%d bands), got %s"
                         % (what, unit_shape + (n_bands,), n_bands, n_bands, np.shape(band_gains)))
    g = np.ascontiguousarray(g.reshape(-1, n_bands))
    bad = np.argwhere(~np.isfinite(g))
    if bad.size:
        raise ValueError("%s: band_gains must be finite, got %r at unit %d, band %d"
                         % (what, float(g[tuple(bad[0])]), int(bad[0][0]), int(bad[0][1])))
    return g


def gains_from_db(db):
    """decibels -> float64 factors 10^(db / 20), any shape: -inf gives 0.0; +inf and NaN are ValueErrors.  No handle, no GPU."""
    try:
        d = np.asarray(db, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("gains_from_db: db must be numbers, got %r" % (db,))
    if np.any(np.isnan(d)) or np.any(d == np.inf):
        raise ValueError("gains_from_db: db must be finite or -inf, got %r" % (db,))
    with np.errstate(over="raise"):
        try:
            return np.where(np.isneginf(d), 0.0, 10.0 ** (np.where(np.isneginf(d), 0.0, d) / 20.0))
        except FloatingPointError:
            raise ValueError("gains_from_db: 10^(db / 20) overflows for %r" % (db,))


def band_mask_gains(n_items, n_bands, rng, n_masks=1, max_width=8, floor=0.0):
    """SpecAugment-style frequency masks -> float64 [n_items][n_bands] of ones in which, per item, n_masks runs of bands are set
    to `floor`: mask j of item i has width = rng.integers(0, min(max_width, n_bands) + 1) bands from first =
    rng.integers(0, n_bands - width + 1), the draws made item by item, mask by mask, width before first -- reproducible from rng
    (a numpy.random.Generator) alone.  Runs may overlap; a width of 0 masks nothing.  No handle, no GPU."""
    for name, v, least in (("n_items", n_items, 0), ("n_bands", n_bands, 1), ("n_masks", n_masks, 0), ("max_width", max_width, 0)):
        if not _is_int(v) or int(v) < least:
            raise ValueError("band_mask_gains: %s must be an int >= %d, got %r" % (name, least, v))
    if int(n_bands) > MAX_BANDS:
        raise ValueError("band_mask_gains: n_bands must not exceed %d, got %r" % (MAX_BANDS, n_bands))
    if isinstance(floor, bool) or not isinstance(floor, (int, float, np.integer, np.floating)) or not np.isfinite(floor):
        raise ValueError("band_mask_gains: floor must be a finite number, got %r" % (floor,))
    if not isinstance(rng, np.random.Generator):
        raise ValueError("band_mask_gains: rng must be a numpy.random.Generator, got %r" % (rng,))
    n_items, n_bands, widest = int(n_items), int(n_bands), min(int(max_width), int(n_bands))
    g = np.ones((n_items, n_bands), np.float64)
    for i in range(n_items):
        for _ in range(int(n_masks)):
            width = int(rng.integers(0, widest + 1))
            first = int(rng.integers(0, n_bands - width + 1))
            g[i, first:first + width] = float(floor)
    return g


def band_line_ranges(sample_rate, a, b, band_edges_hz):
    """mrc_band_line_ranges -> int32 [bands + 1]: band q of a block of shape (a, b) holds MDCT lines [r[q], r[q + 1]), line k
    lying at (k + 0.5) * ((sample_rate / ((a + b) / 2)) / 2.).  No handle, no GPU.  MrcError where the library refuses."""
    edges = np.ascontiguousarray(np.asarray(band_edges_hz, dtype=np.float64).reshape(-1))
    lo = np.zeros(max(edges.size, 1), np.int32)
    rc = lib.mrc_band_line_ranges(float(sample_rate), int(a), int(b), int(edges.size) - 1, edges.ctypes.data, lo.ctypes.data)
    if rc:
        err = _lib.MrcError("libmrc_hip error %d: %s" % (rc, lib.mrc_last_error(None).decode()))
        err.code = rc
        raise err
    return lo


MEL_SCALES = ("htk", "slaney")
FILTER_NORMS = {None: _lib.MRC_FILTER_NORM_NONE, "slaney": _lib.MRC_FILTER_NORM_SLANEY}


def hz_to_mel(f, scale="htk"):
    """"htk": 2595 log10(1 + f / 700).  "slaney": f / (200 / 3) below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 above.  float64"""
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + 27.0 * np.log(np.maximum(f, 1000.0) / 1000.0) / np.log(6.4))


def mel_to_hz(m, scale="htk"):
    """hz_to_mel's inverse"""
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp(np.maximum(m - 15.0, 0.0) * (np.log(6.4) / 27.0)))


def mel_points(n_filters, f_min, f_max, scale="htk"):
    """the points of a mel filter bank for filterbank_window -> float64 [n_filters + 2]: equally spaced in mel from f_min to
    f_max (scale "htk" or "slaney": hz_to_mel), the first and the last set to f_min and f_max exactly; filter q is the
    triangle over points q, q + 1, q + 2.  NumPy only.  ValueError for arguments that make no bank."""
    if not _is_int(n_filters) or not 1 <= int(n_filters) <= MAX_BANDS:
        raise ValueError("mel_points: n_filters must be an int in 1..%d, got %r" % (MAX_BANDS, n_filters))
    if not isinstance(scale, str) or scale not in MEL_SCALES:
        raise ValueError('mel_points: scale must be "htk" or "slaney", got %r' % (scale,))
    for name, v in (("f_min", f_min), ("f_max", f_max)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("mel_points: %s must be a finite number, got %r" % (name, v))
    f_min, f_max = float(f_min), float(f_max)
    if f_min < 0 or not f_min < f_max:
        raise ValueError("mel_points: 0 <= f_min < f_max is required, got %r and %r" % (f_min, f_max))
    points = mel_to_hz(np.linspace(float(hz_to_mel(f_min, scale)), float(hz_to_mel(f_max, scale)), int(n_filters) + 2), scale)
    points[0], points[-1] = f_min, f_max
    if not np.all(np.diff(points) > 0):
        raise ValueError("mel_points: %d filters from %r to %r Hz are too close to tell apart in float64" % (n_filters, f_min, f_max))
    return points


def check_filter_points(points_hz, what="filterbank_window"):
    """filter points in Hz -> float64 [filters + 2], else ValueError: 1 to MAX_BANDS filters, finite, from 0 up, strictly
    increasing"""
    try:
        points = np.ascontiguousarray(np.asarray(points_hz, dtype=np.float64).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError("%s: points_hz must be a sequence of frequencies in Hz, got %r" % (what, points_hz))
    if not 3 <= points.size <= MAX_BANDS + 2:
        raise ValueError("%s: points_hz must hold 3 to %d points (1 to %d filters), got %d" % (what, MAX_BANDS + 2, MAX_BANDS, points.size))
    if not np.all(np.isfinite(points)):
        raise ValueError("%s: points_hz must be finite, got %r" % (what, points_hz))
    if points[0] < 0 or not np.all(np.diff(points) > 0):
        raise ValueError("%s: points_hz must start at or above 0 and increase strictly, got %r" % (what, points_hz))
    return points


def check_filter_norm(norm, what="filterbank_window"):
    """norm (None or "slaney") -> its MRC_FILTER_NORM_* value, else ValueError"""
    if norm is not None and not (isinstance(norm, str) and norm in FILTER_NORMS):
        raise ValueError('%s: norm must be None or "slaney", got %r' % (what, norm))
    return FILTER_NORMS[norm]


def filterbank_line_weights(sample_rate, a, b, points_hz, norm=None):
    """mrc_filterbank_line_weights -> (lo int32 [filters], hi int32 [filters], [row arrays]): filter q of a block of shape
    (a, b) reads MDCT lines [lo[q], hi[q]) with the float64 weights rows[q], the triangle's mean over each line's interval
    [k d, (k + 1) d), d = (sample_rate / ((a + b) / 2)) / 2.  No handle, no GPU.  ValueError for a norm that is none;
    MrcError where the library refuses."""
    norm = check_filter_norm(norm, "filterbank_line_weights")
    points = np.ascontiguousarray(np.asarray(points_hz, dtype=np.float64).reshape(-1))
    n = int(points.size) - 2
    lo, hi = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    count = np.zeros(1, np.int64)

    def call(cap, weight):
        rc = lib.mrc_filterbank_line_weights(float(sample_rate), int(a), int(b), n, points.ctypes.data, norm, lo.ctypes.data,
                                             hi.ctypes.data, cap, weight, count.ctypes.data)
        if rc:
            err = _lib.MrcError("libmrc_hip error %d: %s" % (rc, lib.mrc_last_error(None).decode()))
            err.code = rc
            raise err

    call(0, None)                                                   # sizes only
    weight = np.zeros(max(int(count[0]), 1), np.float64)
    call(int(count[0]), weight.ctypes.data)
    at = np.concatenate([[0], np.cumsum(hi[:n] - lo[:n])])
    return lo[:n], hi[:n], [weight[at[q]:at[q + 1]] for q in range(n)]


MAX_STFT_POINTS = _lib.MRC_MAX_STFT_POINTS
STFT_OUTPUTS = {"complex": _lib.MRC_STFT_COMPLEX, "power": _lib.MRC_STFT_POWER, "bank": _lib.MRC_STFT_BANK}


def stft_points_ok(n_fft):
    """the library's rule for n_fft: an even int in 16..MAX_STFT_POINTS with no prime factor other than 2, 3 and 5"""
    if not _is_int(n_fft) or not 16 <= int(n_fft) <= MAX_STFT_POINTS or int(n_fft) % 2:
        return False
    n = int(n_fft)
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def hann_window(n, periodic=True):
    """float64 [n]: 0.5 - 0.5 cos(2 pi k / n) (periodic: what torch.hann_window(n) gives) or cos(2 pi k / (n - 1))
    (symmetric).  n an int >= 1, else ValueError"""
    if not _is_int(n) or int(n) < 1:
        raise ValueError("hann_window: n must be an int >= 1, got %r" % (n,))
    n = int(n)
    den = n if periodic else n - 1
    if den == 0:
        return np.ones(1, np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / den)


def padded_window(win, n_fft):
    """a window shorter than n_fft centred in n_fft points, as torch.stft(win_length=len(win)) does: (n_fft - len(win)) // 2
    zeros in front, the rest behind -> float64 [n_fft].  ValueError for a window that is not 1-D, empty or longer than n_fft"""
    try:
        w = np.asarray(win, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("padded_window: win must be a 1-D array of taps, got %r" % (win,))
    if not _is_int(n_fft) or w.ndim != 1 or not 1 <= w.size <= int(n_fft):
        raise ValueError("padded_window: win must hold 1 to n_fft = %r taps in one dimension, got shape %s" % (n_fft, w.shape))
    out = np.zeros(int(n_fft), np.float64)
    left = (int(n_fft) - w.size) // 2
    out[left:left + w.size] = w
    return out


def mel_bin_weights(n_fft, sample_rate, points_hz, norm=None):
    """The matrix of a triangular filter bank on STFT bins -> float64 [n_filters][n_fft // 2 + 1] for stft_window(bank=):
    filter q is the triangle over points_hz[q], [q + 1], [q + 2] (mel_points gives them) sampled AT the bin centre
    frequencies f_k = k sample_rate / n_fft: max(0, min((f_k - a) / (b - a), (c - f_k) / (c - b))).  norm="slaney": each
    filter times 2 / (c - a).  This is the rule of torchaudio's melscale_fbanks written out.  Unlike the line-based
    filterbank_line_weights it samples and does not average: a filter narrower than a bin may hold no bin at all and then
    reads 0 -- the STFT's own behaviour.  NumPy only.  ValueError as check_filter_points and check_filter_norm raise it, for
    an n_fft that is no even int >= 2 and a sample rate that is not a positive finite number."""
    what = "mel_bin_weights"
    points = check_filter_points(points_hz, what)
    slaney = check_filter_norm(norm, what) == _lib.MRC_FILTER_NORM_SLANEY
    if not _is_int(n_fft) or int(n_fft) < 2 or int(n_fft) % 2:
        raise ValueError("%s: n_fft must be an even int >= 2, got %r" % (what, n_fft))
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float, np.integer, np.floating)) or \
            not np.isfinite(sample_rate) or not sample_rate > 0:
        raise ValueError("%s: sample_rate must be a positive finite number, got %r" % (what, sample_rate))
    f = np.arange(int(n_fft) // 2 + 1, dtype=np.float64) * float(sample_rate) / float(int(n_fft))
    a, b, c = points[:-2, None], points[1:-1, None], points[2:, None]
    w = np.maximum(0.0, np.minimum((f[None, :] - a) / (b - a), (c - f[None, :]) / (c - b)))
    if slaney:
        w = w * (2.0 / (c - a))
    return np.ascontiguousarray(w)


def check_stft(n_fft, hop, n_frames, frame_window=None, bank=None, output="power", what="stft_window"):
    """the STFT arguments of stft_window -> (n_fft, hop, n_frames, window float64 [n_fft], bank float64 [filters][bins] or
    None, MRC_STFT_* mode), else ValueError: n_fft under stft_points_ok's rule; hop an int >= 1; n_frames an int >= 0 with
    (n_frames - 1) hop + n_fft <= 2^40; frame_window None (the periodic Hann) or n_fft finite taps; output "power",
    "complex" or "bank"; bank a finite [1..MAX_BANDS][n_fft // 2 + 1] matrix with output="bank" and None otherwise"""
    if not stft_points_ok(n_fft):
        raise ValueError("%s: n_fft must be an even int in 16..%d with no prime factor other than 2, 3 and 5, got %r"
                         % (what, MAX_STFT_POINTS, n_fft))
    n_fft = int(n_fft)
    for name, v, least in (("n_frames", n_frames, 0), ("hop", hop, 1)):
        if not _is_int(v) or int(v) < least:
            raise ValueError("%s: %s must be an int >= %d, got %r" % (what, name, least, v))
    hop, n_frames = int(hop), int(n_frames)
    if n_frames and (n_frames - 1) * hop + n_fft > 1 << 40:
        raise ValueError("%s: (n_frames - 1) * hop + n_fft must not exceed 2^40, got %d frames at hop %d" % (what, n_frames, hop))
    if not isinstance(output, str) or output not in STFT_OUTPUTS:
        raise ValueError('%s: output must be "power", "complex" or "bank", got %r' % (what, output))
    if frame_window is None:
        window = hann_window(n_fft)
    else:
        try:
            window = np.ascontiguousarray(np.asarray(frame_window, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError("%s: frame_window must be %d float taps, got %r" % (what, n_fft, frame_window))
        if window.shape != (n_fft,):
            raise ValueError("%s: frame_window must hold n_fft = %d taps (padded_window centres a shorter one), got shape %s"
                             % (what, n_fft, window.shape))
        if not np.all(np.isfinite(window)):
            raise ValueError("%s: frame_window must be finite, tap %d is not" % (what, int(np.flatnonzero(~np.isfinite(window))[0])))
    if output != "bank":
        if bank is not None:
            raise ValueError('%s: bank goes with output="bank", got output=%r' % (what, output))
        return n_fft, hop, n_frames, window, None, STFT_OUTPUTS[output]
    if bank is None:
        raise ValueError('%s: output="bank" needs a bank [filters][%d] (mel_bin_weights)' % (what, n_fft // 2 + 1))
    try:
        matrix = np.ascontiguousarray(np.asarray(bank, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("%s: bank must be a float matrix [filters][%d], got %r" % (what, n_fft // 2 + 1, bank))
    if matrix.ndim != 2 or not 1 <= matrix.shape[0] <= MAX_BANDS or matrix.shape[1] != n_fft // 2 + 1:
        raise ValueError("%s: bank must be [1..%d filters][n_fft // 2 + 1 = %d bins], got shape %s"
                         % (what, MAX_BANDS, n_fft // 2 + 1, matrix.shape))
    if not np.all(np.isfinite(matrix)):
        raise ValueError("%s: bank must be finite" % what)
    return n_fft, hop, n_frames, window, matrix, STFT_OUTPUTS[output]


def _formats():
    import torch
    return {torch.int16: _lib.MRC_WINDOW_PCM16, torch.float32: _lib.MRC_WINDOW_F32, torch.float64: _lib.MRC_WINDOW_F64}


class WindowRows(collections.namedtuple("WindowRows", "rate_divisor mix resample channels bands speeds irs offsets files starts gains routes spans",
                                        defaults=(None, None))):
    """The checked row arguments of a window call: rate_divisor an int, mix None or its MRC_MIX_* value, resample None or
    (up, down, zeros, rolloff), channels as given (1 under a mix), bands None or (edges, gains [terms][n_bands]), speeds None or
    (ratios, zeros, rolloff, index int32 [terms]), irs None or int32 [terms], offsets int64 [rows + 1], files, starts and gains
    flat and contiguous.  decode_window's items are rows of one term each at gain 1.0.  routes: None, or check_routes' (gains
    float64 [terms][C], irs int32 [terms][C]) of a routed call -- gains and irs are then not looked at, and channels is 1, what
    every term gives.  spans: None, or check_spans' (span_first, span_len, fade_in, fade_out), int64 [terms] each."""
    __slots__ = ()


def window_entry(store, rows, caller, window, channels, fmt, out, stream, stft=None):
    """The library entry a window call goes to and its arguments -> (name, args, keep): the ONE place that names the
    mrc_pac_store_decode_window* entries and mrc_pac_store_stft_window.  rows: a WindowRows; caller: "decode_window",
    "decode_window_sum" or "stft_window"; store, out and stream: the store's pointer, the output's and the stream as ints or
    None (no device is needed to ask); stft: stft_window's (n_fft, window array, n_frames, hop, mode, matrix or None).  keep
    holds the arrays made here whose pointers args carries.  The entry per combination, first match:
        routes given: stft_window            mrc_pac_store_stft_window_routed  (route_gain and route_ir in place of gain and
                      else                   ..._routed                         ir_of; `channels` is the routes' last axis)
        spans given:  stft_window            mrc_pac_store_stft_window_spans   (the reverb / STFT entry's arguments with the
                      else                   ..._spans                          four span arrays behind ir_of)
        stft_window                          mrc_pac_store_stft_window (ratios default to the one base ratio, ir_of to -1)
        ir_index given                       ..._reverb
        speeds given                         ..._speeds
        band_gains given                     ..._shaped
        decode_window_sum                    ..._sum
        decode_window: resample given        ..._resampled
                       mix given             ..._mix
                       rate_divisor > 1      ..._reduced
                       else                  mrc_pac_store_decode_window"""
    pad = lambda a: a.ctypes.data if a.size else None
    mix = _lib.MRC_MIX_EACH if rows.mix is None else rows.mix
    n = rows.offsets.size - 1
    terms = (n, rows.offsets.ctypes.data, pad(rows.files), pad(rows.starts), pad(rows.gains))
    tail = (window, channels, fmt, out or None, stream or None)
    up, down, zeros, rolloff = rows.resample if rows.resample is not None else (1, 1, RESAMPLE_ZEROS, RESAMPLE_ROLLOFF)
    if rows.bands is None:
        bands = (0, None, None)
    else:
        bands = (rows.bands[0].size - 1, rows.bands[0].ctypes.data, pad(rows.bands[1]))
    if stft is not None or rows.irs is not None or rows.speeds is not None or rows.routes is not None or rows.spans is not None:   # ... take a list of ratios
        ratios, zeros, rolloff, index = rows.speeds or ([(up, down)], zeros, rolloff, np.zeros(rows.files.size, np.int32))
        ups = np.ascontiguousarray([r[0] for r in ratios], dtype=np.int32)
        downs = np.ascontiguousarray([r[1] for r in ratios], dtype=np.int32)
        irs = rows.irs if rows.irs is not None else np.full(rows.files.size, -1, np.int32)
        head = (store, rows.rate_divisor, mix, len(ratios), ups.ctypes.data, downs.ctypes.data, zeros, rolloff) + bands + terms + (pad(index),)
        keep = (ups, downs, index, irs)
        if stft is not None:
            n_fft, frame_window, n_frames, hop, mode, matrix = stft
            own = (n_fft, frame_window.ctypes.data, n_frames, hop, mode, 0 if matrix is None else matrix.shape[0],
                   None if matrix is None else matrix.ctypes.data)
        if rows.routes is not None:                          # (gain and ir_of leave, the two route arrays stand in their place)
            routed = head[:-2] + (pad(index), pad(rows.routes[0]), pad(rows.routes[1]))
            if stft is not None:
                return "mrc_pac_store_stft_window_routed", routed + own + tail[1:], keep
            return "mrc_pac_store_decode_window_routed", routed + tail, keep
        if rows.spans is not None:
            spans = tuple(pad(a) for a in rows.spans)
            if stft is not None:
                return "mrc_pac_store_stft_window_spans", head + (pad(irs),) + spans + own + tail[1:], keep
            return "mrc_pac_store_decode_window_spans", head + (pad(irs),) + spans + tail, keep
        if stft is not None:
            return "mrc_pac_store_stft_window", head + (pad(irs),) + own + tail[1:], keep
        if rows.irs is not None:
            return "mrc_pac_store_decode_window_reverb", head + (pad(irs),) + tail, keep
        return "mrc_pac_store_decode_window_speeds", head + tail, keep
    single = (store, rows.rate_divisor, mix, up, down, zeros, rolloff)
    if rows.bands is not None:
        return "mrc_pac_store_decode_window_shaped", single + bands + terms + tail, ()
    if caller == "decode_window_sum":
        return "mrc_pac_store_decode_window_sum", single + terms + tail, ()
    items = (n, pad(rows.files), pad(rows.starts))
    if rows.resample is not None:
        return "mrc_pac_store_decode_window_resampled", single + items + tail, ()
    if rows.mix is not None:
        return "mrc_pac_store_decode_window_mix", (store, rows.rate_divisor, mix) + items + (window,) + tail[2:], ()
    if rows.rate_divisor > 1:
        return "mrc_pac_store_decode_window_reduced", (store, rows.rate_divisor) + items + tail, ()
    return "mrc_pac_store_decode_window", (store,) + items + tail, ()


class PacStore:
    """bufs: a list of bytes-like `.pac` files carrying the handle's codec parameters, mono and stereo mixed at will.
    .n_channels, .n_samples (per channel, as Handle.decode_pac_pcm16 returns them), .n_blocks: one NumPy value per file;
    .device_bytes: the device memory the store holds.  Close the store before its handle: a store whose handle has been
    closed refuses every call (MrcError)."""

    def __init__(self, handle, bufs):
        if isinstance(bufs, (bytes, bytearray, memoryview, np.ndarray)):
            bufs = [bufs]
        n = len(bufs)
        sizes = np.fromiter((len(b) for b in bufs), dtype=np.int64, count=n)
        file_offset = np.zeros(n + 1, np.int64)
        np.cumsum(sizes, out=file_offset[1:])
        data = np.frombuffer(b"".join(bytes(b) for b in bufs), np.uint8) if n else np.zeros(1, np.uint8)
        if not data.size:
            data = np.zeros(1, np.uint8)
        self._handle = handle
        self._levels = {}                # levels() of every file, per (rate_divisor, mix)
        self._ir_lengths = np.zeros(0, np.int64)   # set_impulse_responses: the bank's lengths (mrc_pac_store_ir_info)
        self._s = C.c_void_p()
        handle._check(lib.mrc_pac_store_create(handle._h, n, data.ctypes.data, file_offset.ctypes.data, C.byref(self._s)))
        self.n_channels = np.zeros(n, np.int32)
        self.n_samples = np.zeros(n, np.int64)
        self.n_blocks = np.zeros(n, np.int64)
        nf, dev_bytes = C.c_int64(), C.c_int64()
        pad = lambda a: a.ctypes.data if n else None
        handle._check(lib.mrc_pac_store_info(self._s, C.byref(nf), pad(self.n_channels), pad(self.n_samples),
                                             pad(self.n_blocks), C.byref(dev_bytes)))
        self.device_bytes = dev_bytes.value

    def close(self):
        if getattr(self, "_s", None):
            lib.mrc_pac_store_destroy(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.n_channels)

    def n_samples_at(self, rate_divisor):
        """.n_samples at 1 / rate_divisor of the sample rate: n_samples // rate_divisor per file (exact for every divisor the
        library accepts for the handle's block lengths)"""
        return self.n_samples // check_rate_divisor(rate_divisor, "n_samples_at")

    def n_samples_resampled(self, up, down, rate_divisor=1):
        """the output samples of decode_window(resample=(up, down), rate_divisor=) that lie inside each file:
        ceil(n_samples_at(rate_divisor) * up / down)"""
        n = self.n_samples_at(rate_divisor)
        for name, v in (("up", up), ("down", down)):
            if not _is_int(v) or int(v) < 1:
                raise ValueError("n_samples_resampled: %s must be a positive int, got %r" % (name, v))
        return -((-n * int(up)) // int(down))

    def _channels_named(self, files, channels):
        """channels, or for None the largest channel count among the files named that the store has (none: 1)"""
        if channels is not None:
            return channels
        inside = files[(files >= 0) & (files < len(self))]
        return int(self.n_channels[inside].max()) if inside.size else 1

    def _out_tensor(self, what, shape, dtype, out, stream):
        """-> (out, stream): the contiguous tensor of that shape and dtype on the handle's device (given: it must be that,
        else ValueError) and the stream (None: torch's current one)"""
        import torch
        dev = torch.device("cuda", self._handle.cfg.device_id)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or out.device != dev \
                or not out.is_contiguous():
            raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s" % (what, dtype, shape, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        return out, stream

    def _out_side(self, what, files, channels, shape, dtype, out, stream, one_or_two=False):
        """the output side of decode_window, decode_window_sum and stft_window -> (channels, out, stream): channels (None: as
        _channels_named; one_or_two: anything but 1 or 2 is a ValueError), then _out_tensor over shape(channels)"""
        channels = self._channels_named(files, channels)
        if one_or_two and (not _is_int(channels) or int(channels) not in (1, 2)):
            raise ValueError("%s: channels must be None, 1 or 2, got %r" % (what, channels))
        channels = int(channels)
        return (channels,) + self._out_tensor(what, shape(channels), dtype, out, stream)

    def _window_out(self, what, n, files, window, channels, dtype, out, stream):
        """decode_window's and decode_window_sum's -> (format, channels, out, stream): dtype (None: int16, or out's) and
        _out_side over [n][channels][window]"""
        import torch
        if dtype is None:
            dtype = torch.int16 if out is None else out.dtype
        fmt = _formats().get(dtype)
        if fmt is None:
            raise ValueError("%s: dtype must be torch.int16, torch.float32 or torch.float64, got %s" % (what, dtype))
        return (fmt,) + self._out_side(what, files, channels, lambda c: (n, c, max(window, 0)), dtype, out, stream)

    def _call_window(self, rows, caller, window, channels, fmt, out, stream, stft=None):
        """window_entry's choice, called (its arrays live until the call returns); -> out"""
        name, args, _keep = window_entry(self._s, rows, caller, window, channels, fmt, out.data_ptr() if out.numel() else None, stream, stft)
        self._handle._check(getattr(lib, name)(*args))
        return out

    def _band_args(self, what, band_gains, band_edges_hz, unit_shape):
        """band_gains / band_edges_hz of a window call -> None, or (edges float64 [n_bands + 1], gains float64 [units][n_bands]);
        ValueError as check_band_edges and check_band_gains raise it"""
        if band_gains is None:
            check_band_gains(None, unit_shape, 0, what, band_edges_hz)
            return None
        edges = critical_band_edges(self._handle.cfg.sample_rate) if band_edges_hz is None else check_band_edges(band_edges_hz, what)
        return edges, check_band_gains(band_gains, unit_shape, edges.size - 1, what)

    def _speed_args(self, what, resample, speed_factors, speed_index, unit_shape):
        """speed_factors / speed_index of a window call -> None, or (ratios [(up, down)], zeros, rolloff, index int32 [units]);
        ValueError as speed_ratios and check_speed_index raise it, and for one of the two given without the other"""
        if speed_factors is None and speed_index is None:
            return None
        if speed_factors is None or speed_index is None:
            raise ValueError("%s: speed_factors and speed_index go together, got only %s"
                             % (what, "speed_index" if speed_factors is None else "speed_factors"))
        ratios, zeros, rolloff = _speed_list(resample, speed_factors, what)
        return ratios, zeros, rolloff, check_speed_index(speed_index, unit_shape, len(ratios), what)

    def set_impulse_responses(self, irs):
        """mrc_pac_store_set_irs: the store's bank of room impulse responses for ir_index= -- a list of 1-D arrays of 1 to
        MAX_IR_TAPS finite taps each, SAMPLED AT THE OUTPUT RATE of the terms that will name them (ir_at_rate brings a recorded
        response there).  The call replaces the previous bank; None or [] drops it.  The partitions' transforms are computed
        once on the device and stay resident (32 bytes per tap, lengths rounded up to REVERB_BLOCK).  A bank that is not such
        a list is a ValueError before any library call; a failed allocation (MrcError) leaves the store without a bank."""
        offsets, taps = check_impulse_responses(irs)
        n = offsets.size - 1
        try:
            self._handle._check(lib.mrc_pac_store_set_irs(self._s, n, offsets.ctypes.data, taps.ctypes.data if n else None))
        finally:
            count = C.c_int64()
            self._handle._check(lib.mrc_pac_store_ir_info(self._s, C.byref(count), None))
            lengths = np.zeros(count.value, np.int64)
            self._handle._check(lib.mrc_pac_store_ir_info(self._s, None, lengths.ctypes.data if count.value else None))
            self._ir_lengths = lengths

    @property
    def impulse_response_lengths(self):
        """the taps of every impulse response of the bank, int64 [n_irs] (mrc_pac_store_ir_info); empty without a bank"""
        return self._ir_lengths.copy()

    def reverb_ms(self):
        """mrc_pac_store_reverb_ms: the device time of the last ir_index= call's two kernels, summed over its slabs"""
        ms = np.zeros(2, np.float64)
        self._handle._check(lib.mrc_pac_store_reverb_ms(self._s, ms.ctypes.data))
        return {"forward": float(ms[0]), "fold": float(ms[1])}

    def source_spans(self, starts, window, ratios, index, rate_divisor=1):
        """Where the units of decode_window(speed_factors=, speed_index=) lie in the signal at 1 / rate_divisor of the sample
        rate -> (first, length), int64 arrays of starts' shape: unit k, read at ratios[index[k]] = (up, down) (speed_ratios
        gives the list), has its `window` outputs over the intermediate samples [first, first + length), first =
        floor(starts[k] down / up) and length = ceil(window down / up) -- without the filter's tails.  Those are the
        coordinates of levels(rate_divisor): LevelMap.gains_for_snr, .gains_to and .sample_starts can be asked about a sped-up
        term with (first, length) in place of (start, window).  No library call.  ValueError for ratios that are not pairs
        of positive ints, an index outside the list or of another shape, a negative window."""
        what = "source_spans"
        check_rate_divisor(rate_divisor, what)
        starts = np.asarray(starts, dtype=np.int64)
        if not isinstance(ratios, (tuple, list)) or not ratios or \
                not all(isinstance(r, (tuple, list)) and len(r) == 2 and all(_is_int(v) and int(v) >= 1 for v in r) for r in ratios):
            raise ValueError("%s: ratios must be a list of (up, down) pairs of positive ints, got %r" % (what, ratios))
        if not _is_int(window) or int(window) < 0:
            raise ValueError("%s: window must be an int >= 0, got %r" % (what, window))
        idx = check_speed_index(index, starts.shape, len(ratios), what).reshape(starts.shape)
        up = np.array([int(r[0]) for r in ratios], np.int64)[idx]
        down = np.array([int(r[1]) for r in ratios], np.int64)[idx]
        return np.floor_divide(starts * down, up), -np.floor_divide(-int(window) * down, up)

    def decode_window(self, files, starts, window, channels=None, dtype=None, out=None, stream=None, rate_divisor=1,
                      mix=None, resample=None, band_gains=None, band_edges_hz=None, speed_factors=None, speed_index=None,
                      ir_index=None):
        """Item i = samples [starts[i], starts[i] + window) of file files[i], zeros where that leaves the file (starts may be
        negative or past the end) -> a torch tensor [n][channels][window] on the handle's device.  dtype: torch.int16 (the
        default: the codes Handle.decode_pac_pcm16 writes, bit for bit), torch.float64 (the overlap-added signal before the
        PCM quantiser, bit for bit) or torch.float32 (that value converted once).  channels: 1 or 2; None: the largest channel
        count among the items' files.  A mono file fills both channels of a two-channel call; a stereo file in a one-channel
        call is refused.  out: a contiguous tensor of that shape, dtype and device to write into (else ValueError, before any
        library call).  stream: a raw stream; None: torch's current stream on the device.  The call returns when the result
        is there.
        rate_divisor: 1, 2 or 4 (else ValueError, before any library call).  2 or 4: starts and window count samples at that
        fraction of the sample rate (n_samples_at), sample m being the band-limited signal at full-rate time
        D m + (D - 1) / 2; torch.float64 is then the reduced overlap-added signal, torch.float32 and torch.int16 its
        conversions.  A divisor the handle's block shapes do not divide by is refused by the library (MrcError).
        mix: None, or "mid", "left" or "right": one channel of every item, [n][1][window], a stereo file's left or right
        channel (the bits of that channel of the two-channel call) or its mid (L + R) / 2, formed on the MDCT lines before
        the one inverse transform (torch.float64: that plane; the other dtypes its conversions); a mono file gives its
        channel.  channels must then be None or 1, and any other mix is a ValueError, before any library call.
        resample: None, or (up, down) or (up, down, zeros, rolloff) (mrc_pac_store_decode_window_resampled): the signal of
        this call at that rate_divisor and mix, at up / down of its rate through a Hann-windowed sinc (resample_taps; zeros
        16, rolloff 0.9475 unless given) that reads the float64 planes on the device -- 48 kHz files at 16 kHz:
        rate_divisor=2, resample=(2, 3), which resample_plan(48000, 16000) says.  starts and window then count OUTPUT
        samples, output n at time n down / up of the rate_divisor signal (n_samples_resampled of them lie inside a file);
        torch.float64 is the fold defined in the header, bit for bit, the other dtypes its conversions.  A ratio of 1 after
        reduction is the call without resample.  A ratio outside [1 / 8, 8], terms above 1024 after reduction, zeros outside
        1..64 and rolloff outside [0.5, 1] are ValueErrors, before any library call.
        band_gains: None, or float64 [n][n_bands] ([n_bands]: the same row for every item): the spectrum of item i changed on its
        MDCT lines (mrc_pac_store_decode_window_shaped, as one-term rows at gain 1.0) -- every decoded line whose frequency lies
        in band q = [band_edges_hz[q], band_edges_hz[q + 1]) is multiplied once by band_gains[i][q] before the inverse
        transform that runs anyway; lines outside every band are left alone; all channels of an item share its row.  Zero
        and negative gains are allowed (a telephone band, an EQ tilt from gains_from_db, masks from band_mask_gains).
        band_edges_hz: 2 to 257 increasing frequencies from 0 up; None: critical_band_edges(sample_rate), the codec's own
        bands.  The line frequencies are the full-rate block's at every rate_divisor (bands above the reduced Nyquist are
        ignored), and everything else of the call -- mix, resample, dtype, zeros outside the file -- is unchanged: gains of
        1.0 give the bits of the call without band_gains, gains that are all one power of two that multiple of its float64
        window.  Not an LTI filter: where neighbouring lines get different gains the time-domain aliasing of adjacent blocks
        no longer cancels exactly -- smooth gain curves are clean, a brick-wall edge leaves a small aliasing residue near the
        edge frequency (DESIGN.md has figures).  A wrong shape, values that are not finite numbers and band_edges_hz without
        band_gains are ValueErrors, before any library call.
        speed_factors, speed_index: None, or a list of 1 to 8 (num, den) pairs and an int array [n] of indices into it
        (mrc_pac_store_decode_window_speeds, as one-term rows at gain 1.0): item i is read at speed num / den -- above 1 plays
        faster -- that is at resample's base ratio (None: 1 / 1) divided by its speed, reduced (speed_ratios gives the list).
        Item i is then, bit for bit, what decode_window(resample=that ratio) gives for it: starts and window count output
        samples at the item's OWN ratio, and a ratio of 1 is the call without a filter.  Speed perturbation of a batch --
        0.9x, 1.0x, 1.1x drawn per item -- is one call, one plan and one output kernel.  Only one of the two given, a wrong
        shape, an index outside the list, a factor that is not a pair of positive ints and a combined ratio outside what
        resample takes (named with its reduced terms) are ValueErrors, before any library call.
        ir_index: None (this call as it always was), or an int array [n]: item i convolved with impulse response ir_index[i] of
        the store's bank (set_impulse_responses), -1 for none (mrc_pac_store_decode_window_reverb, as one-term rows at gain
        1.0).  The response is sampled at the item's OUTPUT rate and applied last: y[t] = sum_j h[j] x[t - j] over the
        signal this call gives otherwise, which is zero outside the file -- so the item rings len(h) - 1 samples past the
        file's end.  An item with -1 is this call's window bit for bit; a convolved item is float64 overlap-save within the
        tolerance the header states, and independent to the bit of the batch it is in.  A wrong shape and an index that is
        neither -1 nor inside the bank are ValueErrors, before any library call."""
        rate_divisor = check_rate_divisor(rate_divisor)
        mix = check_mix(mix, channels)
        resample_arg, resample = resample, check_resample(resample)
        if mix is not None:
            channels = 1
        files = np.ascontiguousarray(np.asarray(files, dtype=np.int64).reshape(-1))
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
        if files.shape != starts.shape:
            raise ValueError("decode_window: one start per file index (%d files, %d starts)" % (files.size, starts.size))
        n, window = files.size, int(window)
        bands = self._band_args("decode_window", band_gains, band_edges_hz, (n,))
        speeds = self._speed_args("decode_window", resample_arg, speed_factors, speed_index, (n,))
        irs = None if ir_index is None else check_ir_index(ir_index, (n,), self._ir_lengths.size)
        fmt, channels, out, stream = self._window_out("decode_window", n, files, window, channels, dtype, out, stream)
        rows = WindowRows(rate_divisor, mix, resample, channels, bands, speeds, irs, np.arange(n + 1, dtype=np.int64), files, starts,
                          np.ones(n, np.float64))
        return self._call_window(rows, "decode_window", window, channels, fmt, out, stream)

    def decode_window_sum(self, files, starts, gains, window, item_offsets=None, channels=None, dtype=None, out=None, stream=None,
                          rate_divisor=1, mix=None, resample=None, band_gains=None, band_edges_hz=None, speed_factors=None,
                          speed_index=None, ir_index=None, span_first=None, span_len=None, fade_in=None, fade_out=None):
        """mrc_pac_store_decode_window_sum -> a torch tensor [n][channels][window] on the handle's device: item i is the sum
        over its terms k, IN THE ORDER GIVEN, of gains[k] * (the float64 window decode_window gives for files[k], starts[k]
        at this rate_divisor, mix and resample), folded from +0.0 with every product rounded once, then added -- speech over
        noise, an event inside a background, mixup -- in one call that writes no per-term window.  torch.float64 is that sum,
        bit for bit; torch.float32 and torch.int16 (the default, saturating at full scale) are conversions of it.
        files, starts, gains: 2-D [n][K] (every item has K terms), or 1-D [terms] with item_offsets [n + 1] (item i's terms are
        [item_offsets[i], item_offsets[i + 1]); an item without terms is zeros).  A start may be negative or past the end:
        the term reads zeros there, which is how a term is placed inside the window.  levels.LevelMap.gains_for_snr and
        .gains_to give factors without decoding anything.  A one-term item with gain 1.0 is decode_window's window.
        window, channels, dtype, out, stream, rate_divisor, mix, resample: as decode_window's (with resample, starts and window
        count output samples).  Shapes that do not agree, offsets that do not start at 0 or that decrease and gains that are
        not finite are ValueErrors, like decode_window's argument errors, before any library call.
        band_gains, band_edges_hz: as decode_window's, PER TERM: band_gains has the shape of files plus a last axis [n_bands]
        ([n_bands] alone: every term), and term k's lines are multiplied by its row before its inverse transform
        (mrc_pac_store_decode_window_shaped) -- a telephone band for the speech term and none for the noise is a row of gains
        and a row of ones.  The fold over the terms is unchanged.
        speed_factors, speed_index: as decode_window's, PER TERM (mrc_pac_store_decode_window_speeds): speed_index has the shape
        of files, and term k is the float64 window decode_window gives at ITS ratio -- the speech term at a drawn speed over a
        noise term at speed 1 is one call.  starts and window count output samples at the term's own ratio;
        source_spans says where a term lies in the source, for LevelMap's gains.  Per-term band_gains still apply.
        ir_index: as decode_window's, PER TERM (mrc_pac_store_decode_window_reverb): it has the shape of files, and term k is
        convolved with impulse response ir_index[k] of the store's bank before it is weighted and added, -1 for none -- speech
        through a room over dry noise is one call.  It composes with resample, speed_factors / speed_index, band_gains, mix
        and rate_divisor: the response acts last, at the term's output rate.  None: this call as it always was.
        span_first, span_len, fade_in, fade_out: PER TERM (mrc_pac_store_decode_window_spans), the shape of files (a fade may be
        a scalar, every term, or None, 0): term k sounds only at row samples span_first[k] <= t < span_first[k] + span_len[k], its
        first fade_in and last fade_out samples there on a linear ramp ((2 j + 1) / (2 fade) at the j-th sample from the end it
        fades at), and adds nothing elsewhere.  starts[k] stays the source position at row sample 0, so the piece from source
        sample p placed at row sample a is starts = p - a, span_first = a; concat_spans lays pieces end to end.  Only the blocks
        under a term's span are parsed and synthesised.  Spans compose with every argument above (the response acts after the
        envelope, a gated piece rings on); check_spans makes the ValueErrors.  None: this call as it always was."""
        what = "decode_window_sum"
        rows = self._sum_rows(what, files, starts, gains, item_offsets, channels, rate_divisor, mix, resample, band_gains, band_edges_hz,
                              speed_factors, speed_index, ir_index)
        rows = rows._replace(spans=check_spans(span_first, span_len, fade_in, fade_out, np.shape(files), what))
        n, window = rows.offsets.size - 1, int(window)
        fmt, channels, out, stream = self._window_out(what, n, rows.files, window, rows.channels, dtype, out, stream)
        return self._call_window(rows, what, window, channels, fmt, out, stream)

    def decode_window_routed(self, files, starts, route_gains, route_irs, window, item_offsets=None, dtype=None, out=None,
                             stream=None, rate_divisor=1, mix=None, resample=None, band_gains=None, band_edges_hz=None,
                             speed_factors=None, speed_index=None):
        """mrc_pac_store_decode_window_routed -> a torch tensor [n][C][window] on the handle's device: rows of C OUTPUT channels
        from terms that each give ONE channel, with a gain and a response per (term, output channel) -- an utterance through the
        C microphones of a room (array_routes builds the routes), or the reverberant mixture, the dry speech and the noise
        alone of the same terms as three channels -- in one call that parses, synthesises and transforms every term once.
        files, starts, item_offsets: as decode_window_sum's ([n][K], or 1-D with item_offsets).  route_gains, route_irs: the
        shape of files plus a last axis [C], 1 <= C <= MAX_ROUTE_CHANNELS; route_irs[k][c] is ROUTE_NONE (term k does not reach
        channel c), -1 (dry) or an index into the store's bank (set_impulse_responses).
        Channel c of item i is, bit for bit and in every dtype, decode_window_sum(..., ir_index=)[i][0] over the item's terms whose
        route to c is not ROUTE_NONE, in the order given, with gains route_gains[:, c] and ir_index route_irs[:, c], every
        other argument equal; a channel no term reaches is +0.0.  Nothing depends on which other channels the call has.
        mix: "mid", "left" or "right"; None only where every file named is mono (the library refuses a stereo file then).
        window, dtype, out, stream, rate_divisor, resample, band_gains, band_edges_hz, speed_factors, speed_index: as
        decode_window_sum's, per term.  Routes of another shape, gains that are not finite and an index below ROUTE_NONE or
        outside the bank are ValueErrors (check_routes), before any library call.  route_info() says what the call shared."""
        what = "decode_window_routed"
        files, starts = self._routed_terms(what, files, starts)
        rows = self._sum_rows(what, files, starts, np.ones(files.shape, np.float64), item_offsets, None, rate_divisor, mix, resample,
                              band_gains, band_edges_hz, speed_factors, speed_index, None)
        routes = check_routes(route_gains, route_irs, rows.files.size, self._ir_lengths.size, what)
        rows = rows._replace(channels=1, routes=routes)
        n, window, n_ch = rows.offsets.size - 1, int(window), routes[0].shape[1]
        import torch
        if dtype is None:
            dtype = torch.int16 if out is None else out.dtype
        fmt = _formats().get(dtype)
        if fmt is None:
            raise ValueError("%s: dtype must be torch.int16, torch.float32 or torch.float64, got %s" % (what, dtype))
        out, stream = self._out_tensor(what, (n, n_ch, max(window, 0)), dtype, out, stream)
        return self._call_window(rows, what, window, n_ch, fmt, out, stream)

    @staticmethod
    def _routed_terms(what, files, starts):
        """files and starts of a routed call as int64 arrays of one shape, else ValueError (a routed call has no gains to name)"""
        files, starts = np.asarray(files, dtype=np.int64), np.asarray(starts, dtype=np.int64)
        if files.shape != starts.shape:
            raise ValueError("%s: files and starts must have one shape, got %s and %s" % (what, files.shape, starts.shape))
        return files, starts

    def route_info(self):
        """mrc_pac_store_route_info: what the last routed call (decode_window_routed, stft_window(route_gains=)) did, summed
        over its slabs -- forward_segments transformed (one source per term and distinct response length among its wet routes),
        inverse_transforms (one per wet route and output block) and the spectra_bytes written"""
        counts = np.zeros(3, np.int64)
        self._handle._check(lib.mrc_pac_store_route_info(self._s, counts.ctypes.data))
        return {"forward_segments": int(counts[0]), "inverse_transforms": int(counts[1]), "spectra_bytes": int(counts[2])}

    def _sum_rows(self, what, files, starts, gains, item_offsets, channels, rate_divisor, mix, resample, band_gains, band_edges_hz,
                  speed_factors, speed_index, ir_index):
        """the row arguments of decode_window_sum and stft_window, checked in the one order -> a WindowRows; ValueError as
        decode_window_sum documents"""
        rate_divisor = check_rate_divisor(rate_divisor, what)
        mix = check_mix(mix, channels, what)
        resample_arg, resample = resample, check_resample(resample, what)
        if mix is not None:
            channels = 1
        files, starts = np.asarray(files, dtype=np.int64), np.asarray(starts, dtype=np.int64)
        gains = np.asarray(gains, dtype=np.float64)
        if not (files.shape == starts.shape == gains.shape):
            raise ValueError("%s: files, starts and gains must have one shape, got %s, %s and %s"
                             % (what, files.shape, starts.shape, gains.shape))
        bands = self._band_args(what, band_gains, band_edges_hz, files.shape)
        speeds = self._speed_args(what, resample_arg, speed_factors, speed_index, files.shape)
        irs = None if ir_index is None else check_ir_index(ir_index, files.shape, self._ir_lengths.size, what)
        if item_offsets is None:
            if files.ndim != 2:
                raise ValueError("%s: files, starts and gains must be [n][K], or 1-D with item_offsets; got shape %s" % (what, files.shape))
            offsets = np.arange(files.shape[0] + 1, dtype=np.int64) * files.shape[1]
        else:
            if files.ndim != 1:
                raise ValueError("%s: with item_offsets, files, starts and gains must be 1-D; got shape %s" % (what, files.shape))
            offsets = np.ascontiguousarray(np.asarray(item_offsets, dtype=np.int64))
            if offsets.ndim != 1 or offsets.size < 1 or offsets[0] != 0 or np.any(np.diff(offsets) < 0):
                raise ValueError("%s: item_offsets must be [n + 1], start at 0 and not decrease, got %r" % (what, item_offsets))
            if offsets[-1] != files.size:
                raise ValueError("%s: item_offsets end at %d, there are %d terms" % (what, int(offsets[-1]), files.size))
        files, starts, gains = (np.ascontiguousarray(a.reshape(-1)) for a in (files, starts, gains))
        bad = np.flatnonzero(~np.isfinite(gains))
        if bad.size:
            raise ValueError("%s: gains must be finite, got %r at term %d" % (what, float(gains[bad[0]]), int(bad[0])))
        return WindowRows(rate_divisor, mix, resample, channels, bands, speeds, irs, offsets, files, starts, gains)

    def stft_window(self, files, starts, n_frames, hop, n_fft, frame_window=None, bank=None, output="power", center=False,
                    gains=None, item_offsets=None, channels=None, dtype=None, out=None, stream=None, rate_divisor=1, mix=None,
                    resample=None, band_gains=None, band_edges_hz=None, speed_factors=None, speed_index=None, ir_index=None,
                    route_gains=None, route_irs=None, span_first=None, span_len=None, fade_in=None, fade_out=None):
        """mrc_pac_store_stft_window -> a torch tensor [n][channels][n_fft // 2 + 1 | filters][n_frames] on the handle's device:
        the short-time Fourier transform of the rows decode_window_sum gives on the same row arguments, without the rows ever
        being written out.  Row i is that call's float64 row over (n_frames - 1) hop + n_fft samples from its terms' starts;
        frame m is samples [m hop, m hop + n_fft) of it times frame_window (float64 [n_fft]; None: hann_window(n_fft), which
        is torch.hann_window(n_fft); padded_window centres a shorter one as torch.stft(win_length=) does), transformed in
        float64: X[k] = sum_n g[n] x[m hop + n] e^{-2 pi i k n / n_fft}.
        output: "power" (|X|^2, given X every bit defined), "complex" (a complex tensor, torch.view_as_complex of (re, im)), or
        "bank": bank [filters][n_fft // 2 + 1] times the power, each filter a left fold over its support in ascending bin
        (mel_bin_weights builds torchaudio's matrix; any matrix of 1 to MAX_BANDS rows is taken as it is).
        n_fft: even, 16..MAX_STFT_POINTS, factors 2, 3 and 5 only.  hop >= 1.  There is no padding: starts is sample 0 of frame
        0.  center=True subtracts n_fft // 2 from every term's start and does nothing else -- frame m is then centred on sample
        m hop of the row and reads REAL signal around the crop (zeros outside the file), where torch.stft(center=True) reflects
        the crop at its own ends.
        gains=None: one term per item at gain 1.0 (files and starts 1-D); else files, starts, gains and item_offsets as
        decode_window_sum's.  channels, stream, rate_divisor, mix, resample, band_gains, band_edges_hz, speed_factors,
        speed_index, ir_index: decode_window_sum's, unchanged.  dtype: torch.float32 (the default) or torch.float64 (complex64
        or complex128 for output="complex"); out: a contiguous tensor of the result's shape and dtype.  Argument errors are
        ValueErrors before any library call.
        route_gains, route_irs: None, or the routes of decode_window_routed (mrc_pac_store_stft_window_routed): the result is
        [n][C][n_fft // 2 + 1 | filters][n_frames], channel c the transform of that call's channel c, bit for bit.  They stand in
        the place of gains and ir_index and are refused together with either, and with channels; files and starts are 1-D (one
        term per item, or terms with item_offsets) or [n][K].
        span_first, span_len, fade_in, fade_out: decode_window_sum's (mrc_pac_store_stft_window_spans), in the shape of files;
        center=True adds n_fft // 2 to span_first as it subtracts it from starts, so a span keeps its place in the signal.
        Routed calls do not take spans."""
        import torch
        what = "stft_window"
        n_fft, hop, n_frames, window, matrix, mode = check_stft(n_fft, hop, n_frames, frame_window, bank, output, what)
        routed = route_gains is not None or route_irs is not None
        if routed:
            if route_gains is None or route_irs is None:
                raise ValueError("%s: route_gains and route_irs go together, got only %s"
                                 % (what, "route_irs" if route_gains is None else "route_gains"))
            for name, v in (("gains", gains), ("ir_index", ir_index), ("channels", channels)):
                if v is not None:
                    raise ValueError("%s: route_gains and route_irs stand in the place of gains and ir_index and give the channels; "
                                     "%s must be None with them" % (what, name))
            files, starts = self._routed_terms(what, files, starts)
            if item_offsets is not None or files.ndim != 1:
                gains = np.ones(files.shape, np.float64)
        if gains is None:
            files = np.asarray(files, dtype=np.int64).reshape(-1)
            starts = np.asarray(starts, dtype=np.int64).reshape(-1)
            if files.shape != starts.shape:
                raise ValueError("%s: one start per file index (%d files, %d starts)" % (what, files.size, starts.size))
            if item_offsets is not None:
                raise ValueError("%s: item_offsets goes with gains" % what)
            gains, item_offsets = np.ones(files.size, np.float64), np.arange(files.size + 1, dtype=np.int64)
        rows = self._sum_rows(what, files, starts, gains, item_offsets, channels, rate_divisor, mix, resample, band_gains, band_edges_hz,
                              speed_factors, speed_index, ir_index)
        if not isinstance(center, (bool, np.bool_)):
            raise ValueError("%s: center must be True or False, got %r" % (what, center))
        spans = check_spans(span_first, span_len, fade_in, fade_out, np.shape(files), what)
        if spans is not None and routed:
            raise ValueError("%s: route_gains and route_irs do not go with spans" % what)
        if center:
            rows = rows._replace(starts=rows.starts - n_fft // 2)
            if spans is not None:
                spans = (spans[0] + n_fft // 2,) + spans[1:]
        rows = rows._replace(spans=spans)
        n = rows.offsets.size - 1
        is_complex = mode == _lib.MRC_STFT_COMPLEX
        real = {torch.float32: torch.float32, torch.float64: torch.float64, torch.complex64: torch.float32,
                torch.complex128: torch.float64}
        if dtype is None:
            dtype = out.dtype if isinstance(out, torch.Tensor) else torch.float32
        if dtype not in real or (dtype.is_complex and not is_complex):
            raise ValueError("%s: dtype must be torch.float32 or torch.float64%s, got %s"
                             % (what, " (or complex64 / complex128)" if is_complex else "", dtype))
        real_dtype = real[dtype]
        result_dtype = {torch.float32: torch.complex64, torch.float64: torch.complex128}[real_dtype] if is_complex else real_dtype
        n_out = matrix.shape[0] if matrix is not None else n_fft // 2 + 1
        if routed:
            routes = check_routes(route_gains, route_irs, rows.files.size, self._ir_lengths.size, what)
            rows, channels = rows._replace(channels=1, routes=routes), routes[0].shape[1]
            out, stream = self._out_tensor(what, (n, channels, n_out, n_frames), result_dtype, out, stream)
        else:
            channels, out, stream = self._out_side(what, rows.files, rows.channels, lambda c: (n, c, n_out, n_frames), result_dtype,
                                                   out, stream, one_or_two=True)
        return self._call_window(rows, what, n_frames, channels, _formats()[real_dtype], out, stream,
                                 stft=(n_fft, window, n_frames, hop, mode, matrix))

    def stft_ms(self):
        """mrc_pac_store_stft_ms: the device time of the last stft_window's stft_kernel, summed over its slabs"""
        ms = np.zeros(1, np.float64)
        self._handle._check(lib.mrc_pac_store_stft_ms(self._s, ms.ctypes.data))
        return float(ms[0])

    def _energy_window(self, what, table, launch, files, starts, n_frames, hop, channels, dtype, out, stream, mix):
        """band_energy_window and filterbank_window: the checks in the one order, the output tensor, the call.  table() checks
        the call's bands or filters where the band call always has and -> (what launch receives for them, the rows of an
        output channel); launch(mix, n, files, starts, n_frames, hop, table, channels, format, out, stream) -> the library's
        return code."""
        import torch
        mix = check_mix(mix, channels, what)
        if mix is not None:
            channels = 1
        files = np.ascontiguousarray(np.asarray(files, dtype=np.int64).reshape(-1))
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
        if files.shape != starts.shape:
            raise ValueError("%s: one start per file index (%d files, %d starts)" % (what, files.size, starts.size))
        for name, v, least in (("n_frames", n_frames, 0), ("hop", hop, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < least:
                raise ValueError("%s: %s must be an int >= %d, got %r" % (what, name, least, v))
        n, n_frames, hop = files.size, int(n_frames), int(hop)
        if n_frames * hop > 1 << 62:
            raise ValueError("%s: n_frames * hop must not exceed 2^62, got %d * %d" % (what, n_frames, hop))
        table, n_rows = table()
        if dtype is None:
            dtype = torch.float32 if out is None else out.dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: dtype must be torch.float32 or torch.float64, got %s" % (what, dtype))
        channels = self._channels_named(files, channels)
        if not _is_int(channels) or int(channels) not in (1, 2):
            raise ValueError("%s: channels must be None, 1 or 2, got %r" % (what, channels))
        channels = int(channels)
        if n and (files.min() < 0 or files.max() >= len(self)):
            raise ValueError("%s: files must be indices into the store's %d files, got %r" % (what, len(self), files.tolist()))
        if mix is None and n and int(self.n_channels[files].max()) > channels:
            raise ValueError("%s: a stereo file in a one-channel call (channels=1): ask for 2 channels or a mix" % what)
        out, stream = self._out_tensor(what, (n, channels, n_rows, n_frames), dtype, out, stream)
        self._handle._check(launch(_lib.MRC_MIX_EACH if mix is None else mix, n, files.ctypes.data, starts.ctypes.data, n_frames, hop,
                                   table, channels, _formats()[dtype], out.data_ptr() if out.numel() else None, stream or None))
        return out

    def band_energy_window(self, files, starts, n_frames, hop, band_edges_hz, channels=None, dtype=None, out=None, stream=None,
                           mix=None):
        """mrc_pac_store_band_energy_window -> a torch tensor [n][channels][n_bands][n_frames] on the handle's device: the
        energy that band q = [band_edges_hz[q], band_edges_hz[q + 1]) holds in frame j = samples [starts[i] + j hop,
        starts[i] + (j + 1) hop) of file files[i] (decode_window's full-rate coordinates; starts may be negative or past the
        end, a frame outside the file's blocks is 0), from the MDCT lines alone: each block's sum of squares per band, spread
        evenly over the block's tile (levels.LevelMap's), so that bands [0, fs / 2] and frames over the whole file add up to
        the decoded signal's sum of squares.  Only the blocks whose tile a frame touches are parsed; nothing is synthesised.
        band_edges_hz: 2 to 257 increasing frequencies from 0 up (critical_band_edges(sample_rate): the codec's own bands);
        a band narrower than a short block's line spacing may hold no line of such a block and then reads 0 there.
        dtype: torch.float32 (the default) or torch.float64 (every bit defined: see the header).  channels, out, stream: as
        decode_window's; mix: None (every channel), "mid", "left" or "right" (one channel, channels None or 1).  Argument
        errors are ValueErrors before any library call."""
        def edges():
            e = check_band_edges(band_edges_hz, "band_energy_window")
            return e, e.size - 1
        launch = lambda mix, n, files, starts, n_frames, hop, e, channels, fmt, out, stream: lib.mrc_pac_store_band_energy_window(
            self._s, mix, n, files, starts, n_frames, hop, e.size - 1, e.ctypes.data, channels, fmt, out, stream)
        return self._energy_window("band_energy_window", edges, launch, files, starts, n_frames, hop, channels, dtype, out, stream, mix)

    def filterbank_window(self, files, starts, n_frames, hop, points_hz, norm=None, channels=None, dtype=None, out=None,
                          stream=None, mix=None):
        """mrc_pac_store_filterbank_window -> a torch tensor [n][channels][n_filters][n_frames] on the handle's device:
        band_energy_window with a bank of overlapping triangular filters in place of the rectangular bands -- a mel spectrogram
        from the MDCT lines alone.  points_hz: n_filters + 2 increasing frequencies from 0 up (mel_points(80, 0, fs / 2)); filter
        q rises from points_hz[q] to 1 at points_hz[q + 1] and falls to points_hz[q + 2].  A line's weight is the triangle's mean
        over the line's own frequency interval (filterbank_line_weights), so a filter narrower than a short block's line
        spacing still reads its share of the line it lies in: no filter is empty, no frame inside the file reads 0 for want
        of a line.  norm: None, or "slaney" (every filter times 2 / its width in Hz).  Frames, starts, channels, mix, dtype
        (torch.float32 by default; torch.float64: every bit defined, see the header), out and stream are
        band_energy_window's, and so is what the estimate resolves: a block's tile in time, a block's line spacing in
        frequency -- this is not an STFT.  Log compression is the caller's: torch.log(e.clamp_min(1e-10)).  Argument errors
        are ValueErrors before any library call."""
        def table():
            points = check_filter_points(points_hz, "filterbank_window")
            return (points, check_filter_norm(norm, "filterbank_window")), points.size - 2
        launch = lambda mix, n, files, starts, n_frames, hop, t, channels, fmt, out, stream: lib.mrc_pac_store_filterbank_window(
            self._s, mix, n, files, starts, n_frames, hop, t[0].size - 2, t[0].ctypes.data, t[1], channels, fmt, out, stream)
        return self._energy_window("filterbank_window", table, launch, files, starts, n_frames, hop, channels, dtype, out, stream, mix)

    def block_energy(self, rate_divisor=1, mix=None, files=None):
        """mrc_pac_store_block_energy -> (entry_offset [n + 1], blocks [entries][3] (block_start, a, b), energy [entries]):
        one entry per block and channel of every selected file (files: indices into the store; None: every file in order), or
        per block with mix="mid"; selection k's entries are [entry_offset[k], entry_offset[k + 1]), ordered by block, then
        channel.  Every chunk of the selected files is parsed; nothing is synthesised."""
        rate_divisor = check_rate_divisor(rate_divisor, "levels")
        mix = check_levels_mix(mix)
        if files is None:
            sel, n = None, len(self)
            counts = self.n_blocks * (1 if mix == _lib.MRC_MIX_MID else self.n_channels)
        else:
            sel = np.ascontiguousarray(np.asarray(files, dtype=np.int64).reshape(-1))
            n = sel.size
            if n and (sel.min() < 0 or sel.max() >= len(self)):
                raise ValueError("levels: files must be indices into the store's %d files, got %r" % (len(self), files))
            counts = (self.n_blocks * (1 if mix == _lib.MRC_MIX_MID else self.n_channels))[sel]
        cap = int(np.sum(counts))
        entry_offset = np.zeros(n + 1, np.int64)
        blocks, energy = np.zeros((max(cap, 1), 3), np.int64), np.zeros(max(cap, 1), np.float64)
        self._handle._check(lib.mrc_pac_store_block_energy(self._s, rate_divisor, mix, n, None if sel is None else sel.ctypes.data,
                                                           entry_offset.ctypes.data, cap, blocks.ctypes.data, energy.ctypes.data,
                                                           None))
        return entry_offset, blocks[:cap], energy[:cap]

    def levels(self, rate_divisor=1, mix=None, files=None):
        """-> a levels.LevelMap of the selected files (files: indices into the store, map file k = files[k]; None: every file,
        and the map is cached per (rate_divisor, mix)) at 1 / rate_divisor of the sample rate, in the coordinates of
        decode_window at that divisor: per channel (mix=None) or of the mid (mix="mid": one channel per file, a mono file its
        own).  "left" and "right" are columns of mix=None and are refused, like every other argument error, with a ValueError
        before any library call.  One call parses every chunk of the selected files once (block_energy_kernel: the sum of
        squares of each block's decoded lines, no inverse transform)."""
        from .levels import LevelMap
        rate_divisor = check_rate_divisor(rate_divisor, "levels")
        check_levels_mix(mix)
        if files is None and (rate_divisor, mix) in self._levels:
            return self._levels[(rate_divisor, mix)]
        entry_offset, blocks, energy = self.block_energy(rate_divisor, mix, files)
        sel = np.arange(len(self)) if files is None else np.asarray(files, dtype=np.int64).reshape(-1)
        cfg = self._handle.cfg
        per_file = []
        for k, f in enumerate(sel):
            lo, hi = int(entry_offset[k]), int(entry_offset[k + 1])
            nch = 1 if mix == "mid" else int(self.n_channels[f])
            per_file.append(dict(blocks=blocks[lo:hi:nch], energy=energy[lo:hi].reshape(-1, nch),
                                 n_samples=int(self.n_samples[f]) // rate_divisor))
        m = LevelMap(per_file, cfg.n_mdct_lines, rate_divisor, cfg.n_short)
        if files is None:
            self._levels[(rate_divisor, mix)] = m
        return m

    def stats(self):
        """of the last decode_window: chunks_parsed, decode_launches, slabs, plan_bytes_uploaded, and ms: the device time of
        the plan upload, the unpack kernel, the synthesis and window_out_kernel (with resample=: resample_out_kernel, and the
        counts are those of the intermediate spans), summed over the slabs.  After decode_window_sum(): the same, the counts
        those of all terms and ms["window_out"] the time of sum_out_kernel (resample_sum_out_kernel).  With speed_factors=:
        chunks_parsed is the sum over the units of what the single-ratio call parses for each at its own ratio, slabs counts
        runs of rows whose units, each at the call's largest span, fit MRC_OPT_STORE_SLAB_SAMPLES, plan_bytes_uploaded includes
        the units' ratio indices and the table of ratios, and ms["window_out"] is resample_multi_sum_out_kernel's.  After levels() or
        block_energy(): decode_launches counts block_energy_kernel launches, ms["synthesis"] is that kernel's time and
        ms["window_out"] is 0.  After band_energy_window(): decode_launches counts band_energy_kernel launches,
        ms["synthesis"] is the band sums' time (that kernel) and ms["window_out"] the frame assembly's (band_frames_kernel);
        after filterbank_window() the same with filterbank_energy_kernel in band_energy_kernel's place."""
        st, ms = np.zeros(4, np.int64), np.zeros(4, np.float64)
        self._handle._check(lib.mrc_pac_store_stats(self._s, st.ctypes.data, ms.ctypes.data))
        r = {k: int(v) for k, v in zip(STAT_NAMES, st)}
        r["ms"] = {k: float(v) for k, v in zip(MS_NAMES, ms)}
        return r
