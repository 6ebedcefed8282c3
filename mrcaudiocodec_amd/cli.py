"""
Encode direction of the reference's command line (`python pacfileThem.py in.wav`, pacfileThem.py:1064-1231)
on the MI355X path:  python -m mrcaudiocodec_amd.cli in.wav out.pac [--no-huffman] [--device N]  (mono or stereo)

WAV ingest (pcmfile.py:34-102: 16-bit PCM, int16 code c -> sign(c) 2|c|/65535), transient detection with
one hop of look-ahead (pacfileThem.py:1025-1056, 1182-1214), joint-stereo blocks with the bit reservoir
chained through the Huffman savings, Close()'s flush block, `.pac` framing -- the whole loop in one library call on
the GPU.  Like the reference, the last hop of the file is analysed but never encoded.
Mono WAVs: the same loop with WriteDataBlock in place of JointWriteDataBlock (the reference library's mono path,
pacfileThem.py:622-790 and the commented-out call at 1218): one-channel blocks, one Close() block.  Other channel
counts are refused: the file format's readers stop at two channels and Close() flushes at most two.

Bit rates: --bits-per-sample 4 encodes at 4 bits per sample instead of the reference's 2.86.  A comma-separated list is a
rate LADDER, encoded in one library call (mrc_encode_chained_ladder_pac: the transform and the psychoacoustic model once,
the reservoir scan per rate); the output name must then contain {bps}, replaced by each value as written:
    python -m mrcaudiocodec_amd.cli in.wav out_{bps}.pac --bits-per-sample 1.5,2.86,4

Decode direction (row f-4):  python -m mrcaudiocodec_amd.cli -d in.pac out.wav
One library call (mrc_decode_pac_pcm16): chunk parsing and Huffman decoding, dequantise / M-S / IMDCT / window /
overlap-add and the interleaved 16-bit PCM codes all on the GPU, then the WAV header of pcmfile.py:141-153.  The first decoded block (the MDCT's half-block delay) is dropped as in the
reference's loop; everything after it is written, header sample count = what was decoded.
An excerpt:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --start S --samples N  decodes N samples from sample S of that
output on through a one-file resident store (mrc_pac_store_decode_window): only the blocks the excerpt overlaps are parsed
and synthesised.  --start defaults to 0, --samples to the rest of the file; what lies outside the file is silence.
At half or quarter rate:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --rate-divisor 2  (or 4) decodes through the same
store straight from the MDCT lines (mrc_pac_store_decode_window_reduced): the WAV's header carries sample_rate // D, and
--start / --samples then count samples at that rate.  Refused when D does not divide the file's sample rate.
One channel:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --mix mid  (or left, right) writes a one-channel WAV through
the same store (mrc_pac_store_decode_window_mix): the mid (L + R) / 2 of a stereo file, formed on the MDCT lines before the
one inverse transform, or its left or right channel; a mono file gives its channel.  Composes with --rate-divisor, --start
and --samples.
At any rate:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --sample-rate 16000  decodes through the same store at the
largest rate divisor that still holds the band and a polyphase resampler on the device for the rest
(mrc_pac_store_decode_window_resampled, store.resample_plan: 48 kHz -> 16 kHz is half-rate synthesis, then 2 / 3): the WAV's
header carries HZ, and --start / --samples count samples at HZ.  Composes with --mix, --start and --samples; refused together
with --rate-divisor.
A mixture:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --overlay other.pac --snr-db DB [--overlay-start N]  puts both files
into one store and writes in.pac + g * other.pac in ONE call of two terms (mrc_pac_store_decode_window_sum), g the factor that
puts in.pac DB above other.pac over the excerpt (levels.LevelMap.gains_for_snr, from the block energies; printed).  N is the
overlay's sample under the excerpt's first; a negative N starts the overlay that far into the excerpt.  Codec settings that
differ between the files are refused, the parameter named.  Composes with --start, --samples, --mix, --rate-divisor and
--sample-rate.
A changed spectrum:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --band-gains-db "0-300:-inf,3400-24000:-inf"  multiplies
the file's MDCT lines between LO and HI Hz by DB decibels (-inf: zero) before the inverse transform, through the same store
(mrc_pac_store_decode_window_shaped): bands ascend and do not overlap, a gap stays at 0 dB.  Composes with --start, --samples,
--rate-divisor, --mix, --sample-rate and --overlay (the overlay is left as it is); refused without -d and with --band-energies.
Per-line gains are not an LTI filter: a brick-wall edge leaves a small aliasing residue near the edge frequency.
At another speed:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --speed 11/10  plays the file NUM/DEN times as fast (pitch and
tempo together, the speed perturbation of speech recipes) through the same store (mrc_pac_store_decode_window_speeds): the
file is read at the output rate's ratio divided by the speed, the WAV's header carries the output rate unchanged, and
--start / --samples count output samples -- the whole file is n_samples_resampled of the combined ratio.  Composes with
--sample-rate, --rate-divisor, --mix, --band-gains-db and --overlay; the overlay stays at speed 1, in the same one call.
Refused without -d and with --band-energies.
Through a room:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --ir room.npy  (or a mono 16-bit room.wav) convolves the file
with that impulse response through the same store (mrc_pac_store_decode_window_reverb), last of all: at the output rate, after
the speed.  A .npy array is taken as sampled at the output rate; a WAV is brought there from its own rate (store.ir_at_rate).
Composes with --sample-rate, --rate-divisor, --speed, --mix, --band-gains-db, --start, --samples and --overlay; the overlay
stays dry, in the same one call.  Refused without -d.
Levels:  python -m mrcaudiocodec_amd.cli --levels a.pac [b.pac ...] [--levels-window N]  decodes nothing and writes nothing: per
file one JSON line with its channels, samples, RMS level per channel (dB re full scale) and its loudest and quietest window of
N samples (default one second) on the short-block grid with their starts, from the energies of the blocks' MDCT lines
(mrc_pac_store_block_energy, levels.LevelMap).  Composes with --rate-divisor and --mix mid; refuses every other flag.
Band energies:  python -m mrcaudiocodec_amd.cli --band-energies in.pac out.npy --hop N [--band-edges f0,f1,...] [--mix CH]
decodes nothing: out.npy holds float32 [channels][bands][frames], the energy of each band in frame [j N, (j + 1) N) of the
file from its MDCT lines (mrc_pac_store_band_energy_window); default bands: the codec's critical bands.  Refuses every
encode, decode and levels flag.
Filter-bank energies:  python -m mrcaudiocodec_amd.cli --filterbank-energies in.pac out.npy --hop N (--mel N [--f-min HZ]
[--f-max HZ] [--mel-scale htk|slaney] | --filter-points f0,f1,...) [--filter-norm slaney] [--mix CH]  is the same with a bank
of overlapping triangular filters (mrc_pac_store_filterbank_window): out.npy holds float32 [channels][filters][frames].  --mel N
spaces N filters equally in mel from --f-min (default 0) to --f-max (default Nyquist); --filter-points names the filters'
points itself.  A filter narrower than a block's line spacing reads its share of the line it lies in: no row is empty.
Refuses every encode, decode, levels and band-energy flag.
STFT energies:  python -m mrcaudiocodec_amd.cli --stft-energies in.pac out.npy --n-fft N --hop H [--win-length W] [--mel N [--f-min HZ]
[--f-max HZ] [--mel-scale htk|slaney] [--filter-norm slaney]] [--complex]  writes the short-time Fourier transform of the row that
-d would decode (mrc_pac_store_stft_window): float32 power [channels][N / 2 + 1][frames], with --mel the totals of N mel filters
on the bins (store.mel_bin_weights: torchaudio's rule), with --complex the complex64 bins.  The frame window is the periodic
Hann of W taps (default N) centred in N points; frame j is samples [j H, j H + N) of the row, and --samples is rounded down to
whole frames.  It composes with the flags -d takes for a row: --start, --samples, --rate-divisor, --sample-rate, --mix, --speed,
--ir, --band-gains-db, --overlay, --snr-db; it refuses -d itself and every encode, levels and line-energy flag.
One after another:  python -m mrcaudiocodec_amd.cli -d in.pac out.wav --append other.pac [--crossfade N]  decodes in.pac followed by
other.pac (same codec settings) in ONE call of two terms with spans (PacStore.decode_window_sum(span_first=, span_len=)); with
--crossfade the two overlap by N output samples, in.pac fading out and other.pac fading in linearly.  Composes with
--rate-divisor, --sample-rate and --mix; refused without -d and with the other row flags.

Quality (mrc_pac_nmr): --nmr on an encode prints, per file written (every rung of a ladder), one JSON line with the
noise-to-mask ratio of the file against the WAV, measured with the codec's own masking model: nmr_max_db (worst band),
nmr_total_db (band-averaged ratio, weighted by block length), disturbed_blocks (blocks with a band whose noise exceeds
its mask) and n_blocks.  --measure prints the same lines for existing dst file(s) against src without encoding:
    python -m mrcaudiocodec_amd.cli in.wav out_{bps}.pac --bits-per-sample 1.5,2.86,4 --measure

Constant-quality VBR (mrc_encode_vbr_nmr_pac): --vbr-nmr DB codes every band with the fewest bits that keep its noise-to-mask
ratio <= DB; no bit rate is given, one JSON line reports bits per sample, capped bands and the NMR of the file written.
Target quality (mrc_encode_chained_target_nmr_pac): --target-nmr DB with an ascending --bits-per-sample list of two rates or
more encodes the ladder, measures every rung on the device and writes ONE file to dst: the lowest rate whose nmr_total_db
is <= DB (the top rate if none is).  One JSON line says which: chosen_bits_per_sample, met, and per rung nmr_total_db,
nmr_max_db and disturbed_blocks.  The numbers are those of pacfile.measure_nmr on each rung's file against the samples up
to the end of the last coded block; --measure reads the whole WAV and so holds Close()'s block against the file's last hop,
which the encoder analyses but never codes: the two agree when that hop is silent.
    python -m mrcaudiocodec_amd.cli in.wav out.pac --bits-per-sample 1.5,2.86,4,8 --target-nmr -3
"""
import argparse
import json
import os
import sys
from collections import namedtuple
from contextlib import contextmanager
from struct import pack, unpack

import numpy as np

from . import Handle, MrcError, pacfile, transient
from ._lib import MRC_MAX_CEILINGS, MRC_MAX_RATES


def read_wav_pcm(path, hop=1024):
    """-> (sample_rate, n_channels, num_samples, int16 [nCh][nHops*hop]): the file's own codes, the last hop zero padded.
    The float map of pcmfile.py:91-100 (x = sign(c) 2|c| / 65535, -32768 -> 0.0) is applied on the device, on load."""
    with open(path, "rb") as fp:
        head = fp.read(12)
        if head[0:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("not a RIFF/WAVE file")
        while True:
            tag = fp.read(4)
            if len(tag) < 4:
                raise ValueError("no 'fmt ' chunk")
            if tag == b"fmt ":
                break
        (_, fmt, n_ch, rate, _, _, bits) = unpack("<LHHLLHH", fp.read(20))
        if fmt != 1 or bits != 16:
            raise ValueError("only 16-bit PCM WAV files are supported")
        while True:
            tag = fp.read(4)
            if len(tag) < 4:
                raise ValueError("no 'data' chunk")
            if tag == b"data":
                break
        num_samples = unpack("<L", fp.read(4))[0] // (n_ch * 2)
        raw = fp.read(num_samples * n_ch * 2)
    codes = np.frombuffer(raw, dtype="<i2")
    codes = codes[:(len(codes) // n_ch) * n_ch].reshape(-1, n_ch).T
    n_hops = -(-codes.shape[1] // hop)
    pcm = np.zeros((n_ch, n_hops * hop), np.int16)
    pcm[:, :codes.shape[1]] = codes
    return rate, n_ch, num_samples, pcm


def read_wav(path, hop=1024):
    """-> (sample_rate, n_channels, num_samples, float64 [nCh][nHops*hop]) as pcmfile.py:91-100 hands the samples on."""
    rate, n_ch, num_samples, pcm = read_wav_pcm(path, hop)
    c = pcm.astype(np.float64)
    mag = np.abs(c)
    return rate, n_ch, num_samples, np.where(mag >= 32768, 0.0, np.sign(c) * 2.0 * mag / 65535)


def parse_bits_per_sample(value):
    """--bits-per-sample: a number, or several separated by commas (a str), or a sequence of numbers -> [(text as written,
    float)].  Every value must be finite and in (0, 64] (the rates the library takes)."""
    if isinstance(value, str):
        texts = [t.strip() for t in value.split(",")]
    elif isinstance(value, (int, float, np.integer, np.floating)):
        texts = [str(value)]
    else:
        texts = [str(v) for v in value]
    if not texts or any(not t for t in texts):
        raise ValueError("--bits-per-sample: expected a comma-separated list of numbers, got %r" % (value,))
    out = []
    for t in texts:
        try:
            v = float(t)
        except ValueError:
            raise ValueError("--bits-per-sample: %r is not a number" % t)
        if not np.isfinite(v) or not 0.0 < v <= 64.0:
            raise ValueError("--bits-per-sample: %s lies outside (0, 64]" % t)
        out.append((t, v))
    if len(out) > MRC_MAX_RATES:
        raise ValueError("--bits-per-sample: at most %d rates in one ladder" % MRC_MAX_RATES)
    return out


def ladder_paths(out_path, rates):
    """out_path with {bps} replaced by each rate as written"""
    return [out_path.replace("{bps}", t) for (t, _) in rates]


_Wav = namedtuple("_Wav", "h n_ch num_samples rate codes shapes header")


@contextmanager
def _wav_on_handle(in_path, handle, device_id, exact_spread, new_handle=None, options=None):
    """What every encode of a WAV file starts and ends with.  Reads in_path (1 or 2 channels, a sample rate the reference can
    encode), takes the caller's handle or creates one (new_handle: further keyword arguments of Handle), sets
    MRC_OPT_EXACT_SPREAD if asked and the options {option: value} besides, prepends the zero prior hop
    (pacfileThem.py:615-618) and runs the transient detector.
    Yields (h, n_ch, num_samples, rate, codes int16 [n_ch][n], shapes, the file's header bytes).  On exit a caller's handle
    gets back option 1 and those of `options` as it came with them, whatever the body set; a handle created here is closed."""
    rate, n_ch, num_samples, pcm = read_wav_pcm(in_path)
    if n_ch not in (1, 2):
        raise ValueError("%d-channel input: mono and stereo WAV files only (the .pac readers refuse more than two channels "
                         "and the reference's Close() flushes at most two)" % n_ch)
    shape = {} if handle is None else dict(n_mdct_lines=handle.cfg.n_mdct_lines, n_short=handle.cfg.n_short)
    try:                                 # (the rate decides the band tables: below ~31 kHz the reference's raise IndexError)
        header = pacfile.header(pacfile.make_config(sample_rate=rate, **shape), n_ch, num_samples)
    except MrcError as e:
        raise ValueError("%d Hz input: outside the sample rates the reference can encode (%s)" % (rate, e))
    h = handle if handle is not None else Handle(sample_rate=rate, device_id=device_id, **(new_handle or {}))
    options = {**(options or {}), **({1: 1} if exact_spread else {})}
    came_with = {opt: h.get_option(opt) for opt in {1, *options}}
    try:
        for opt, value in options.items():
            h.set_option(opt, value)
        L = h.cfg.n_mdct_lines
        codes = np.concatenate([np.zeros((n_ch, L), np.int16), pcm], axis=1)
        shapes = transient.block_shape_array(h, codes)
        if not len(shapes):
            raise ValueError("file too short: fewer than two hops")
        if shapes[-1, 2] != L:
            raise ValueError("the stream must end with a long block (the reference's Close() assumes it)")
        yield _Wav(h, n_ch, num_samples, rate, codes, shapes, header)
    finally:
        if handle is None:
            h.close()
        else:
            for opt, value in came_with.items():
                h.set_option(opt, value)


def _write(out_path, data):
    if out_path:
        with open(out_path, "wb") as f:
            f.write(data)


def encode_wav(in_path, out_path=None, use_huffman=True, device_id=0, handle=None, exact_spread=False, certify=None,
               bits_per_sample=None):
    """bits_per_sample: None -- the handle's rate (a new handle: the reference's 2.86); one value -- that target bit rate;
    several (a comma-separated str or a sequence) -- a rate ladder in ONE chained call (mrc_encode_chained_ladder_pac):
    out_path must then contain {bps}, written once per rate with the value as given, and a list of byte strings (one per
    rate) is returned.  A ladder refuses certify.  These checks run before the file is read or a device is touched.
    certify: a dict to fill with the sensitivity certificate of the encode (mrc_get_sensitivity: how many integer decisions
    were taken within a guard band of floating-point rounding); if any was, the file is encoded once more with the masker
    spreading evaluated operation by operation (MRC_OPT_EXACT_SPREAD) and certify["bytes_equal_exact_spread"] says whether
    the two encodes gave the same bytes.
    exact_spread: evaluate the masker spreading operation by operation like psychoac.py:68-78 (MRC_OPT_EXACT_SPREAD,
    ~30x slower kernel).  Both modes give the reference driver's bytes on every fixture and sweep; neither is
    bit-identical by construction (README.md, "Parity").
    The file's int16 codes go to the device as they are: the transient detector (mrc_transient_peaks_ex) and the whole
    encode loop (ONE call, mrc_encode_chained_stream_pcm16_pac) read them there; 2 bytes per sample on the host."""
    rates = None if bits_per_sample is None else parse_bits_per_sample(bits_per_sample)
    ladder = rates is not None and len(rates) > 1
    if ladder and certify is not None:
        raise ValueError("--certify takes one bit rate (the sensitivity certificate covers one encode)")
    if ladder and out_path is not None and "{bps}" not in out_path:
        raise ValueError("several bit rates: the output name must contain {bps} (e.g. out_{bps}.pac)")
    if rates is not None and not ladder and handle is not None and rates[0][1] != handle.cfg.target_bits_per_sample:
        ladder = True                    # (a caller's handle at another rate: a ladder of one, the handle stays as it is)
        if certify is not None:
            raise ValueError("--certify: the handle's target_bits_per_sample differs from bits_per_sample")
    tbps = {} if rates is None or ladder else dict(target_bits_per_sample=rates[0][1])
    sens = {} if certify is None else {5: 1}
    if certify is not None and handle is not None:
        handle.sensitivity()             # (counts a caller's handle still holds are not this encode's)
    with _wav_on_handle(in_path, handle, device_id, exact_spread, new_handle=tbps, options=sens) as w:
        if ladder:
            datas = pacfile.encode_stream_ladder(w.h, w.codes, w.shapes, [v for (_, v) in rates], use_huffman=use_huffman,
                                                 num_samples=w.num_samples)
            if out_path:
                for path, d in zip(ladder_paths(out_path, rates), datas):
                    _write(path, d)
            return datas if len(rates) > 1 else datas[0]
        right = None if w.n_ch == 1 else w.codes[1][None]                      # (None: mono streams)
        once = lambda: w.h.encode_chained_pac(w.codes[0][None], right, [w.shapes], use_huffman=use_huffman, with_flush=True,
                                              num_samples=[w.num_samples])["bytes"].tobytes()
        data = once()
        if certify is not None:
            certify.update(w.h.sensitivity())
            near = sum(certify[k] for k in ("quantiser_edges", "bitalloc_near_ties", "ms_switch_near_threshold", "peak_near_ties"))
            certify["decisions_near_an_edge"] = near
            if near and not exact_spread:
                w.h.set_option(5, 0)
                w.h.set_option(1, 1)
                certify["bytes_equal_exact_spread"] = once() == data
    _write(out_path, data)
    return data


def _only_encodes(what, decode, certify, measure):
    if decode or certify or measure:
        raise ValueError("%s: it does not go with -d, --certify or --measure" % what)


def _writes_one_file(flag, out_path):
    if out_path is not None and "{bps}" in out_path:
        raise ValueError("%s writes ONE file: dst must not contain {bps}" % flag)


def _number(flag, value, kind=float, what="a number"):
    try:
        return kind(value)
    except (TypeError, ValueError):
        raise ValueError("%s: %r is not %s" % (flag, value, what))


def check_target_args(bits_per_sample, target_nmr, out_path=None, decode=False, certify=False, measure=False):
    """The refusals of --target-nmr, before a file is read or a device is touched.  -> [(text, rate)], the target (float)."""
    _only_encodes("--target-nmr encodes one file at the rate it picks", decode, certify, measure)
    target = _number("--target-nmr", target_nmr)
    if np.isnan(target):
        raise ValueError("--target-nmr: the target must not be NaN")
    if bits_per_sample is None:
        raise ValueError("--target-nmr needs --bits-per-sample with two rates or more to choose from")
    rates = parse_bits_per_sample(bits_per_sample)
    if len(rates) < 2:
        raise ValueError("--target-nmr needs two rates or more to choose from (--bits-per-sample 1.5,2.86,4)")
    if any(b[1] <= a[1] for a, b in zip(rates, rates[1:])):
        raise ValueError("--target-nmr: --bits-per-sample must be strictly ascending")
    _writes_one_file("--target-nmr", out_path)
    return rates, target


def encode_wav_target_nmr(in_path, out_path, bits_per_sample, target_nmr, use_huffman=True, device_id=0, handle=None,
                          exact_spread=False):
    """encode_wav at the lowest rate of the ladder bits_per_sample whose nmr_total_db against the WAV is <= target_nmr, in
    one library call (mrc_encode_chained_target_nmr_pac).  Writes the one file to out_path (if given) and returns the
    report: data, chosen, chosen_bits_per_sample (as written), rate, met, per-rung nmr_total_db / nmr_max_db /
    disturbed_blocks, n_blocks.  The argument checks run before the file is read or a device is touched."""
    rates, target = check_target_args(bits_per_sample, target_nmr, out_path)
    with _wav_on_handle(in_path, handle, device_id, exact_spread) as w:
        r = pacfile.encode_stream_target_nmr(w.h, w.codes, w.shapes, [v for (_, v) in rates], target, use_huffman=use_huffman,
                                             num_samples=w.num_samples)
    r["chosen_bits_per_sample"] = rates[r["chosen"]][0]
    r["bits_per_sample"] = [t for (t, _) in rates]
    _write(out_path, r["data"])
    return r


def check_vbr_args(vbr_nmr, bits_per_sample=None, target_nmr=None, out_path=None, decode=False, certify=False, measure=False):
    """The refusals of --vbr-nmr, before a file is read or a device is touched.  -> the ceiling in dB (float)."""
    _only_encodes("--vbr-nmr encodes one file", decode, certify, measure)
    if bits_per_sample is not None or target_nmr is not None:
        raise ValueError("--vbr-nmr has no bit rate: it does not go with --bits-per-sample or --target-nmr")
    ceiling = _number("--vbr-nmr", vbr_nmr)
    if np.isnan(ceiling):
        raise ValueError("--vbr-nmr: the ceiling must not be NaN")
    _writes_one_file("--vbr-nmr", out_path)
    return ceiling


def _coded_samples(shapes):
    return sum(int(b) for (_, _, b) in shapes)


def encode_wav_vbr_nmr(in_path, out_path, vbr_nmr, use_huffman=True, device_id=0, handle=None, exact_spread=False):
    """encode_wav as constant-quality VBR (mrc_encode_vbr_nmr_pac): every band coded with the fewest bits that keep its
    noise-to-mask ratio <= vbr_nmr dB.  Writes the file to out_path (if given) and returns the report of
    pacfile.encode_stream_vbr_nmr plus bits_per_sample = coded_bits / (channels x coded samples)."""
    ceiling = check_vbr_args(vbr_nmr, out_path=out_path)
    with _wav_on_handle(in_path, handle, device_id, exact_spread) as w:
        r = pacfile.encode_stream_vbr_nmr(w.h, w.codes, w.shapes, ceiling, use_huffman=use_huffman, num_samples=w.num_samples)
    r["bits_per_sample"] = r["coded_bits"] / float(w.n_ch * _coded_samples(w.shapes))
    _write(out_path, r["data"])
    return r


def vbr_size_target_bytes(bits_per_sample, header_bytes, coded_samples, channels, chunks):
    """--vbr-bits-per-sample X as a file size: header + floor(X * coded_samples * channels / 8) + 4 * chunks."""
    return int(header_bytes) + int(np.floor(float(bits_per_sample) * coded_samples * channels / 8.0)) + 4 * int(chunks)


def check_vbr_size_args(vbr_bytes=None, vbr_bits_per_sample=None, vbr_grid=None, bits_per_sample=None, target_nmr=None,
                        vbr_nmr=None, out_path=None, decode=False, certify=False, measure=False):
    """The refusals of --vbr-bytes / --vbr-bits-per-sample, before a file is read or a device is touched.
    -> (bytes or None, bits per sample or None, (lo_db, step_db, n))."""
    which = "--vbr-bytes" if vbr_bytes is not None else "--vbr-bits-per-sample"
    if vbr_bytes is None and vbr_bits_per_sample is None:
        raise ValueError("--vbr-grid goes with --vbr-bytes or --vbr-bits-per-sample")
    if vbr_bytes is not None and vbr_bits_per_sample is not None:
        raise ValueError("--vbr-bytes and --vbr-bits-per-sample are two ways to give ONE size: take one")
    _only_encodes("%s encodes one file" % which, decode, certify, measure)
    if bits_per_sample is not None or target_nmr is not None or vbr_nmr is not None:
        raise ValueError("%s searches the ceiling itself: it does not go with --bits-per-sample, --target-nmr or --vbr-nmr" % which)
    _writes_one_file(which, out_path)
    nbytes = bps = None
    if vbr_bytes is not None:
        nbytes = _number("--vbr-bytes", vbr_bytes, int, "a whole number")
        if nbytes < 0:
            raise ValueError("--vbr-bytes: the size must not be negative")
    else:
        bps = _number("--vbr-bits-per-sample", vbr_bits_per_sample)
        if not np.isfinite(bps) or bps < 0:
            raise ValueError("--vbr-bits-per-sample: the rate must be finite and not negative")
    grid = (-30.0, 0.25, 256)
    if vbr_grid is not None:
        parts = str(vbr_grid).split(":")
        try:
            if len(parts) != 3:
                raise ValueError
            grid = (float(parts[0]), float(parts[1]), int(parts[2]))
        except ValueError:
            raise ValueError("--vbr-grid: %r is not LO:STEP:N (two numbers and a count)" % (vbr_grid,))
        if not np.isfinite(grid[0]) or not np.isfinite(grid[1]) or not grid[1] > 0:
            raise ValueError("--vbr-grid: LO and STEP must be finite, STEP > 0")
        if not 1 <= grid[2] <= MRC_MAX_CEILINGS:
            raise ValueError("--vbr-grid: N must lie in 1..%d" % MRC_MAX_CEILINGS)
    return nbytes, bps, grid


def encode_wav_vbr_size(in_path, out_path, vbr_bytes=None, vbr_bits_per_sample=None, vbr_grid=None, use_huffman=True, device_id=0,
                        handle=None, exact_spread=False):
    """encode_wav as constant-quality VBR to a size (mrc_encode_vbr_size_pac): the tightest ceiling of the grid whose file
    is <= vbr_bytes, or <= vbr_size_target_bytes(vbr_bits_per_sample, ..).  Writes the file to out_path (if given) and
    returns the report of pacfile.encode_stream_vbr_size plus target_bytes and bits_per_sample."""
    nbytes, bps, grid = check_vbr_size_args(vbr_bytes, vbr_bits_per_sample, vbr_grid, out_path=out_path)
    with _wav_on_handle(in_path, handle, device_id, exact_spread) as w:
        coded = _coded_samples(w.shapes)
        if nbytes is None:
            nbytes = vbr_size_target_bytes(bps, len(w.header), coded, w.n_ch, w.n_ch * (len(w.shapes) + 1))
        r = pacfile.encode_stream_vbr_size(w.h, w.codes, w.shapes, nbytes, grid[0], grid[1], grid[2], use_huffman=use_huffman,
                                           num_samples=w.num_samples)
    r["target_bytes"] = nbytes
    r["bits_per_sample"] = r["coded_bits"] / float(w.n_ch * coded)
    _write(out_path, r["data"])
    return r


def wav_header(n_ch, n_data_bytes, sample_rate):
    """pcmfile.py:141-153"""
    return pack('<4sL4s4sLHHLLHH4sL', b"RIFF", 36 + n_data_bytes, b"WAVE", b"fmt ", 16, 1, n_ch, sample_rate,
                sample_rate * n_ch * 2, n_ch * 2, 16, b"data", n_data_bytes)


def wav_bytes(pcm, sample_rate):
    """pcmfile.py:141-153 header + interleaved little-endian int16 samples; pcm int16 [nCh][samples]."""
    n_ch, n = pcm.shape
    data = np.ascontiguousarray(pcm.T).astype("<i2").tobytes()
    return wav_header(n_ch, len(data), sample_rate) + data


def check_excerpt_args(start, samples, decode):
    """--start / --samples as given (None: not given) -> (start, samples or None for "to the end"), or None when neither was
    given.  They cut an excerpt out of a decode: refused without -d, and a negative sample count is refused."""
    if start is None and samples is None:
        return None
    if not decode:
        raise ValueError("--start and --samples cut an excerpt out of a decode: they need -d")
    if samples is not None and samples < 0:
        raise ValueError("--samples: %d is negative" % samples)
    return (0 if start is None else int(start)), (None if samples is None else int(samples))


def check_rate_divisor_args(rate_divisor, decode):
    """--rate-divisor as given (None: not given) -> the divisor (1 when not given).  It decodes at a fraction of the sample
    rate: refused without -d, and anything but 1, 2 or 4 is refused."""
    if rate_divisor is None:
        return 1
    if not decode:
        raise ValueError("--rate-divisor decodes at a fraction of the sample rate: it needs -d")
    if isinstance(rate_divisor, bool) or not isinstance(rate_divisor, (int, np.integer)) or int(rate_divisor) not in (1, 2, 4):
        raise ValueError("--rate-divisor: %r is not 1, 2 or 4" % (rate_divisor,))
    return int(rate_divisor)


def check_sample_rate_args(sample_rate, decode, rate_divisor_given=False):
    """--sample-rate as given (None: not given) -> the rate in Hz or None.  It decodes at that rate: refused without -d,
    together with --rate-divisor (it picks the divisor itself), and when it is not a positive whole number."""
    if sample_rate is None:
        return None
    if not decode:
        raise ValueError("--sample-rate decodes at another sample rate: it needs -d")
    if rate_divisor_given:
        raise ValueError("--sample-rate picks the rate divisor itself: it does not go with --rate-divisor")
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or int(sample_rate) < 1:
        raise ValueError("--sample-rate: %r is not a positive number of Hz" % (sample_rate,))
    return int(sample_rate)


def check_mix_args(mix, decode):
    """--mix as given (None: not given) -> "mid", "left", "right" or None.  It picks one channel of a decode: refused
    without -d, and any other word is refused."""
    if mix is None:
        return None
    if not decode:
        raise ValueError("--mix decodes one channel of a stereo file: it needs -d")
    if mix not in ("mid", "left", "right"):
        raise ValueError("--mix: %r is not mid, left or right" % (mix,))
    return mix


def check_overlay_args(overlay, snr_db, overlay_start, decode):
    """--overlay, --snr-db and --overlay-start as given (None: not given) -> (path, SNR in dB, the overlay's start), or None
    without --overlay.  --overlay adds a second file under a decode at a signal-to-noise ratio: refused without -d and
    without --snr-db; --snr-db and --overlay-start are refused without --overlay; the SNR is a finite number of dB."""
    if overlay is None:
        for flag, v in (("--snr-db", snr_db), ("--overlay-start", overlay_start)):
            if v is not None:
                raise ValueError("%s belongs to --overlay: it needs --overlay" % flag)
        return None
    if not decode:
        raise ValueError("--overlay adds a second .pac file under a decode: it needs -d")
    if snr_db is None:
        raise ValueError("--overlay needs --snr-db: the level of src over the overlay in dB")
    snr = _number("--snr-db", snr_db)
    if not np.isfinite(snr):
        raise ValueError("--snr-db: %r is not a finite number of dB" % (snr_db,))
    if overlay_start is not None and (isinstance(overlay_start, bool) or not isinstance(overlay_start, (int, np.integer))):
        raise ValueError("--overlay-start: %r is not a whole number of samples" % (overlay_start,))
    return str(overlay), snr, (0 if overlay_start is None else int(overlay_start))


LEVELS_REFUSES = ("src", "dst", "-d", "--no-huffman", "--exact-spread", "--certify", "--bits-per-sample", "--nmr", "--measure",
                  "--target-nmr", "--vbr-nmr", "--vbr-bytes", "--vbr-bits-per-sample", "--vbr-grid", "--start", "--samples",
                  "--sample-rate")


def check_levels_args(levels, levels_window, given):
    """--levels as given (None: not given) with --levels-window -> (paths, window or None), or None without --levels.  It
    reads `.pac` files and writes nothing: given (flag -> whether it was given, for LEVELS_REFUSES) must be empty of
    positional files and of every encode, decode, excerpt and measure flag; --levels-window needs --levels and is >= 1."""
    if levels is None:
        if levels_window is not None:
            raise ValueError("--levels-window is the window of --levels: it needs --levels")
        return None
    for flag in LEVELS_REFUSES:
        if given.get(flag):
            raise ValueError("--levels prints the levels of .pac files and nothing else: it does not go with %s%s"
                             % (flag, " (name the files behind --levels)" if flag in ("src", "dst") else ""))
    if levels_window is not None and (isinstance(levels_window, bool) or not isinstance(levels_window, (int, np.integer))
                                      or int(levels_window) < 1):
        raise ValueError("--levels-window: %r is not a positive number of samples" % (levels_window,))
    return list(levels), (None if levels_window is None else int(levels_window))


def levels_of_files(pac_paths, window=None, device_id=0, rate_divisor=1, mix=None):
    """One dict per `.pac` file from its block energies (PacStore.levels: no file is decoded): file, channels, samples,
    rms_db (per channel, over the whole file), window, and the loudest and quietest window of that many samples on the n_short
    grid with their starts (None for a file shorter than the window).  window None: one second.  rate_divisor 2 or 4: all of
    it at that fraction of the sample rate; mix "mid": of the mid (L + R) / 2, one channel."""
    from .store import PacStore, check_levels_mix
    rate_divisor = check_rate_divisor_args(rate_divisor, True)
    check_levels_mix(mix, "--mix")
    bufs, groups = [], {}
    for i, p in enumerate(pac_paths):
        with open(p, "rb") as fp:
            bufs.append(fp.read())
        try:
            c, _, _, _ = pacfile.read_header(bufs[-1])
        except MrcError as e:
            raise ValueError("%s: not a .pac file (%s)" % (p, e))
        if c.sample_rate % rate_divisor:
            raise ValueError("--rate-divisor %d does not divide the sample rate of %s, %d Hz" % (rate_divisor, p, c.sample_rate))
        groups.setdefault((c.sample_rate, c.n_mdct_lines, c.n_scale_bits, c.n_mant_size_bits), []).append(i)
    out = [None] * len(pac_paths)
    for (rate, lines, scale_bits, mant_bits), members in groups.items():
        h = Handle(sample_rate=rate, n_mdct_lines=lines, n_scale_bits=scale_bits, n_mant_size_bits=mant_bits, device_id=device_id)
        try:
            with PacStore(h, [bufs[i] for i in members]) as store:
                m = store.levels(rate_divisor, mix)
                for k, i in enumerate(members):
                    n = int(store.n_samples_at(rate_divisor)[k])
                    w = rate // rate_divisor if window is None else window
                    nch = 1 if mix == "mid" else int(store.n_channels[k])
                    r = dict(file=pac_paths[i], channels=nch, samples=n, window=w,
                             rms_db=[float(v) for v in m.window_rms_db([k], [0], n)[0, :nch]] if n else [float("-inf")] * nch,
                             loudest_db=None, loudest_start=None, quietest_db=None, quietest_start=None)
                    starts, db = m.grid_levels(k, w)
                    if starts.size:
                        hi, lo = int(np.argmax(db)), int(np.argmin(db))
                        r.update(loudest_db=float(db[hi]), loudest_start=int(starts[hi]), quietest_db=float(db[lo]),
                                 quietest_start=int(starts[lo]))
                    out[i] = r
        finally:
            h.close()
    return out


BAND_ENERGIES_REFUSES = tuple(f for f in LEVELS_REFUSES if f not in ("src", "dst")) + ("--levels", "--levels-window", "--rate-divisor",
                                                                                        "--band-gains-db", "--speed")


def check_band_energies_args(band_energies, hop, band_edges, given):
    """--band-energies as given with --hop and --band-edges -> (hop, edges as float64 or None: the critical bands), or None
    without --band-energies.  It reads src, a `.pac` file, and writes dst, a .npy file: given (flag -> whether it was given, for
    BAND_ENERGIES_REFUSES) must be empty of every encode, decode, excerpt, measure and levels flag; --hop is needed and >= 1;
    --hop and --band-edges need --band-energies."""
    if not band_energies:
        for flag, v in (("--hop", hop), ("--band-edges", band_edges)):
            if v is not None:
                raise ValueError("%s belongs to --band-energies: it needs --band-energies" % flag)
        return None
    for flag in BAND_ENERGIES_REFUSES:
        if given.get(flag):
            raise ValueError("--band-energies writes the band energies of a .pac file and nothing else: it does not go with %s" % flag)
    if hop is None or isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or int(hop) < 1:
        raise ValueError("--band-energies needs --hop N, a positive number of samples, got %r" % (hop,))
    edges = None
    if band_edges is not None:
        from .store import check_band_edges
        try:
            values = [float(v) for v in str(band_edges).split(",")]
        except ValueError:
            raise ValueError("--band-edges: %r is not a comma-separated list of frequencies in Hz" % (band_edges,))
        edges = check_band_edges(values, "--band-edges")
    return int(hop), edges


def _whole_file_energies(pac_path, npy_path, hop, device_id, mix, call):
    """--band-energies and --filterbank-energies: call(store, sample_rate, n_frames) over the whole file from sample 0,
    ceil(samples / hop) frames -> float32 [channels][rows][frames], written to npy_path as a .npy file"""
    from .store import PacStore, check_mix
    check_mix(mix, None, "--mix")
    with open(pac_path, "rb") as fp:
        buf = fp.read()
    try:
        c, _, _, _ = pacfile.read_header(buf)
    except MrcError as e:
        raise ValueError("%s: not a .pac file (%s)" % (pac_path, e))
    h = Handle(sample_rate=c.sample_rate, n_mdct_lines=c.n_mdct_lines, n_scale_bits=c.n_scale_bits,
               n_mant_size_bits=c.n_mant_size_bits, device_id=device_id)
    try:
        with PacStore(h, [buf]) as store:
            n_frames = -(-int(store.n_samples[0]) // hop)
            e = call(store, c.sample_rate, n_frames)[0].cpu().numpy()
    finally:
        h.close()
    with open(npy_path, "wb") as fp:
        np.save(fp, e)
    return e


def band_energies_of_file(pac_path, npy_path, hop, band_edges_hz=None, device_id=0, mix=None):
    """The whole file's band energies (PacStore.band_energy_window: nothing is decoded) -> float32 [channels][bands][frames],
    written to npy_path as a .npy file: frame j is samples [j hop, (j + 1) hop) of the decoded file, ceil(samples / hop)
    frames; band_edges_hz None: store.critical_band_edges of the file's sample rate; mix "mid", "left" or "right": one
    channel."""
    import torch
    from .store import critical_band_edges

    def call(store, sample_rate, n_frames):
        edges = critical_band_edges(sample_rate) if band_edges_hz is None else band_edges_hz
        return store.band_energy_window([0], [0], n_frames, hop, edges, dtype=torch.float32, mix=mix)
    return _whole_file_energies(pac_path, npy_path, hop, device_id, mix, call)


FILTERBANK_ENERGIES_REFUSES = BAND_ENERGIES_REFUSES + ("--band-energies", "--band-edges")
FILTERBANK_FLAGS = ("--mel", "--f-min", "--f-max", "--mel-scale", "--filter-points", "--filter-norm")


def check_filterbank_energies_args(filterbank_energies, hop, mel, f_min, f_max, mel_scale, filter_points, filter_norm, given):
    """--filterbank-energies as given with --hop and its filter flags -> (hop, bank), or None without it.  bank is
    dict(points=float64 points or None, mel=(n, f_min, f_max or None: Nyquist, scale) or None, norm=None or "slaney"): exactly
    one of --mel N and --filter-points; --f-min, --f-max and --mel-scale go with --mel.  Like --band-energies it reads src, a
    `.pac` file, and writes dst, a .npy file: given (flag -> whether it was given, for FILTERBANK_ENERGIES_REFUSES) must be
    empty of every encode, decode, excerpt, measure, levels and band-energy flag; --hop is needed and >= 1; the filter flags
    need --filterbank-energies."""
    flags = dict(zip(FILTERBANK_FLAGS, (mel, f_min, f_max, mel_scale, filter_points, filter_norm)))
    if not filterbank_energies:
        for flag, v in flags.items():
            if v is not None:
                raise ValueError("%s belongs to --filterbank-energies: it needs --filterbank-energies" % flag)
        return None
    for flag in FILTERBANK_ENERGIES_REFUSES:
        if given.get(flag):
            raise ValueError("--filterbank-energies writes the filter-bank energies of a .pac file and nothing else: it does not "
                             "go with %s" % flag)
    if hop is None or isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or int(hop) < 1:
        raise ValueError("--filterbank-energies needs --hop N, a positive number of samples, got %r" % (hop,))
    from .store import MAX_BANDS, MEL_SCALES, check_filter_norm, check_filter_points, mel_points
    if (mel is None) == (filter_points is None):
        raise ValueError("--filterbank-energies needs exactly one of --mel N and --filter-points f0,f1,...")
    bank = dict(points=None, mel=None, norm=filter_norm)
    try:
        check_filter_norm(filter_norm, "--filter-norm")
    except ValueError:
        raise ValueError("--filter-norm: the one norm is slaney, got %r" % (filter_norm,))
    if filter_points is not None:
        for flag in ("--f-min", "--f-max", "--mel-scale"):
            if flags[flag] is not None:
                raise ValueError("%s goes with --mel, not with --filter-points" % flag)
        try:
            values = [float(v) for v in str(filter_points).split(",")]
        except ValueError:
            raise ValueError("--filter-points: %r is not a comma-separated list of frequencies in Hz" % (filter_points,))
        bank["points"] = check_filter_points(values, "--filter-points")
        return int(hop), bank
    if isinstance(mel, bool) or not isinstance(mel, (int, np.integer)) or not 1 <= int(mel) <= MAX_BANDS:
        raise ValueError("--mel: the number of filters is an int in 1..%d, got %r" % (MAX_BANDS, mel))
    scale = "htk" if mel_scale is None else mel_scale
    if scale not in MEL_SCALES:
        raise ValueError("--mel-scale is htk or slaney, got %r" % (mel_scale,))
    lo = 0.0 if f_min is None else f_min
    for flag, v in (("--f-min", lo), ("--f-max", f_max)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v)
                              or v < 0):
            raise ValueError("%s: a frequency in Hz at or above 0, got %r" % (flag, v))
    if f_max is not None:
        try:
            mel_points(int(mel), float(lo), float(f_max), scale)
        except ValueError as e:
            raise ValueError("--f-min, --f-max: %s" % e)
    bank["mel"] = (int(mel), float(lo), None if f_max is None else float(f_max), scale)
    return int(hop), bank


def filterbank_energies_of_file(pac_path, npy_path, hop, bank, device_id=0, mix=None):
    """The whole file's filter-bank energies (PacStore.filterbank_window: nothing is decoded) -> float32
    [channels][filters][frames], written to npy_path as a .npy file, frames as band_energies_of_file's; bank as
    check_filterbank_energies_args gives it (mel with f_max None: up to the file's Nyquist frequency)."""
    import torch
    from .store import mel_points

    def call(store, sample_rate, n_frames):
        points = bank["points"]
        if points is None:
            n, f_min, f_max, scale = bank["mel"]
            try:
                points = mel_points(n, f_min, sample_rate / 2.0 if f_max is None else f_max, scale)
            except ValueError as e:
                raise ValueError("--mel: %s" % e)
        return store.filterbank_window([0], [0], n_frames, hop, points, norm=bank["norm"], dtype=torch.float32, mix=mix)
    return _whole_file_energies(pac_path, npy_path, hop, device_id, mix, call)


STFT_ENERGIES_REFUSES = ("-d", "--no-huffman", "--exact-spread", "--certify", "--bits-per-sample", "--nmr", "--measure", "--target-nmr",
                         "--vbr-nmr", "--vbr-bytes", "--vbr-bits-per-sample", "--vbr-grid", "--levels", "--levels-window",
                         "--band-energies", "--band-edges", "--filterbank-energies", "--filter-points")
STFT_FLAGS = ("--n-fft", "--win-length", "--complex")


def check_stft_energies_args(stft_energies, n_fft, hop, win_length, mel, f_min, f_max, mel_scale, filter_norm, complex_bins, given):
    """--stft-energies as given with its flags -> dict(n_fft, hop, window float64 [n_fft], mel=(n, f_min, f_max or None: the
    output's Nyquist, scale) or None, norm, complex), or None without it.  It reads src, a `.pac` file, and writes dst, a .npy
    file, through PacStore.stft_window on the row -d would decode: given (flag -> whether it was given) must be empty of
    STFT_ENERGIES_REFUSES; --n-fft (store.stft_points_ok's rule) and --hop >= 1 are needed; --win-length W in 1..n_fft: the
    periodic Hann of W taps centred in n_fft points; --f-min, --f-max, --mel-scale and --filter-norm go with --mel; --complex
    does not go with --mel; --n-fft, --win-length and --complex need --stft-energies."""
    if not stft_energies:
        for flag, v in zip(STFT_FLAGS, (n_fft, win_length, complex_bins or None)):
            if v is not None:
                raise ValueError("%s belongs to --stft-energies: it needs --stft-energies" % flag)
        return None
    for flag in STFT_ENERGIES_REFUSES:
        if given.get(flag):
            raise ValueError("--stft-energies writes the short-time Fourier transform of a decoded row and nothing else: it does "
                             "not go with %s" % flag)
    from .store import MAX_BANDS, MEL_SCALES, check_filter_norm, check_stft, hann_window, mel_points, padded_window
    if n_fft is None:
        raise ValueError("--stft-energies needs --n-fft N, the points of a frame")
    if hop is None:
        raise ValueError("--stft-energies needs --hop H, the samples between two frames")
    try:
        check_stft(n_fft, hop, 0, what="--stft-energies")
    except ValueError as e:
        raise ValueError(str(e).replace("stft_window", "--stft-energies"))
    if win_length is not None and not 1 <= int(win_length) <= int(n_fft):
        raise ValueError("--win-length: the frame window holds 1 to --n-fft = %d taps, got %r" % (n_fft, win_length))
    window = padded_window(hann_window(int(n_fft) if win_length is None else int(win_length)), int(n_fft))
    spec = dict(n_fft=int(n_fft), hop=int(hop), window=window, mel=None, norm=filter_norm, complex=bool(complex_bins))
    if mel is None:
        for flag, v in (("--f-min", f_min), ("--f-max", f_max), ("--mel-scale", mel_scale), ("--filter-norm", filter_norm)):
            if v is not None:
                raise ValueError("%s goes with --mel" % flag)
        return spec
    if complex_bins:
        raise ValueError("--complex writes the bins themselves: it does not go with --mel")
    if isinstance(mel, bool) or not isinstance(mel, (int, np.integer)) or not 1 <= int(mel) <= MAX_BANDS:
        raise ValueError("--mel: the number of filters is an int in 1..%d, got %r" % (MAX_BANDS, mel))
    try:
        check_filter_norm(filter_norm, "--filter-norm")
    except ValueError:
        raise ValueError("--filter-norm: the one norm is slaney, got %r" % (filter_norm,))
    scale = "htk" if mel_scale is None else mel_scale
    if scale not in MEL_SCALES:
        raise ValueError("--mel-scale is htk or slaney, got %r" % (mel_scale,))
    lo = 0.0 if f_min is None else f_min
    for flag, v in (("--f-min", lo), ("--f-max", f_max)):
        if v is not None and (not np.isfinite(v) or v < 0):
            raise ValueError("%s: a frequency in Hz at or above 0, got %r" % (flag, v))
    if f_max is not None:
        try:
            mel_points(int(mel), float(lo), float(f_max), scale)
        except ValueError as e:
            raise ValueError("--f-min, --f-max: %s" % e)
    spec["mel"] = (int(mel), float(lo), None if f_max is None else float(f_max), scale)
    return spec


def check_band_gains_db_args(band_gains_db, decode):
    """--band-gains-db as given (None: not given), "LO-HI:DB[,LO-HI:DB...]" -> (edges in Hz float64 [bands + 1], gains float64
    [bands]) for PacStore.decode_window(band_gains=, band_edges_hz=), or None.  LO and HI are frequencies in Hz, 0 <= LO < HI,
    the bands ascending and not overlapping; DB is a number of decibels or -inf.  A gap between two bands becomes a band of
    its own at 0 dB (factor 1.0); what lies below the first LO and at or above the last HI is left alone.  It changes the
    spectrum of a decode: refused without -d."""
    if band_gains_db is None:
        return None
    if not decode:
        raise ValueError("--band-gains-db changes the spectrum of a decode: it needs -d")
    from .store import MAX_BANDS, gains_from_db
    edges, db = [], []
    for part in str(band_gains_db).split(","):
        try:
            span, level = part.split(":")
            lo, hi = span.split("-")                     # (frequencies are not negative: the one '-' separates them)
            lo, hi, level = float(lo), float(hi), float(level)
        except ValueError:
            raise ValueError("--band-gains-db: %r is not LO-HI:DB (frequencies in Hz, decibels or -inf)" % (part,))
        if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi):
            raise ValueError("--band-gains-db: %r: the band must be 0 <= LO < HI, finite" % (part,))
        if np.isnan(level) or level == np.inf:
            raise ValueError("--band-gains-db: %r: DB must be a finite number of decibels or -inf" % (part,))
        if edges and lo < edges[-1]:
            raise ValueError("--band-gains-db: %r starts below the end of the band before it: bands ascend and do not overlap" % (part,))
        if edges and lo > edges[-1]:
            db.append(0.0)                               # the gap: a band at 0 dB
        if not edges or lo > edges[-1]:
            edges.append(lo)
        edges.append(hi)
        db.append(level)
    if len(db) > MAX_BANDS:
        raise ValueError("--band-gains-db: %d bands (gaps included) are more than %d" % (len(db), MAX_BANDS))
    return np.array(edges, np.float64), gains_from_db(db)


def check_speed_args(speed, decode):
    """--speed as given (None: not given), "NUM/DEN" or "NUM" -> (num, den), positive ints, or None.  It plays a decode faster
    or slower: refused without -d."""
    if speed is None:
        return None
    if not decode:
        raise ValueError("--speed plays a decode faster or slower: it needs -d")
    try:
        parts = str(speed).split("/")
        num, den = (int(parts[0]), 1) if len(parts) == 1 else (int(parts[0]), int(parts[1]))
        if len(parts) > 2 or num < 1 or den < 1:
            raise ValueError
    except ValueError:
        raise ValueError("--speed: %r is not NUM/DEN, two positive whole numbers" % (speed,))
    return num, den


def check_ir_args(ir, decode):
    """--ir as given (None: not given) -> the path or None.  It reverberates a decode: refused without -d."""
    if ir is not None and not decode:
        raise ValueError("--ir reverberates a decode with an impulse response: it needs -d")
    return ir


def read_ir(path, rate_out):
    """the impulse response of --ir -> float64 [taps] at rate_out Hz.  A .npy file holds a 1-D array of numbers that is taken as
    it is (it carries no rate: it must be sampled at the output rate); anything else is a mono 16-bit PCM WAV, read with
    read_wav and brought from its own rate to rate_out by store.ir_at_rate."""
    from .store import check_impulse_responses, ir_at_rate
    if str(path).lower().endswith(".npy"):
        try:
            taps = np.load(path, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError("--ir: %s: %s" % (path, e))
        try:
            return check_impulse_responses([taps], "--ir")[1]
        except ValueError as e:
            raise ValueError("%s (%s)" % (e, path))
    try:
        rate, n_ch, num_samples, x = read_wav(path, 1)
    except (OSError, ValueError) as e:
        raise ValueError("--ir: %s: %s" % (path, e))
    if n_ch != 1 or num_samples < 1:
        raise ValueError("--ir: %s: a WAV impulse response must have one channel and at least one sample, got %d x %d"
                         % (path, n_ch, num_samples))
    try:
        return ir_at_rate(x[0, :num_samples], int(rate), int(rate_out))
    except ValueError as e:
        raise ValueError("--ir: %s: %s" % (path, e))


def check_array_ir_args(array_ir, ir, decode):
    """--array-ir as given (None: not given) -> the path or None.  It decodes one channel through the C responses of a microphone
    array into a C-channel WAV: refused without -d, and together with --ir (one room or one array)."""
    if array_ir is None:
        return None
    if not decode:
        raise ValueError("--array-ir decodes a file through the responses of a microphone array: it needs -d")
    if ir is not None:
        raise ValueError("--array-ir and --ir both convolve the decoded file: give one of them")
    return array_ir


def read_array_ir(path, rate_out):
    """the impulse responses of --array-ir -> a list of C float64 [taps] at rate_out Hz, 1 <= C <= store.MAX_ROUTE_CHANNELS.  A
    .npy file holds a [C][taps] array of numbers taken as it is (sampled at the output rate); anything else is a C-channel
    16-bit PCM WAV, read with read_wav, each channel brought from the file's rate to rate_out by store.ir_at_rate."""
    from .store import MAX_ROUTE_CHANNELS, check_impulse_responses, ir_at_rate
    what = "--array-ir"
    if str(path).lower().endswith(".npy"):
        try:
            taps = np.load(path, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError("%s: %s: %s" % (what, path, e))
        if taps.ndim != 2 or not 1 <= taps.shape[0] <= MAX_ROUTE_CHANNELS:
            raise ValueError("%s: %s: the array must be [C][taps] with 1 to %d microphones, got shape %s"
                             % (what, path, MAX_ROUTE_CHANNELS, taps.shape))
        try:
            offsets, flat = check_impulse_responses(list(taps), what)
        except ValueError as e:
            raise ValueError("%s (%s)" % (e, path))
        return [flat[offsets[j]:offsets[j + 1]] for j in range(taps.shape[0])]
    try:
        rate, n_ch, num_samples, x = read_wav(path, 1)
    except (OSError, ValueError) as e:
        raise ValueError("%s: %s: %s" % (what, path, e))
    if not 1 <= n_ch <= MAX_ROUTE_CHANNELS or num_samples < 1:
        raise ValueError("%s: %s: a WAV of impulse responses must have 1 to %d channels and at least one sample, got %d x %d"
                         % (what, path, MAX_ROUTE_CHANNELS, n_ch, num_samples))
    try:
        return [ir_at_rate(x[c, :num_samples], int(rate), int(rate_out)) for c in range(n_ch)]
    except ValueError as e:
        raise ValueError("%s: %s: %s" % (what, path, e))


CODEC_SETTINGS = ("sample_rate", "n_mdct_lines", "n_scale_bits", "n_mant_size_bits")   # what a .pac header says of its codec


def _levels_of_mix(store, rate_divisor, mix):
    """the LevelMap of the channels decode_window gives under mix: every channel, the mid, or the left / right column of the
    per-channel energies (a mono file its own)"""
    if mix not in ("left", "right"):
        return store.levels(rate_divisor, mix)
    from .levels import LevelMap
    entry_offset, blocks, energy = store.block_energy(rate_divisor, None)
    cfg, per_file = store._handle.cfg, []
    for f in range(len(store)):
        lo, hi, nch = int(entry_offset[f]), int(entry_offset[f + 1]), int(store.n_channels[f])
        per_file.append(dict(blocks=blocks[lo:hi:nch], energy=energy[lo:hi].reshape(-1, nch)[:, min(("left", "right").index(mix), nch - 1)],
                             n_samples=int(store.n_samples[f]) // rate_divisor))
    return LevelMap(per_file, cfg.n_mdct_lines, rate_divisor, cfg.n_short)


def decode_pac_file(pac_path, wav_path, device_id=0, excerpt=None, rate_divisor=1, mix=None, sample_rate=None, overlay=None,
                    band_gains=None, speed=None, ir=None, stft=None, array_ir=None):
    """excerpt: None (the whole file, mrc_decode_pac_pcm16) or (start, samples): that many samples from sample `start` on
    (samples None: to the end of the file), decoded through a one-file PacStore -- only the blocks the excerpt overlaps are
    parsed and synthesised; what lies outside the file is silence.  rate_divisor 2 or 4: at that fraction of the sample rate,
    through the store as well (excerpt None: the whole file); start and samples count samples at the reduced rate, which the
    WAV's header carries.  mix "mid", "left" or "right": a one-channel WAV of that channel (mid: (L + R) / 2, formed on the
    MDCT lines), through the store as well.  sample_rate: None or the rate in Hz to decode at, through the store as well
    (store.resample_plan picks the divisor and the fraction; rate_divisor must be 1): start and samples count samples at
    that rate, which the WAV's header carries.  overlay: None or (path, snr_db, start): a second `.pac` file of the same codec
    settings added under the excerpt in ONE PacStore.decode_window_sum call of two terms -- the file at 1.0 and the overlay,
    from its sample `start` on (negative: it begins that far into the excerpt), at the factor that puts the excerpt snr_db
    above it (levels.LevelMap.gains_for_snr over the excerpt, from the block energies; the factor is printed).
    band_gains: None or (edges in Hz, gains) of check_band_gains_db_args: the file's MDCT lines multiplied band by band before
    the inverse transform (PacStore.decode_window(band_gains=)), through the store as well; the overlay is left as it is, and
    its level is set against the unshaped excerpt.
    speed: None or (num, den): the file read num / den times as fast (PacStore.decode_window(speed_factors=)), through the store
    as well: start and samples count output samples, the whole file is n_samples_resampled of the combined ratio, the WAV's
    header carries the output rate unchanged; the overlay stays at speed 1, a second term of the same one call, its level set
    against the stretch of source under the excerpt (PacStore.source_spans).
    ir: None or the path of an impulse response (read_ir: a .npy array at the output rate, or a mono 16-bit WAV brought to it):
    the file convolved with it through the store as well (PacStore.decode_window(ir_index=)), last of all -- at the output rate,
    after the speed; the overlay stays dry, the same one call.  The output keeps the length it has without --ir.
    array_ir: None or the path of the C impulse responses of a microphone array (read_array_ir): ONE channel of the file (mix; None:
    "mid" for a stereo file) through every one of them in one PacStore.decode_window_routed call -- the file is parsed,
    synthesised and transformed once -- into a C-channel WAV (with stft: C channels of spectra); the overlay is dry on every
    channel.  Not together with ir.
    stft: None, or check_stft_energies_args' dict: wav_path is then a .npy file and receives PacStore.stft_window of the very row
    the other arguments describe, (samples - n_fft) // hop + 1 whole frames of it (none: an empty array), in place of the WAV
    -> the array as written.
    -> int16 [nCh][samples] as written."""
    with open(pac_path, "rb") as fp:
        buf = fp.read()
    try:
        cfg, _, _, _ = pacfile.read_header(buf)
    except MrcError as e:
        if stft is None:
            raise
        raise ValueError("%s: not a .pac file (%s)" % (pac_path, e))
    bufs = [buf]
    if overlay is not None:
        with open(overlay[0], "rb") as fp:
            bufs.append(fp.read())
        try:
            other, _, _, _ = pacfile.read_header(bufs[1])
        except MrcError as e:
            raise ValueError("--overlay: %s: not a .pac file (%s)" % (overlay[0], e))
        for name in CODEC_SETTINGS:
            if getattr(other, name) != getattr(cfg, name):
                raise ValueError("--overlay: %s differs: %s has %d, %s has %d"
                                 % (name, pac_path, getattr(cfg, name), overlay[0], getattr(other, name)))
    rate_divisor = check_rate_divisor_args(rate_divisor, True)
    if cfg.sample_rate % rate_divisor:
        raise ValueError("--rate-divisor %d does not divide the file's sample rate, %d Hz" % (rate_divisor, cfg.sample_rate))
    mix = check_mix_args(mix, True)
    resample = None
    if check_sample_rate_args(sample_rate, True, rate_divisor != 1) is not None:
        from .store import resample_plan
        rate_divisor, up, down = resample_plan(cfg.sample_rate, int(sample_rate))
        resample = None if up == down else (up, down)
    ratio = None
    if speed is not None:
        from .store import speed_ratios
        try:
            ratio = speed_ratios(resample, [speed])[0]
        except ValueError as e:
            raise ValueError("--speed: %s" % e)
    if (rate_divisor != 1 or mix is not None or resample is not None or overlay is not None or band_gains is not None
            or speed is not None or ir is not None or stft is not None or array_ir is not None) and excerpt is None:
        excerpt = (0, None)
    taps = None if ir is None else read_ir(ir, cfg.sample_rate // rate_divisor if sample_rate is None else int(sample_rate))
    mics = None if array_ir is None else read_array_ir(array_ir, cfg.sample_rate // rate_divisor if sample_rate is None else int(sample_rate))
    h = Handle(sample_rate=cfg.sample_rate, n_mdct_lines=cfg.n_mdct_lines, n_scale_bits=cfg.n_scale_bits,
               n_mant_size_bits=cfg.n_mant_size_bits, device_id=device_id)
    try:
        if excerpt is None:
            inter = h.decode_pac_pcm16(buf)[0]      # [samples][nCh] in WAV order, parsed and decoded on the device
        else:
            from .store import PacStore
            with PacStore(h, bufs) as store:
                start, samples = excerpt
                if samples is None:
                    n = store.n_samples_resampled(*ratio, rate_divisor) if ratio is not None else \
                        store.n_samples_at(rate_divisor) if resample is None else store.n_samples_resampled(*resample, rate_divisor)
                    samples = max(0, int(n[0]) - start)
                shaped = {} if band_gains is None else dict(band_edges_hz=band_gains[0])
                if speed is not None:                    # the file at its speed; the overlay, a second term, at speed 1
                    shaped.update(speed_factors=[speed, (1, 1)], speed_index=[0] if overlay is None else [[0, 1]])
                if taps is not None:                     # the file through the room; the overlay dry
                    store.set_impulse_responses([taps])
                    shaped.update(ir_index=[0] if overlay is None else [[0, -1]])
                if mics is not None:                     # one channel of the file through every microphone; the overlay dry
                    if mix is None and int(store.n_channels.max()) > 1:
                        mix = "mid"
                    store.set_impulse_responses(mics)
                    from .store import array_routes
                    routes = dict(zip(("route_gains", "route_irs"), array_routes([0] if overlay is None else [[0, -1]], len(mics))))
                if stft is not None:                     # the same row, framed and transformed instead of written
                    from .store import mel_bin_weights, mel_points
                    rate_out = cfg.sample_rate // rate_divisor if sample_rate is None else int(sample_rate)
                    frames = max(0, (samples - stft["n_fft"]) // stft["hop"] + 1)
                    spectrum = dict(frame_window=stft["window"], output="complex" if stft["complex"] else "power")
                    if stft["mel"] is not None:
                        n_mel, f_min, f_max, scale = stft["mel"]
                        try:
                            points = mel_points(n_mel, f_min, rate_out / 2.0 if f_max is None else f_max, scale)
                        except ValueError as e:
                            raise ValueError("--mel: %s" % e)
                        spectrum.update(output="bank", bank=mel_bin_weights(stft["n_fft"], rate_out, points, stft["norm"]))
                    window = lambda files, starts, _samples, **kw: store.stft_window(files, starts, frames, stft["hop"], stft["n_fft"],
                                                                                     **spectrum, **kw)
                    window_sum = lambda files, starts, gains, _samples, **kw: window(files, starts, _samples, gains=gains, **kw)
                    routed = window                      # (routes in the place of gains: 1-D one term per item, or [n][K])
                else:
                    window, window_sum = store.decode_window, store.decode_window_sum
                    # (files, starts, the routes and every per-term argument keep the one shape they were built in: a 1-D list is
                    # rows of one term each)
                    routed = lambda files, starts, _samples, route_gains, route_irs, **kw: store.decode_window_routed(
                        files, starts, route_gains, route_irs, _samples,
                        item_offsets=np.arange(len(files) + 1) if np.ndim(files) == 1 else None, **kw)
                if overlay is None:
                    if band_gains is not None:
                        shaped["band_gains"] = band_gains[1]
                    if mics is not None:
                        got = routed([0], [start], samples, rate_divisor=rate_divisor, mix=mix, resample=resample, **routes, **shaped)
                    else:
                        got = window([0], [start], samples, rate_divisor=rate_divisor, mix=mix, resample=resample, **shaped)
                else:
                    # the levels live at the rate divisor's rate: the excerpt's span there (the whole of it, rounded outwards)
                    up, down = resample if resample is not None else (1, 1)
                    at = lambda v: v * down // up
                    first, span = at(start), max(1, -(-(start + samples) * down // up) - at(start))
                    if ratio is not None:                # the stretch of source under the sped-up excerpt
                        first, span = (int(v[0]) for v in store.source_spans([start], samples, [ratio], [0], rate_divisor))
                        span = max(1, span)
                    gain = float(_levels_of_mix(store, rate_divisor, mix).gains_for_snr(
                        overlay[1], [0], [first], [1], [at(overlay[2])], span)[0]) if samples else 1.0
                    print("overlay: %s at a factor of %.9g (%g dB under the excerpt)" % (overlay[0], gain, overlay[1]))
                    if band_gains is not None:           # (the overlay's row: ones)
                        shaped["band_gains"] = np.stack([band_gains[1], np.ones_like(band_gains[1])])[None]
                    if mics is not None:                 # (the overlay's factor on every channel)
                        routes["route_gains"] = routes["route_gains"] * np.array([1.0, gain])[None, :, None]
                        got = routed([[0, 1]], [[start, overlay[2]]], samples, rate_divisor=rate_divisor, mix=mix,
                                     resample=resample, **routes, **shaped)
                    else:
                        got = window_sum([[0, 1]], [[start, overlay[2]]], [[1.0, gain]], samples, rate_divisor=rate_divisor,
                                         mix=mix, resample=resample, **shaped)
                inter = got[0].cpu().numpy() if stft is not None else np.ascontiguousarray(got[0].cpu().numpy().T)
    finally:
        h.close()
    if stft is not None:
        with open(wav_path, "wb") as fp:
            np.save(fp, inter)
        return inter
    data = inter.astype("<i2", copy=False)
    with open(wav_path, "wb") as fp:
        fp.write(wav_header(inter.shape[1], data.nbytes, cfg.sample_rate // rate_divisor if sample_rate is None else int(sample_rate)))
        fp.write(data.tobytes())
    return inter.T


def check_append_args(append, crossfade, decode, others):
    """--append and --crossfade as given (None: not given) -> (path, crossfade in samples), or None without --append.  --append
    decodes src followed by a second file in one call: refused without -d, and with every flag in `others` that is given (it
    composes with --rate-divisor, --sample-rate and --mix alone); --crossfade is refused without --append and is a whole number
    of output samples >= 0."""
    if append is None:
        if crossfade is not None:
            raise ValueError("--crossfade belongs to --append: it needs --append")
        return None
    if not decode:
        raise ValueError("--append decodes src followed by a second .pac file: it needs -d")
    for flag, given in others.items():
        if given:
            raise ValueError("--append composes with --rate-divisor, --sample-rate and --mix: it does not take %s" % flag)
    if crossfade is not None and (isinstance(crossfade, bool) or not isinstance(crossfade, (int, np.integer)) or crossfade < 0):
        raise ValueError("--crossfade: %r is not a whole number of samples >= 0" % (crossfade,))
    return str(append), (0 if crossfade is None else int(crossfade))


def decode_appended_files(pac_path, wav_path, append, device_id=0, rate_divisor=1, mix=None, sample_rate=None):
    """-d --append: src followed by append[0], the two overlapping by append[1] output samples over which src fades out and
    the second file fades in (0: they abut), in ONE PacStore.decode_window_sum call of two terms with spans
    (store.concat_spans); each file is parsed and synthesised under its own piece only.  rate_divisor, mix and sample_rate
    as decode_pac_file's.  Both files carry the same codec settings and channel count (a mix makes one channel of either).
    -> int16 [nCh][samples] as written."""
    bufs = []
    for path in (pac_path, append[0]):
        with open(path, "rb") as fp:
            bufs.append(fp.read())
    try:
        (cfg, nch, _, _), (other, nch2, _, _) = pacfile.read_header(bufs[0]), pacfile.read_header(bufs[1])
    except MrcError as e:
        raise ValueError("--append: not a .pac file (%s)" % e)
    for name in CODEC_SETTINGS:
        if getattr(other, name) != getattr(cfg, name):
            raise ValueError("--append: %s differs: %s has %d, %s has %d" % (name, pac_path, getattr(cfg, name), append[0], getattr(other, name)))
    mix = check_mix_args(mix, True)
    if mix is None and nch != nch2:
        raise ValueError("--append: %s has %d channel(s), %s has %d: give --mix" % (pac_path, nch, append[0], nch2))
    rate_divisor = check_rate_divisor_args(rate_divisor, True)
    if cfg.sample_rate % rate_divisor:
        raise ValueError("--rate-divisor %d does not divide the file's sample rate, %d Hz" % (rate_divisor, cfg.sample_rate))
    resample = None
    if check_sample_rate_args(sample_rate, True, rate_divisor != 1) is not None:
        from .store import resample_plan
        rate_divisor, up, down = resample_plan(cfg.sample_rate, int(sample_rate))
        resample = None if up == down else (up, down)
    rate_out = cfg.sample_rate // rate_divisor if sample_rate is None else int(sample_rate)
    h = Handle(sample_rate=cfg.sample_rate, n_mdct_lines=cfg.n_mdct_lines, n_scale_bits=cfg.n_scale_bits,
               n_mant_size_bits=cfg.n_mant_size_bits, device_id=device_id)
    try:
        from .store import PacStore, concat_spans
        with PacStore(h, bufs) as store:
            n = store.n_samples_at(rate_divisor) if resample is None else store.n_samples_resampled(*resample, rate_divisor)
            try:
                starts, first, length, fin, fout = concat_spans([[int(n[0]), int(n[1])]], [[0, 0]], crossfade=append[1])
            except ValueError as e:
                raise ValueError("--crossfade: %s" % e)
            got = store.decode_window_sum([[0, 1]], starts, [[1.0, 1.0]], int(first[0, 1] + length[0, 1]), rate_divisor=rate_divisor, mix=mix,
                                          resample=resample, span_first=first, span_len=length, fade_in=fin, fade_out=fout)
            inter = np.ascontiguousarray(got[0].cpu().numpy().T)
    finally:
        h.close()
    data = inter.astype("<i2", copy=False)
    with open(wav_path, "wb") as fp:
        fp.write(wav_header(inter.shape[1], data.nbytes, rate_out))
        fp.write(data.tobytes())
    return inter.T


def measure_files(wav_path, pac_paths, bits_per_sample=None, device_id=0, exact_spread=False):
    """The NMR of each `.pac` file in pac_paths against the WAV it was coded from, in one library call (mrc_pac_nmr).
    bits_per_sample: one value per file (or None) for the report.  -> one dict per file: file, bits_per_sample and the
    four numbers of pacfile.measure_nmr."""
    bufs = []
    for p in pac_paths:
        with open(p, "rb") as fp:
            bufs.append(fp.read())
    rate, n_ch, num_samples, pcm = read_wav_pcm(wav_path)
    cfg = None
    for p, buf in zip(pac_paths, bufs):          # the WAV must be what every file was coded from: refused before any device use
        try:
            c, nch, _, _ = pacfile.read_header(buf)
        except MrcError as e:
            raise ValueError("%s: not a .pac file (%s)" % (p, e))
        if (c.sample_rate, nch) != (rate, n_ch):
            raise ValueError("%s holds %d channel(s) at %d Hz, %s %d channel(s) at %d Hz: not its source"
                             % (p, nch, c.sample_rate, wav_path, n_ch, rate))
        if cfg is None:
            cfg = c
    h = Handle(sample_rate=cfg.sample_rate, n_mdct_lines=cfg.n_mdct_lines, n_scale_bits=cfg.n_scale_bits,
               n_mant_size_bits=cfg.n_mant_size_bits, device_id=device_id)
    try:
        if exact_spread:
            h.set_option(1, 1)
        res = pacfile.measure_nmr(h, bufs, np.ascontiguousarray(pcm[:, :num_samples]))
    finally:
        h.close()
    bps = [None] * len(pac_paths) if bits_per_sample is None else list(bits_per_sample)
    return [dict(file=p, bits_per_sample=b, **r) for p, b, r in zip(pac_paths, bps, res)]


def _print_nmr(ap, a, paths, bps):
    try:
        res = measure_files(a.src, paths, bps, a.device, a.exact_spread)
    except ValueError as e:
        ap.error(str(e))
    for r in res:
        print(json.dumps(r))


def _nmr_fields(r):
    """the NMR tail of a report's JSON line: one number each, or (a ladder's report) one per rung"""
    plain = lambda v, typ: [typ(x) for x in v] if np.ndim(v) else v
    return dict(nmr_total_db=plain(r["nmr_total_db"], float), nmr_max_db=plain(r["nmr_max_db"], float),
                disturbed_blocks=plain(r["disturbed_blocks"], int), n_blocks=r["n_blocks"])


def _vbr_fields(r):
    return dict(ceiling_ratio=r["ceiling_ratio"], bits_per_sample=r["bits_per_sample"], coded_bits=r["coded_bits"],
                capped_bands=r["capped_bands"], **_nmr_fields(r))


def _join_vbr_grid(argv):
    """argv with "--vbr-grid VALUE" written "--vbr-grid=VALUE": a grid usually starts at a negative LO, and argparse takes
    "-30:0.25:256" (a leading minus, yet no number) for an option and never hands it to --vbr-grid as its value."""
    argv, out, i = list(argv), [], 0
    while i < len(argv):
        if argv[i] == "--":
            return out + argv[i:]
        if argv[i] == "--vbr-grid" and i + 1 < len(argv) and ":" in argv[i + 1]:
            out.append("--vbr-grid=" + argv[i + 1])
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Encode a mono or stereo 16-bit WAV to .pac (or, with -d, decode a .pac to WAV) "
                                             "on an MI355X")
    ap.add_argument("src", nargs="?", default=None)
    ap.add_argument("dst", nargs="?", default=None)
    ap.add_argument("-d", "--decode", action="store_true")
    ap.add_argument("--no-huffman", action="store_true")
    ap.add_argument("--exact-spread", action="store_true",
                    help="masker spreading operation by operation as in psychoac.py:68-78 (slower kernel)")
    ap.add_argument("--certify", action="store_true",
                    help="report how many integer decisions of the encode lay within a guard band of floating-point rounding "
                         "(quantiser edges, bit-allocation ties, M/S threshold, peak test); if any did, encode again with "
                         "--exact-spread and say whether the bytes are the same")
    ap.add_argument("--bits-per-sample", default=None, metavar="LIST",
                    help="target bits per sample (default 2.86, the reference's); several, comma separated (e.g. 1.5,2.86,4), "
                         "encode a rate ladder in one call, and dst must then contain {bps}")
    ap.add_argument("--nmr", action="store_true",
                    help="after the encode, print one JSON line per file written with its noise-to-mask ratio against src")
    ap.add_argument("--measure", action="store_true",
                    help="do not encode: print the noise-to-mask ratio of the existing dst file(s) against src, one JSON "
                         "line per file (dst may hold {bps} with --bits-per-sample)")
    ap.add_argument("--target-nmr", default=None, metavar="DB",
                    help="with an ascending --bits-per-sample list of two rates or more: write ONE file to dst, the lowest "
                         "rate whose nmr_total_db against src is <= DB (the top rate if none is), and print one JSON line")
    ap.add_argument("--vbr-nmr", default=None, metavar="DB",
                    help="constant-quality VBR: no bit rate; every band gets the fewest bits that keep its noise-to-mask ratio "
                         "<= DB.  Writes ONE file to dst and prints one JSON line (bits per sample, capped bands, NMR)")
    ap.add_argument("--vbr-bytes", default=None, metavar="N",
                    help="constant-quality VBR to a size: the tightest noise-to-mask ceiling of the grid whose whole file is "
                         "<= N bytes, searched in one call.  Writes ONE file to dst and prints one JSON line (--vbr-nmr's "
                         "plus chosen_db, met, probes)")
    ap.add_argument("--vbr-bits-per-sample", default=None, metavar="X",
                    help="--vbr-bytes with N = header + floor(X * coded_samples * channels / 8) + 4 * chunks")
    ap.add_argument("--vbr-grid", default=None, metavar="LO:STEP:N",
                    help="the ceilings --vbr-bytes / --vbr-bits-per-sample search: LO + i * STEP dB, i < N <= 256 "
                         "(default -30:0.25:256)")
    ap.add_argument("--start", type=int, default=None, metavar="S",
                    help="with -d: decode an excerpt that starts at sample S of the decoded file (default 0)")
    ap.add_argument("--samples", type=int, default=None, metavar="N",
                    help="with -d: decode an excerpt of N samples (default: to the end of the file)")
    ap.add_argument("--rate-divisor", type=int, default=None, metavar="D",
                    help="with -d: decode at 1/D of the sample rate (D = 2 or 4) straight from the MDCT lines; the WAV says "
                         "sample_rate // D, and --start / --samples count samples at that rate")
    ap.add_argument("--sample-rate", type=int, default=None, metavar="HZ",
                    help="with -d: decode at HZ samples per second (16000 from a 48 kHz file: half-rate synthesis, then a 2 / 3 "
                         "polyphase resampler on the device); the WAV says HZ, and --start / --samples count samples at HZ; "
                         "does not go with --rate-divisor")
    ap.add_argument("--mix", default=None, metavar="CH",
                    help="with -d: write a one-channel WAV, CH = mid ((L + R) / 2 of a stereo file, formed on the MDCT lines), "
                         "left or right; composes with --rate-divisor, --start and --samples")
    ap.add_argument("--overlay", default=None, metavar="PAC",
                    help="with -d: add a second .pac file of the same codec settings under the decode, src at 1.0 and PAC at the "
                         "factor that puts src --snr-db above it over the excerpt (from the block energies), in one call on the "
                         "device; composes with --start, --samples, --mix, --rate-divisor and --sample-rate")
    ap.add_argument("--snr-db", default=None, metavar="DB", help="with --overlay: the level of src over the overlay in dB")
    ap.add_argument("--overlay-start", type=int, default=None, metavar="N",
                    help="with --overlay: the overlay's sample that falls on the excerpt's first (default 0; negative: the "
                         "overlay begins that many samples into the excerpt)")
    ap.add_argument("--append", default=None, metavar="PAC",
                    help="with -d: decode src followed by this .pac file (same codec settings) in one call of two terms with "
                         "spans; composes with --rate-divisor, --sample-rate and --mix")
    ap.add_argument("--crossfade", type=int, default=None, metavar="N",
                    help="with --append: the two files overlap by N output samples, src fading out and PAC fading in linearly")
    ap.add_argument("--band-gains-db", default=None, metavar="LO-HI:DB,...",
                    help="with -d: multiply the MDCT lines between LO and HI Hz by DB decibels (-inf: silence them) before the "
                         "inverse transform, e.g. 0-300:-inf,3400-24000:-inf for a telephone band; bands ascend and do not "
                         "overlap, gaps stay at 0 dB; composes with --start, --samples, --rate-divisor, --mix, --sample-rate and "
                         "--overlay (the overlay is left as it is)")
    ap.add_argument("--speed", default=None, metavar="NUM/DEN",
                    help="with -d: play the file NUM/DEN times as fast (11/10: speed perturbation) through the resident store; the "
                         "WAV's rate is unchanged, --start / --samples count output samples; composes with --sample-rate, "
                         "--rate-divisor, --mix, --band-gains-db and --overlay (the overlay stays at speed 1)")
    ap.add_argument("--ir", default=None, metavar="FILE",
                    help="with -d: convolve the decoded file with the impulse response in FILE, a .npy float array sampled at the "
                         "output rate or a mono 16-bit WAV (brought to the output rate), through the resident store on the device; "
                         "composes with --sample-rate, --speed, --mix, --overlay (the overlay stays dry), --start and --samples")
    ap.add_argument("--array-ir", default=None, metavar="FILE",
                    help="with -d: decode ONE channel of the file (--mix; mid by default for a stereo file) through the C impulse "
                         "responses in FILE, a .npy float array [C][taps] sampled at the output rate or a C-channel 16-bit WAV "
                         "(brought to the output rate), into a C-channel WAV -- one microphone each, the file parsed and "
                         "transformed once; composes with what --ir composes with and is refused together with --ir")
    ap.add_argument("--levels", nargs="+", default=None, metavar="PAC",
                    help="no src, no dst: print one JSON line per .pac file with its channels, samples, RMS level per channel "
                         "(dB re full scale) and its loudest and quietest window on the short-block grid, from the block "
                         "energies of the MDCT lines (nothing is decoded); composes with --rate-divisor and --mix mid")
    ap.add_argument("--levels-window", type=int, default=None, metavar="N",
                    help="with --levels: the window in samples (default: one second)")
    ap.add_argument("--band-energies", action="store_true",
                    help="src is a .pac file, dst a .npy file: write the whole file's band energies, float32 "
                         "[channels][bands][frames], frame j = samples [j N, (j + 1) N) for --hop N, from the MDCT lines (nothing "
                         "is decoded); composes with --band-edges and --mix")
    ap.add_argument("--hop", type=int, default=None, metavar="N", help="with --band-energies: the frame length in samples")
    ap.add_argument("--band-edges", default=None, metavar="F0,F1,...",
                    help="with --band-energies: the band edges in Hz, increasing (default: 0, the codec's critical-band "
                         "limits below Nyquist, Nyquist)")
    ap.add_argument("--filterbank-energies", action="store_true",
                    help="src is a .pac file, dst a .npy file: write the whole file's energies in a bank of triangular filters, "
                         "float32 [channels][filters][frames], frames as --band-energies' (--hop N), from the MDCT lines (nothing "
                         "is decoded); needs --mel N or --filter-points; composes with --filter-norm and --mix")
    ap.add_argument("--mel", type=int, default=None, metavar="N",
                    help="with --filterbank-energies: N mel filters from --f-min (default 0) to --f-max (default Nyquist)")
    ap.add_argument("--f-min", type=float, default=None, metavar="HZ", help="with --mel: the first filter's lower foot")
    ap.add_argument("--f-max", type=float, default=None, metavar="HZ", help="with --mel: the last filter's upper foot")
    ap.add_argument("--mel-scale", default=None, metavar="htk|slaney", help="with --mel: the mel scale (default htk)")
    ap.add_argument("--filter-points", default=None, metavar="F0,F1,...",
                    help="with --filterbank-energies: the filters' points in Hz, increasing; filter q is the triangle over "
                         "points q, q + 1, q + 2")
    ap.add_argument("--filter-norm", default=None, metavar="slaney",
                    help="with --filterbank-energies: slaney divides every filter by half its width in Hz")
    ap.add_argument("--stft-energies", action="store_true",
                    help="src is a .pac file, dst a .npy file: write the short-time Fourier transform of the row -d would decode, "
                         "float32 power [channels][N / 2 + 1][frames] for --n-fft N --hop H (frame j: samples [j H, j H + N), "
                         "--samples rounded down to whole frames); --mel N: the totals of N mel filters on the bins; --complex: "
                         "the complex64 bins; composes with --start, --samples, --rate-divisor, --sample-rate, --mix, --speed, "
                         "--ir, --band-gains-db, --overlay and --snr-db")
    ap.add_argument("--n-fft", type=int, default=None, metavar="N",
                    help="with --stft-energies: the points of a frame, even, 16..2048, factors 2, 3 and 5 only")
    ap.add_argument("--win-length", type=int, default=None, metavar="W",
                    help="with --stft-energies: the periodic Hann window's taps, centred in the N points (default N)")
    ap.add_argument("--complex", action="store_true", help="with --stft-energies: write the complex bins, not their power")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(_join_vbr_grid(sys.argv[1:] if argv is None else argv))
    try:
        given = {
            "src": a.src is not None, "dst": a.dst is not None, "-d": a.decode, "--no-huffman": a.no_huffman,
            "--exact-spread": a.exact_spread, "--certify": a.certify, "--bits-per-sample": a.bits_per_sample is not None,
            "--nmr": a.nmr, "--measure": a.measure, "--target-nmr": a.target_nmr is not None, "--vbr-nmr": a.vbr_nmr is not None,
            "--vbr-bytes": a.vbr_bytes is not None, "--vbr-bits-per-sample": a.vbr_bits_per_sample is not None,
            "--vbr-grid": a.vbr_grid is not None, "--start": a.start is not None, "--samples": a.samples is not None,
            "--sample-rate": a.sample_rate is not None}
        given_energies = dict(
            given, **{"--levels": a.levels is not None, "--levels-window": a.levels_window is not None,
                      "--rate-divisor": a.rate_divisor is not None, "--band-gains-db": a.band_gains_db is not None,
                      "--speed": a.speed is not None, "--ir": a.ir is not None, "--array-ir": a.array_ir is not None})
        stft = check_stft_energies_args(a.stft_energies, a.n_fft, a.hop, a.win_length, a.mel, a.f_min, a.f_max, a.mel_scale, a.filter_norm,
                                        a.complex, dict(given_energies, **{"--band-energies": a.band_energies,
                                                                           "--band-edges": a.band_edges is not None,
                                                                           "--filterbank-energies": a.filterbank_energies,
                                                                           "--filter-points": a.filter_points is not None}))
        # (--hop and the mel flags are --stft-energies' when it is given: the line-energy checks do not see them)
        mel_flags = (None,) * 4 if stft is not None else (a.mel, a.f_min, a.f_max, a.mel_scale)
        bank = check_filterbank_energies_args(a.filterbank_energies, a.hop, *mel_flags, a.filter_points,
                                              None if stft is not None else a.filter_norm,
                                              dict(given_energies, **{"--band-energies": a.band_energies,
                                                                      "--band-edges": a.band_edges is not None}))
        bands = check_band_energies_args(a.band_energies, a.hop if bank is None and stft is None else None, a.band_edges, given_energies)
        row = a.decode or stft is not None                   # the flags that describe a decoded row
        levels = check_levels_args(a.levels, a.levels_window, given)
        if levels is None and (a.src is None or a.dst is None):
            raise ValueError("the following arguments are required: src, dst")
        excerpt = check_excerpt_args(a.start, a.samples, row)
        rate_divisor = check_rate_divisor_args(a.rate_divisor, row or levels is not None)
        mix = check_mix_args(a.mix, row or levels is not None or bands is not None or bank is not None)
        sample_rate = check_sample_rate_args(a.sample_rate, row, a.rate_divisor is not None)
        overlay = check_overlay_args(a.overlay, a.snr_db, a.overlay_start, row)
        band_gains = check_band_gains_db_args(a.band_gains_db, row)
        speed = check_speed_args(a.speed, row)
        ir = check_ir_args(a.ir, row)
        array_ir = check_array_ir_args(a.array_ir, ir, row)
        append = check_append_args(a.append, a.crossfade, a.decode, {
            "--start": a.start is not None, "--samples": a.samples is not None, "--overlay": a.overlay is not None,
            "--band-gains-db": a.band_gains_db is not None, "--speed": a.speed is not None, "--ir": a.ir is not None,
            "--array-ir": a.array_ir is not None, "--stft-energies": a.stft_energies, "--nmr": a.nmr, "--measure": a.measure})
        if levels is not None:
            from .store import check_levels_mix
            check_levels_mix(mix, "--mix")
    except ValueError as e:
        ap.error(str(e))
    if stft is not None:
        try:
            spectrum = decode_pac_file(a.src, a.dst, a.device, excerpt, rate_divisor, mix, sample_rate, overlay, band_gains, speed, ir, stft, array_ir)
        except ValueError as e:
            ap.error(str(e))
        print("%s: %s %s" % (a.dst, " x ".join(str(v) for v in spectrum.shape), spectrum.dtype))
        return
    if bands is not None:
        try:
            band_energies_of_file(a.src, a.dst, bands[0], bands[1], a.device, mix)
        except ValueError as e:
            ap.error(str(e))
        return
    if bank is not None:
        try:
            filterbank_energies_of_file(a.src, a.dst, bank[0], bank[1], a.device, mix)
        except ValueError as e:
            ap.error(str(e))
        return
    if levels is not None:
        try:
            for r in levels_of_files(levels[0], levels[1], a.device, rate_divisor, mix):
                print(json.dumps(r))
        except ValueError as e:
            ap.error(str(e))
        return
    if a.vbr_bytes is not None or a.vbr_bits_per_sample is not None or a.vbr_grid is not None:
        try:
            check_vbr_size_args(a.vbr_bytes, a.vbr_bits_per_sample, a.vbr_grid, a.bits_per_sample, a.target_nmr, a.vbr_nmr, a.dst,
                                a.decode, a.certify, a.measure)
            r = encode_wav_vbr_size(a.src, a.dst, a.vbr_bytes, a.vbr_bits_per_sample, a.vbr_grid, not a.no_huffman, a.device,
                                    exact_spread=a.exact_spread)
        except ValueError as e:
            ap.error(str(e))
        print(json.dumps(dict(file=a.dst, bytes=len(r["data"]), target_bytes=r["target_bytes"], chosen_db=r["chosen_db"],
                              met=r["met"], probes=r["probes"], **_vbr_fields(r))))
        return
    if a.vbr_nmr is not None:
        try:
            check_vbr_args(a.vbr_nmr, a.bits_per_sample, a.target_nmr, a.dst, a.decode, a.certify, a.measure)
            r = encode_wav_vbr_nmr(a.src, a.dst, a.vbr_nmr, not a.no_huffman, a.device, exact_spread=a.exact_spread)
        except ValueError as e:
            ap.error(str(e))
        print(json.dumps(dict(file=a.dst, bytes=len(r["data"]), ceiling_db=float(a.vbr_nmr), **_vbr_fields(r))))
        return
    if a.target_nmr is not None:
        try:
            check_target_args(a.bits_per_sample, a.target_nmr, a.dst, a.decode, a.certify, a.measure)
            r = encode_wav_target_nmr(a.src, a.dst, a.bits_per_sample, a.target_nmr, not a.no_huffman, a.device,
                                      exact_spread=a.exact_spread)
        except ValueError as e:
            ap.error(str(e))
        print(json.dumps(dict(file=a.dst, bytes=len(r["data"]), chosen_bits_per_sample=float(r["rate"]), met=r["met"],
                              target_nmr_total_db=float(a.target_nmr), bits_per_sample=[float(t) for t in r["bits_per_sample"]],
                              **_nmr_fields(r))))
        return
    if a.decode and (a.nmr or a.measure):
        ap.error("-d decodes: --nmr and --measure apply to .pac files coded from src")
    if a.measure:
        rates = None if a.bits_per_sample is None else parse_bits_per_sample(a.bits_per_sample)
        if rates is not None and len(rates) > 1 and "{bps}" not in a.dst:
            ap.error("several bit rates: dst must contain {bps} (e.g. out_{bps}.pac)")
        paths = [a.dst] if rates is None else ladder_paths(a.dst, rates)
        missing = [p for p in paths if not os.path.isfile(p)]
        if missing:
            ap.error("--measure: no such file: %s" % ", ".join(missing))
        _print_nmr(ap, a, paths, None if rates is None else [v for (_, v) in rates])
        return
    if a.decode and append is not None:
        try:
            pcm = decode_appended_files(a.src, a.dst, append, a.device, rate_divisor, mix, sample_rate)
        except ValueError as e:
            ap.error(str(e))
        print("%s: %d channels x %d samples" % (a.dst, pcm.shape[0], pcm.shape[1]))
        return
    if a.decode:
        try:
            pcm = decode_pac_file(a.src, a.dst, a.device, excerpt, rate_divisor, mix, sample_rate, overlay, band_gains, speed, ir, array_ir=array_ir)
        except ValueError as e:
            ap.error(str(e))
        print("%s: %d channels x %d samples" % (a.dst, pcm.shape[0], pcm.shape[1]))
        return
    cert = {} if a.certify else None
    if a.bits_per_sample is not None and len(parse_bits_per_sample(a.bits_per_sample)) > 1:
        rates = parse_bits_per_sample(a.bits_per_sample)
        if cert is not None:
            ap.error("--certify takes one bit rate")
        if "{bps}" not in a.dst:
            ap.error("several bit rates: dst must contain {bps} (e.g. out_{bps}.pac)")
        datas = encode_wav(a.src, a.dst, not a.no_huffman, a.device, exact_spread=a.exact_spread, bits_per_sample=a.bits_per_sample)
        for path, d in zip(ladder_paths(a.dst, rates), datas):
            print("%s: %d bytes" % (path, len(d)))
        if a.nmr:
            _print_nmr(ap, a, ladder_paths(a.dst, rates), [v for (_, v) in rates])
        return
    data = encode_wav(a.src, a.dst, not a.no_huffman, a.device, exact_spread=a.exact_spread, certify=cert,
                      bits_per_sample=a.bits_per_sample)
    print("%s: %d bytes" % (a.dst, len(data)))
    if cert is not None:
        print("certificate: %d blocks examined; decisions within a guard band of rounding: %d (quantiser edges %d, "
              "bit-allocation ties %d, M/S threshold %d, peak test %d); chunks the slope-node evaluation sent back: %d"
              % (cert["blocks_examined"], cert["decisions_near_an_edge"], cert["quantiser_edges"], cert["bitalloc_near_ties"],
                 cert["ms_switch_near_threshold"], cert["peak_near_ties"], cert["node_chunks_sent_back"]))
        if "bytes_equal_exact_spread" in cert:
            print("  re-encoded with --exact-spread: bytes %s" % ("identical" if cert["bytes_equal_exact_spread"] else "DIFFER"))
    if a.nmr:                            # one rate: the one given, else the one a new handle encodes at (pacfileThem.py:1108)
        _print_nmr(ap, a, [a.dst], [2.86 if a.bits_per_sample is None else parse_bits_per_sample(a.bits_per_sample)[0][1]])


if __name__ == "__main__":
    main()
