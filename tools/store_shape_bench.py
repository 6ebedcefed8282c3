"""
Crops of resident 48 kHz `.pac` files with a spectrum of their own as float32 tensors on an MI355X, on the `streams` corpus of
tools/store_reduced_bench.py (256 stereo streams of 600 hops): every item is a one-second crop under a random row of 25 band
gains (the codec's critical bands, store.critical_band_edges).  Three routes take turns in one process, call after call, so
that none has the device to itself at another moment than the others:
  shaped  PacStore.decode_window(band_gains=): mrc_pac_store_decode_window_shaped, one multiplication per MDCT line between the
          dequantiser and the inverse transform
  plain   the same call without band_gains: what the synthesis costs without the gains
  stft    what a user did before the call existed: the plain float32 call, torch.stft (n_fft 2048, hop 512, Hann), a per-item
          gain per bin (the bin's band by its centre frequency), torch.istft
Cases: `full_stereo` -- one second at full rate, both channels; `16k_mid` -- one second at 16 kHz (rate_divisor=2,
resample=(2, 3), mix="mid"; the bins' bands are then those of the 16 kHz signal).  All routes allocate their tensors inside the
timed call.  After a warm-up round, per route the median over the timed rounds of the wall seconds, the interquartile range of
those rounds, the device time of the store's stages (PacStore.stats(): plan_upload, unpack, synthesis, window_out; the stft
route has its torch part alone, by events) and the peak of torch.cuda.max_memory_allocated.  The shaped synthesis stage over
the plain one of the same run is recorded with both spreads beside it.  Nothing here decides a ratio in advance: the JSON
holds what was measured.
Deviation: per-line gains on a lapped transform are not an LTI filter -- where neighbouring lines get different gains the
time-domain aliasing of adjacent blocks no longer cancels exactly.  For 64 full-rate stereo crops, under (a) a smooth tilt of
+3 to -9 dB over the 25 bands and (b) a brick-wall low-pass (bands above 3700 Hz at 0), the shaped window minus the stft
route's window is analysed by the same STFT, and per band q the energy of that difference over the energy the UNSHAPED crop
holds in band q is recorded in dB: the median and the maximum over items and channels, per band, and over all bands.
  timeout -k 10 900 python tools/store_shape_bench.py --out profiles/store_shape_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mrcaudiocodec_amd import Handle                                                  # noqa: E402
from mrcaudiocodec_amd.store import MS_NAMES, PacStore, critical_band_edges, gains_from_db   # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

N_FFT, HOP = 2048, 512
CASES = {
    "full_stereo": dict(window=48000, channels=2, rate=48000, kw=dict(channels=2)),
    "16k_mid": dict(window=16000, channels=1, rate=16000, kw=dict(rate_divisor=2, resample=(2, 3), mix="mid")),
}


def bin_bands(edges, rate):
    """the band of every STFT bin by its centre frequency (-1: in no band)"""
    f = np.arange(N_FFT // 2 + 1) * (rate / N_FFT)
    band = np.full(f.size, -1, np.int64)
    for q in range(edges.size - 1):
        band[(edges[q] <= f) & (f < edges[q + 1])] = q
    return band


def stft_route(x, bin_gain, window_fn):
    """x float32 [n][c][t], bin_gain float32 [n][bins] -> the filtered signal, same shape"""
    import torch
    n, c, t = x.shape
    X = torch.stft(x.reshape(n * c, t), N_FFT, HOP, window=window_fn, return_complex=True)
    X = X.reshape(n, c, X.shape[1], X.shape[2]) * bin_gain[:, None, :, None]
    return torch.istft(X.reshape(n * c, X.shape[2], X.shape[3]), N_FFT, HOP, window=window_fn, length=t).reshape(n, c, t)


def run_case(store, name, case, crops, reps):
    import torch
    dev = torch.device("cuda", 0)
    window, kw = case["window"], case["kw"]
    rng = np.random.default_rng(29)
    edges = critical_band_edges(48000)
    nb = edges.size - 1
    files = rng.integers(0, len(store), crops)
    scale = window / 48000.0
    starts = (rng.random(crops) * (store.n_samples[files] * scale - window)).astype(np.int64)
    rows = gains_from_db(rng.uniform(-12.0, 6.0, (crops, nb)))
    band = bin_bands(edges, case["rate"])
    bin_gain = np.where(band >= 0, rows[:, np.maximum(band, 0)], 1.0).astype(np.float32)
    bin_gain_dev = torch.from_numpy(bin_gain).to(dev)
    hann = torch.hann_window(N_FFT, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def route_shaped():
        store.decode_window(files, starts, window, dtype=torch.float32, band_gains=rows, **kw)
        return store.stats(), None

    def route_plain():
        store.decode_window(files, starts, window, dtype=torch.float32, **kw)
        return store.stats(), None

    def route_stft():
        x = store.decode_window(files, starts, window, dtype=torch.float32, **kw)
        st = store.stats()
        ev0.record()
        stft_route(x, bin_gain_dev, hann)
        ev1.record()
        torch.cuda.synchronize(dev)
        return st, ev0.elapsed_time(ev1)

    routes = (("shaped", route_shaped), ("plain", route_plain), ("stft", route_stft))
    for _, fn in routes:                                         # warm-up round: workspaces, the filter's upload, torch's kernels
        fn()
    wall, sts, peak, torch_ms = ({r: [] for r, _ in routes} for _ in range(4))
    for _ in range(reps):
        for r, fn in routes:
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            st, ms = fn()
            wall[r].append(time.perf_counter() - t0)
            peak[r].append(torch.cuda.max_memory_allocated(dev) - base)
            sts[r].append(st)
            if ms is not None:
                torch_ms[r].append(ms)
    iqr = lambda v: float(np.subtract(*np.percentile(v, [75, 25])))
    res = {"items": crops, "window": window, "bands": nb, "out_shape": [crops, case["channels"], window],
           "arguments": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "rounds_timed": reps, "routes": {}}
    for r, _ in routes:
        ms = {k: round(float(np.median([s["ms"][k] for s in sts[r]])), 3) for k in MS_NAMES}
        res["routes"][r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_wall_interquartile": round(iqr(wall[r]), 5),
                            "seconds_all": [round(v, 5) for v in wall[r]], "device_ms": ms,
                            "synthesis_ms_interquartile": round(iqr([s["ms"]["synthesis"] for s in sts[r]]), 3),
                            "device_ms_total": round(sum(ms.values()), 3), "peak_torch_bytes": int(np.median(peak[r])),
                            "stats": {k: v for k, v in sts[r][-1].items() if k != "ms"}}
    t = res["routes"]["stft"]
    t["torch_device_ms"] = round(float(np.median(torch_ms["stft"])), 3)
    t["torch_device_ms_interquartile"] = round(iqr(torch_ms["stft"]), 3)
    t["device_ms_total"] = round(t["device_ms_total"] + t["torch_device_ms"], 3)
    sh, pl = res["routes"]["shaped"], res["routes"]["plain"]
    res["shaped_synthesis_over_plain_synthesis"] = round(sh["device_ms"]["synthesis"] / pl["device_ms"]["synthesis"], 4)
    res["shaped_wall_over_plain_wall"] = round(sh["seconds_wall"] / pl["seconds_wall"], 4)
    res["stft_wall_over_shaped_wall"] = round(t["seconds_wall"] / sh["seconds_wall"], 3)
    print("%s: shaped %.5f s (synthesis %.3f ms), plain %.5f s (synthesis %.3f ms), stft %.5f s; peak %d / %d / %d MiB" % (
        name, sh["seconds_wall"], sh["device_ms"]["synthesis"], pl["seconds_wall"], pl["device_ms"]["synthesis"], t["seconds_wall"],
        sh["peak_torch_bytes"] >> 20, pl["peak_torch_bytes"] >> 20, t["peak_torch_bytes"] >> 20), flush=True)
    return res


def deviation(store, n=64):
    """the shaped windows against the stft route's, per band, for a smooth tilt and a brick-wall low-pass (see the module's
    docstring)"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    edges = critical_band_edges(48000)
    nb, window = edges.size - 1, 48000
    files = rng.integers(0, len(store), n)
    starts = (rng.random(n) * (store.n_samples[files] - window)).astype(np.int64)
    band = bin_bands(edges, 48000)
    hann = torch.hann_window(N_FFT, device=dev)
    onehot = torch.from_numpy((band[None, :] == np.arange(nb)[:, None]).astype(np.float64)).to(dev)       # [bands][bins]

    def band_energy(x):                                          # float64 [n][c][t] -> [n][c][bands]
        X = torch.stft(x.reshape(-1, x.shape[-1]), N_FFT, HOP, window=hann.double(), return_complex=True)
        p = (X.real ** 2 + X.imag ** 2).sum(dim=2)               # [n c][bins]
        return (p @ onehot.T).reshape(x.shape[0], x.shape[1], nb)

    plain = store.decode_window(files, starts, window, channels=2, dtype=torch.float64)
    e_in = band_energy(plain)
    out = {"items": n, "window": window, "n_fft": N_FFT, "hop": HOP,
           "definition": "10 log10(E_q(shaped - stft) / E_q(unshaped crop)), E_q the STFT energy of band q; over items and channels"}
    curves = {"smooth_tilt_+3_to_-9_dB": gains_from_db(np.linspace(3.0, -9.0, nb)),
              "brick_wall_low_pass_3700_Hz": (edges[1:] <= 3700.0).astype(np.float64)}
    for name, row in curves.items():
        shaped = store.decode_window(files, starts, window, channels=2, dtype=torch.float64, band_gains=row)
        bin_gain = torch.from_numpy(np.where(band >= 0, row[np.maximum(band, 0)], 1.0)).to(dev)
        ref = stft_route(plain, bin_gain[None, :].expand(n, -1), hann.double())
        d = 10.0 * torch.log10(band_energy(shaped - ref) / e_in)                         # [n][c][bands]
        d = d.reshape(-1, nb).cpu().numpy()
        whole = 10.0 * torch.log10(((shaped - ref) ** 2).sum(dim=2) / (plain ** 2).sum(dim=2)).reshape(-1).cpu().numpy()
        out[name] = {"gains": [round(float(v), 6) for v in row],
                     "per_band_median_db": [round(float(v), 2) for v in np.median(d, axis=0)],
                     "per_band_max_db": [round(float(v), 2) for v in d.max(axis=0)],
                     "all_bands_median_db": round(float(np.median(d)), 2), "all_bands_max_db": round(float(d.max()), 2),
                     "whole_signal_median_db": round(float(np.median(whole)), 2), "whole_signal_max_db": round(float(whole.max()), 2)}
        print("%s: difference over the unshaped crop, per band: median %.1f dB, max %.1f dB; whole signal: median %.1f dB" % (
            name, out[name]["all_bands_median_db"], out[name]["all_bands_max_db"], out[name]["whole_signal_median_db"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = a.cases.split(",")
    if a.reps < 1 or a.streams < 1 or any(n not in CASES for n in names):
        ap.error("--reps and --streams at least 1, --cases among %s" % ",".join(CASES))
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "cases": {n: run_case(store, n, CASES[n], a.crops, a.reps) for n in names},
           "deviation_from_the_stft_route": deviation(store)}
    store.close()
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        out = {"tool": "tools/store_shape_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
