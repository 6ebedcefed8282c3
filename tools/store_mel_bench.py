"""
Mel spectrograms of crops of a resident corpus on an MI355X, three routes taking turns in one process on the `streams`
workload of tools/store_bench.py built from its seeds (8192 one-second stereo crops of 256 stereo files of 600 hops; 80 HTK
mel filters over 0 - 24 kHz, hop 480, 100 frames):
  (a) PacStore.filterbank_window (mrc_pac_store_filterbank_window: triangular filters on the squared MDCT lines);
  (b) PacStore.band_energy_window with the 81 edges points[1:], 80 rectangular bands -- the same parse and frames, band_energy_kernel
      in filterbank_energy_kernel's place: (a) - (b), stage by stage from PacStore.stats()["ms"], is what the weights cost;
  (c) the route there was without (a): decode_window of the same crops as float32, torch.stft power (1024-point Hann, hop 480)
      and a mel matrix.
After a warm-up call of each route: the median over the timed rounds of the wall seconds of each (each ends in a device
synchronise), the device time of (a) and (b) by stage and their counts, the device time of (c)'s decode_window calls, and how
(a) and (c) compare: the largest and the median difference in dB of a crop's filter totals over its frames (the frame grids
differ by the STFT's centring and its window, so single frames are not compared), and how many values of (a) and (b) are
exactly 0 (no line with a coded mantissa under the filter or in the band).  Profiler off.
  timeout -k 10 900 python tools/store_mel_bench.py --out profiles/store_mel_bench.json
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
from mrcaudiocodec_amd.store import PacStore, mel_points                              # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

N_FFT = 1024
STAGES = {"plan_upload": "plan_upload", "unpack": "unpack", "synthesis": "sums", "window_out": "frame_assembly"}


def mel_matrix(points, rate, dev):
    """[filters][N_FFT / 2 + 1]: the triangle's value at the bin's frequency, times 2 for the bin and its mirror (bins 0 and
    N_FFT / 2: 1)"""
    import torch
    f = np.arange(N_FFT // 2 + 1) * (rate / N_FFT)
    p0, p1, p2 = points[:-2, None], points[1:-1, None], points[2:, None]
    m = np.maximum(0.0, np.minimum((f - p0) / (p1 - p0), (p2 - f) / (p2 - p1))) * 2.0
    m[:, 0] *= 0.5
    m[:, -1] *= 0.5
    return torch.from_numpy(m.astype(np.float32)).to(dev)


def run(h, files, what, crops, window, hop, n_filters, reps, batch):
    import torch
    dev = torch.device("cuda", 0)
    store = PacStore(h, files)
    rate = h.cfg.sample_rate
    points = mel_points(n_filters, 0.0, rate / 2.0)
    edges = points[1:]                                               # n_filters + 1 edges: n_filters rectangular bands
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - window)).astype(np.int64)      # wholly inside their files
    n_frames = -(-window // hop)
    out = torch.empty((crops, 2, n_filters, n_frames), dtype=torch.float32, device=dev)
    out_b = torch.empty((crops, 2, len(edges) - 1, n_frames), dtype=torch.float32, device=dev)
    hann = torch.hann_window(N_FFT, device=dev)
    mm = mel_matrix(points, rate, dev)
    wave = torch.empty((batch, 2, window), dtype=torch.float32, device=dev)

    def mel_call():
        t0 = time.perf_counter()
        store.filterbank_window(which, starts, n_frames, hop, points, channels=2, dtype=torch.float32, out=out)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, store.stats()

    def bands_call():
        t0 = time.perf_counter()
        store.band_energy_window(which, starts, n_frames, hop, edges, channels=2, dtype=torch.float32, out=out_b)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, store.stats()

    def stft_call(keep):
        """-> wall seconds, the device ms of its decode_window calls (PacStore.stats()), the spectrograms
        [crops][2][filters][frames'] if keep"""
        t0, t_dec, parts = time.perf_counter(), 0.0, []
        for i in range(0, crops, batch):
            n = min(batch, crops - i)
            x = store.decode_window(which[i:i + n], starts[i:i + n], window, channels=2, dtype=torch.float32, out=wave[:n])
            t_dec += sum(store.stats()["ms"].values())
            s = torch.stft(x.reshape(2 * n, window), N_FFT, hop_length=hop, window=hann, return_complex=True)
            p = torch.matmul(mm, s.real.square() + s.imag.square())
            if keep:
                parts.append(p.reshape(n, 2, p.shape[1], p.shape[2]))
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t_dec, (torch.cat(parts) if keep else None)

    first = mel_call()[0]
    bands_call()
    _, _, spec = stft_call(True)                                     # warm-up of the other route; kept for the comparison
    t = {"mel": [], "bands": [], "stft": [], "stft_decode": []}
    sts = {"mel": [], "bands": []}
    for _ in range(reps):                                            # the routes take turns
        for name, call in (("mel", mel_call), ("bands", bands_call)):
            dt, st = call()
            t[name].append(dt)
            sts[name].append(st)
        dt, dd, _ = stft_call(False)
        t["stft"].append(dt)
        t["stft_decode"].append(dd)
    # a crop's filter totals: sum over frames against the STFT's power normalised to a signal's sum of squares (sum_k |S_k|^2
    # over the whole spectrum is N_FFT sum_n (w x)^2, a frame stands for hop samples)
    est = out.double().sum(-1)
    ref = spec.double().sum(-1) * (hop / (N_FFT * float((hann.double() ** 2).sum())))
    both = (est > 1e-9) & (ref > 1e-9)
    db = (10 * torch.log10(est[both] / ref[both])).abs()
    med = lambda v: round(float(np.median(v)), 5)
    ms = {r: {STAGES[k]: round(float(np.median([s["ms"][k] for s in sts[r]])), 3) for k in STAGES} for r in sts}
    res = {"workload": what, "files": len(files), "crops": crops, "window": window, "hop": hop, "filters": n_filters,
           "frames": n_frames, "rounds_timed": reps, "stft": {"n_fft": N_FFT, "window": "hann", "crops_per_call": batch},
           "first_call_seconds": round(first, 5),
           "filterbank_seconds_wall": med(t["mel"]), "band_energy_seconds_wall": med(t["bands"]), "stft_route_seconds_wall": med(t["stft"]),
           "stft_route_decode_window_device_ms": round(float(np.median(t["stft_decode"])), 3),
           "filterbank_seconds_all": [round(v, 5) for v in t["mel"]], "band_energy_seconds_all": [round(v, 5) for v in t["bands"]],
           "stft_route_seconds_all": [round(v, 5) for v in t["stft"]],
           "filterbank_device_ms": ms["mel"], "band_energy_device_ms": ms["bands"],
           "weights_cost_device_ms": {k: round(ms["mel"][k] - ms["bands"][k], 3) for k in ms["mel"]},
           "filterbank_device_ms_total": round(sum(ms["mel"].values()), 3), "band_energy_device_ms_total": round(sum(ms["bands"].values()), 3),
           "filterbank_stats": {k: v for k, v in sts["mel"][-1].items() if k != "ms"},
           "band_energy_stats": {k: v for k, v in sts["bands"][-1].items() if k != "ms"},
           "stft_over_filterbank_wall": round(med(t["stft"]) / med(t["mel"]), 2),
           "filterbank_zero_values": int((out == 0).sum()), "band_energy_zero_values": int((out_b == 0).sum()), "values": out.numel(),
           "crop_filter_totals_db_difference": {"median": round(float(db.median()), 3), "max": round(float(db.max()), 3),
                                                "compared": int(both.sum())}}
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--window", type=int, default=48000)
    ap.add_argument("--hop", type=int, default=480)
    ap.add_argument("--filters", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024, help="crops per decode_window + torch.stft call of the baseline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    res = run(h, files, what, a.crops, a.window, a.hop, a.filters, a.reps, a.batch)
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/store_mel_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res},
                      f, indent=1)


if __name__ == "__main__":
    main()
