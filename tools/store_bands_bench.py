"""
Band-energy spectrograms of crops of a resident corpus on an MI355X: PacStore.band_energy_window
(mrc_pac_store_band_energy_window: each block's sum of squares per band, laid on a frame grid; no inverse transform)
against the route there was without it -- decode_window of the same crops as float32, torch.stft power (2048-point Hann,
hop 512) and a band matrix -- in one process, the two routes taking turns, on the `streams` workload of
tools/store_bench.py built from its seeds: 8192 one-second stereo crops of 256 stereo files of 600 hops, the critical bands,
hop 512.  After a warm-up call of each route: the median over the timed calls of the wall seconds of both (each ends in a
device synchronise), the device time of the band-energy call by stage (plan_upload, unpack, band sums, frame assembly:
PacStore.stats()) and its counts, the device time of the baseline's decode_window calls, and how the two spectrograms compare: the largest
and the median difference in dB of a crop's band totals over its frames (the frame grids differ by the STFT's centring and
its window, so single frames are not compared).  Profiler off.
  timeout -k 10 900 python tools/store_bands_bench.py --out profiles/store_bands_bench.json
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
from mrcaudiocodec_amd.store import PacStore, critical_band_edges                     # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

N_FFT = 2048
MS_NAMES = {"plan_upload": "plan_upload", "unpack": "unpack", "synthesis": "band_sums", "window_out": "frame_assembly"}


def band_matrix(edges, rate, dev):
    """[bands][N_FFT / 2 + 1]: where the bin's frequency lies in the band 2, the bin and its mirror (bins 0 and N_FFT / 2: 1)"""
    import torch
    f = np.arange(N_FFT // 2 + 1) * (rate / N_FFT)
    m = np.array([(f >= lo) & (f < hi) for lo, hi in zip(edges[:-1], edges[1:])], dtype=np.float32) * 2.0
    m[:, 0] *= 0.5
    m[:, -1] *= 0.5
    return torch.from_numpy(m).to(dev)


def run(h, files, what, crops, window, hop, reps, batch):
    import torch
    dev = torch.device("cuda", 0)
    store = PacStore(h, files)
    rate = h.cfg.sample_rate
    edges = critical_band_edges(rate)
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - window)).astype(np.int64)      # wholly inside their files
    n_frames = -(-window // hop)
    out = torch.empty((crops, 2, len(edges) - 1, n_frames), dtype=torch.float32, device=dev)
    hann = torch.hann_window(N_FFT, device=dev)
    bm = band_matrix(edges, rate, dev)
    wave = torch.empty((batch, 2, window), dtype=torch.float32, device=dev)

    def bands_call():
        t0 = time.perf_counter()
        store.band_energy_window(which, starts, n_frames, hop, edges, channels=2, dtype=torch.float32, out=out)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, store.stats()

    def stft_call(keep):
        """-> wall seconds, the device ms of its decode_window calls (PacStore.stats(): a host clock around a call would
        count the STFT queued before it), the spectrograms [crops][2][bands][frames'] if keep"""
        t0, t_dec, parts = time.perf_counter(), 0.0, []
        for i in range(0, crops, batch):
            n = min(batch, crops - i)
            x = store.decode_window(which[i:i + n], starts[i:i + n], window, channels=2, dtype=torch.float32, out=wave[:n])
            t_dec += sum(store.stats()["ms"].values())
            s = torch.stft(x.reshape(2 * n, window), N_FFT, hop_length=hop, window=hann, return_complex=True)
            p = torch.matmul(bm, s.real.square() + s.imag.square())
            if keep:
                parts.append(p.reshape(n, 2, p.shape[1], p.shape[2]))
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t_dec, (torch.cat(parts) if keep else None)

    first = bands_call()[0]
    _, _, spec = stft_call(True)                                     # warm-up of the other route; kept for the comparison
    t = {"bands": [], "stft": [], "stft_decode": []}
    sts = []
    for _ in range(reps):                                            # the routes take turns
        dt, st = bands_call()
        t["bands"].append(dt)
        sts.append(st)
        dt, dd, _ = stft_call(False)
        t["stft"].append(dt)
        t["stft_decode"].append(dd)
    # a crop's band totals: sum over frames of the band energies against the STFT's power, normalised to a signal's sum of
    # squares: sum_k |S_k|^2 over the whole spectrum is N_FFT sum_n (w x)^2, a frame stands for hop samples, and the band
    # matrix counts the one-sided bins with weight 2 (bins 0 and N_FFT / 2: 1)
    est = out.double().sum(-1)
    ref = spec.double().sum(-1) * (hop / (N_FFT * float((hann.double() ** 2).sum())))
    both = (est > 1e-9) & (ref > 1e-9)
    db = (10 * torch.log10(est[both] / ref[both])).abs()
    med = lambda v: round(float(np.median(v)), 5)
    ms = {MS_NAMES[k]: round(float(np.median([s["ms"][k] for s in sts])), 3) for k in MS_NAMES}
    res = {"workload": what, "files": len(files), "crops": crops, "window": window, "hop": hop, "bands": len(edges) - 1,
           "frames": n_frames, "calls_timed": reps, "stft": {"n_fft": N_FFT, "window": "hann", "crops_per_call": batch},
           "first_call_seconds": round(first, 5), "band_energy_seconds_wall": med(t["bands"]), "stft_route_seconds_wall": med(t["stft"]),
           "stft_route_decode_window_device_ms": round(float(np.median(t["stft_decode"])), 3),
           "band_energy_seconds_all": [round(v, 5) for v in t["bands"]], "stft_route_seconds_all": [round(v, 5) for v in t["stft"]],
           "device_ms": ms, "device_ms_total": round(sum(ms.values()), 3), "stats": {k: v for k, v in sts[-1].items() if k != "ms"},
           "stft_over_band_energy_wall": round(med(t["stft"]) / med(t["bands"]), 2),
           "crop_band_totals_db_difference": {"median": round(float(db.median()), 3), "max": round(float(db.max()), 3),
                                              "compared": int(both.sum())}}
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--window", type=int, default=48000)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="crops per decode_window + torch.stft call of the baseline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    res = run(h, files, what, a.crops, a.window, a.hop, a.reps, a.batch)
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/store_bands_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res},
                      f, indent=1)


if __name__ == "__main__":
    main()
