"""
STFT mel spectrograms of crops of a resident corpus on an MI355X, the routes taking turns in one process on the `streams`
workload of tools/store_bench.py built from its seeds (8192 one-second items of 256 stereo files of 600 hops), three workloads:
  mid16k      16 kHz mid (rate_divisor=2, resample=(2, 3)), n_fft 400, hop 160, 80 mel filters over 0 - 8 kHz, 98 frames;
  mixture16k  the same as rows of two terms: speech through a room of the store's bank over dry noise at gain 0.25;
  stereo48k   48 kHz stereo, n_fft 1024, hop 480, 80 mel filters over 0 - 24 kHz, 98 frames;
and three routes:
  (a) the one call, PacStore.stft_window(output="bank") (mrc_pac_store_stft_window), float32 out;
  (b) the route there was without it: decode_window / decode_window_sum of the same rows as float32, torch.stft power
      (center=False, the same window) and the same mel matrix as a float32 matmul, --batch items per call;
  (c) PacStore.filterbank_window, the line-based call, where it applies (stereo48k: full rate, hop 480, 100 frames).
After a warm-up of each route: the median and the interquartile range over the timed rounds of the wall seconds of each (each
ends in a device synchronise); the device time of (a) by stage with stft_kernel's share (mrc_pac_store_stft_ms) and of (b)'s
decode calls; the peak of torch's allocator in a round of each route and the device memory the process holds outside it (the
library's scratch: hipMemGetInfo against torch's reserve); and how far (a)'s float32 values lie from (b)'s on the first 64
items.  Profiler off.
  timeout -k 10 900 python tools/store_stft_bench.py --out profiles/store_stft_bench.json
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
from mrcaudiocodec_amd.store import PacStore, hann_window, mel_bin_weights, mel_points   # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

WORKLOADS = {
    "mid16k": dict(rate=16000, n_fft=400, hop=160, rows=dict(rate_divisor=2, mix="mid", resample=(2, 3)), channels=1, terms=1),
    "mixture16k": dict(rate=16000, n_fft=400, hop=160, rows=dict(rate_divisor=2, mix="mid", resample=(2, 3)), channels=1, terms=2),
    "stereo48k": dict(rate=48000, n_fft=1024, hop=480, rows=dict(), channels=2, terms=1),
}


def room(taps, seed):
    """an exponentially decaying noise tail behind a direct path, T60 = the length"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(taps) * 10.0 ** (-3.0 * np.arange(taps) / taps) * 0.05
    h[0] = 1.0
    return h


def quartiles(v):
    q1, q2, q3 = np.percentile(v, [25, 50, 75])
    return {"median": round(float(q2), 5), "iqr": round(float(q3 - q1), 5)}


def run(h, store, name, w, crops, seconds, n_filters, reps, batch):
    import torch
    dev = torch.device("cuda", 0)
    rate, n_fft, hop, channels = w["rate"], w["n_fft"], w["hop"], w["channels"]
    samples = int(rate * seconds)
    n_frames = (samples - n_fft) // hop + 1
    L = (n_frames - 1) * hop + n_fft
    n_files = len(store)
    rng = np.random.default_rng(17)
    inside = store.n_samples if rate == h.cfg.sample_rate else store.n_samples_resampled(2, 3, 2)
    which = rng.integers(0, n_files, (crops, w["terms"]))
    starts = (rng.random((crops, w["terms"])) * (inside[which] - L)).astype(np.int64)
    rows = dict(w["rows"])
    gains = np.ones((crops, w["terms"]))
    if w["terms"] == 2:
        gains[:, 1] = 0.25
        rows["ir_index"] = np.stack([rng.integers(0, len(store.impulse_response_lengths), crops), np.full(crops, -1)], 1)
    bank = mel_bin_weights(n_fft, rate, mel_points(n_filters, 0.0, rate / 2.0))
    window = hann_window(n_fft)
    out = torch.empty((crops, channels, n_filters, n_frames), dtype=torch.float32, device=dev)
    mm = torch.from_numpy(bank.astype(np.float32)).to(dev)
    hann = torch.from_numpy(window.astype(np.float32)).to(dev)
    wave = torch.empty((batch, channels, L), dtype=torch.float32, device=dev)
    sub = lambda a, i, n: {k: (v[i:i + n] if isinstance(v, np.ndarray) else v) for k, v in a.items()}

    def one_call():
        t0 = time.perf_counter()
        store.stft_window(which, starts, n_frames, hop, n_fft, frame_window=window, bank=bank, output="bank", gains=gains, channels=channels,
                          dtype=torch.float32, out=out, **rows)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, store.stats(), store.stft_ms()

    def torch_route(keep):
        t0, t_dec, parts = time.perf_counter(), 0.0, []
        for i in range(0, crops, batch):
            n = min(batch, crops - i)
            x = store.decode_window_sum(which[i:i + n], starts[i:i + n], gains[i:i + n], L, channels=channels, dtype=torch.float32,
                                        out=wave[:n], **sub(rows, i, n))
            t_dec += sum(store.stats()["ms"].values())
            s = torch.stft(x.reshape(channels * n, L), n_fft, hop_length=hop, window=hann, center=False, return_complex=True)
            p = torch.matmul(mm, s.real.square() + s.imag.square())
            if keep:
                parts.append(p.reshape(n, channels, p.shape[1], p.shape[2]))
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, t_dec, (torch.cat(parts) if keep else None)

    lines = None
    if name == "stereo48k":
        points = mel_points(n_filters, 0.0, rate / 2.0)
        out_l = torch.empty((crops, 2, n_filters, -(-samples // hop)), dtype=torch.float32, device=dev)

        def lines():
            t0 = time.perf_counter()
            store.filterbank_window(which[:, 0], starts[:, 0], out_l.shape[3], hop, points, channels=2, dtype=torch.float32, out=out_l)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t0

    def peak(call):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        call()
        return int(torch.cuda.max_memory_allocated(dev) - base)

    first = one_call()[0]
    _, _, spec = torch_route(True)                                   # warm-up of the other route; 64 items kept for the comparison
    spec = spec[:64].double()
    if lines:
        lines()
    t = {"one_call": [], "torch_route": [], "torch_route_decode": [], "filterbank_window": []}
    sts, kernel = [], []
    for _ in range(reps):                                            # the routes take turns
        dt, st, km = one_call()
        t["one_call"].append(dt)
        sts.append(st)
        kernel.append(km)
        dt, dd, _ = torch_route(False)
        t["torch_route"].append(dt)
        t["torch_route_decode"].append(dd)
        if lines:
            t["filterbank_window"].append(lines())
    free, total = torch.cuda.mem_get_info(dev)
    outside = int(total - free - torch.cuda.memory_reserved(dev))
    est = out[:64].double()
    scale = spec.amax(dim=(2, 3), keepdim=True).clamp_min(1e-30)
    rel = ((est - spec).abs() / scale).amax(dim=(1, 2, 3))
    ms = {k: round(float(np.median([s["ms"][k] for s in sts])), 3) for k in sts[0]["ms"]}
    res = {"workload": name, "items": crops, "terms_per_item": w["terms"], "rate": rate, "n_fft": n_fft, "hop": hop, "frames": n_frames,
           "filters": n_filters, "channels": channels, "rounds_timed": reps, "torch_route_items_per_call": batch,
           "first_call_seconds": round(first, 5),
           "one_call_seconds_wall": quartiles(t["one_call"]), "torch_route_seconds_wall": quartiles(t["torch_route"]),
           "torch_route_over_one_call_wall": round(float(np.median(t["torch_route"]) / np.median(t["one_call"])), 2),
           "one_call_device_ms": ms, "one_call_device_ms_total": round(sum(ms.values()), 3),
           "stft_kernel_ms": round(float(np.median(kernel)), 3),
           "stft_kernel_share_of_device": round(float(np.median(kernel)) / max(sum(ms.values()), 1e-9), 3),
           "torch_route_decode_device_ms": round(float(np.median(t["torch_route_decode"])), 3),
           "one_call_stats": {k: v for k, v in sts[-1].items() if k != "ms"},
           "one_call_torch_peak_bytes": peak(one_call), "torch_route_torch_peak_bytes": peak(lambda: torch_route(False)),
           "output_bytes": out.numel() * 4, "torch_route_waveform_bytes": wave.numel() * 4,
           "device_bytes_outside_torch": outside,
           "float32_difference_on_64_items": {"relative_to_item_peak_max": float(rel.max()), "relative_to_item_peak_median": float(rel.median())}}
    if lines:
        res["filterbank_window_seconds_wall"] = quartiles(t["filterbank_window"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--filters", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024, help="items per decode + torch.stft call of the torch route")
    ap.add_argument("--room-taps", type=int, default=4000, help="taps of the four rooms of the mixture workload, at 16 kHz")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    store.set_impulse_responses([room(a.room_taps, s) for s in range(4)])
    res = {"corpus": what}
    for name in a.workloads.split(","):
        res[name] = run(h, store, name, WORKLOADS[name], a.crops, a.seconds, a.filters, a.reps, a.batch)
        print(json.dumps(res[name]), flush=True)
    store.close()
    h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/store_stft_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "results": res},
                      f, indent=1)


if __name__ == "__main__":
    main()
