"""
Random one-second crops of resident `.pac` files at the full, half and quarter sample rate, as float32 tensors on an MI355X:
PacStore.decode_window(rate_divisor=D) for D = 1, 2 and 4 in one process on the two workloads of tools/store_bench.py
  streams  256 stereo streams of 600 hops (synth.c3_stereo), encoded by the chained stream-mode call
  single   the 65 536-hop stereo stream of tools/single_stream_bench.py (bursts every 37 hops)
with the same 8192 crops for every D: window = 48000 / D reduced samples, start = the full-rate start / D (the full-rate
starts are multiples of 4, so that every D reads the same second).
Per D, after a warm-up call, the median over the timed calls of: the wall seconds of the call and the device time of its
stages (plan_upload, unpack, synthesis, window_out: PacStore.stats()), and the call's counts.
For comparison, what a user did before the reduced call existed: the D = 1 call followed by a strided FIR decimation on the
device in torch (conv1d with a Kaiser-windowed sinc of 32 D taps, cut-off at the new Nyquist frequency, stride D), timed in
the same run: wall seconds of both steps together, and the device time of the conv1d alone (events).  How far the two
results agree on 64 crops is recorded too (SNR of the reduced decode against the FIR route, informative: the two cut the
band differently next to the cut-off).
One workload per process, each under its own time limit, the second only if the first ended well:
  timeout -k 10 900 python tools/store_reduced_bench.py --workload streams --out profiles/store_reduced_bench.json && \\
  timeout -k 10 900 python tools/store_reduced_bench.py --workload single --out profiles/store_reduced_bench.json
(a run adds its workload to the file and keeps the other's).
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
from mrcaudiocodec_amd.store import MS_NAMES, PacStore                                # noqa: E402
from decode_bench import single_stream_file                                           # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

TAPS_PER_D = 32


def fir(D, dev):
    """Kaiser-windowed sinc, 32 D taps, cut-off at 1 / (2 D) of the sample rate, unit gain at 0 Hz; with padding
    (taps - D) / 2 and stride D its output m sits at the full-rate time D m + (D - 1) / 2, as the reduced decode's does"""
    import torch
    T = TAPS_PER_D * D
    j = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(j / D) / D * np.kaiser(T, 8.0)
    return torch.from_numpy((h / h.sum()).astype(np.float32)).to(dev).view(1, 1, T), (T - D) // 2


def median_call(fn, reps):
    """a warm-up, then reps timed calls -> (median wall seconds, all of them, [stats of each call])"""
    fn()
    ts, sts = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        sts.append(fn())
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, sts


def run(h, files, what, crops, window, reps):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    store = PacStore(h, files)
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - window)).astype(np.int64) // 4 * 4   # wholly inside their files
    res = {"workload": what, "files": len(files), "crops": crops, "window_full_rate": window, "calls_timed": reps,
           "rate_divisor": {}}
    outs = {}
    for D in (1, 2, 4):
        out = torch.empty((crops, 2, window // D), dtype=torch.float32, device=dev)
        outs[D] = out

        def call(D=D, out=out):
            store.decode_window(which, starts // D, window // D, channels=2, dtype=torch.float32, out=out, rate_divisor=D)
            return store.stats()
        t, ts, sts = median_call(call, reps)
        ms = {k: round(float(np.median([s["ms"][k] for s in sts])), 3) for k in MS_NAMES}
        res["rate_divisor"][str(D)] = {"window": window // D, "seconds_wall": round(t, 5), "seconds_all": [round(v, 5) for v in ts],
                                       "device_ms": ms, "device_ms_total": round(sum(ms.values()), 3),
                                       "out_bytes": out.numel() * 4,
                                       "stats": {k: v for k, v in sts[-1].items() if k != "ms"}}
    base = res["rate_divisor"]["1"]
    for D in (2, 4):
        r = res["rate_divisor"][str(D)]
        r["speedup_wall_vs_full_rate"] = round(base["seconds_wall"] / r["seconds_wall"], 3)
        r["dominant_stage"] = max(r["device_ms"], key=r["device_ms"].get)
        taps, pad = fir(D, dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        conv_ms = []

        def today(D=D, taps=taps, pad=pad):
            store.decode_window(which, starts, window, channels=2, dtype=torch.float32, out=outs[1])
            ev0.record()
            y = F.conv1d(outs[1].view(crops * 2, 1, window), taps, stride=D, padding=pad)
            ev1.record()
            torch.cuda.synchronize(dev)
            conv_ms.append(ev0.elapsed_time(ev1))
            return y
        try:
            today()                                               # warm-up: conv1d picks its kernel
            conv_ms.clear()
            ts, y = [], None
            for _ in range(reps):
                t0 = time.perf_counter()
                y = today()
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            a, b = outs[D][:64, :, 64:-64].double(), y.view(crops, 2, -1)[:64, :, 64:-64].double()
            snr = float(10 * torch.log10((b * b).sum() / ((a - b) ** 2).sum()))
            r["full_rate_then_fir"] = {"taps": TAPS_PER_D * D, "seconds_wall": round(t, 5), "seconds_all": [round(v, 5) for v in ts],
                                       "conv1d_device_ms": round(float(np.median(conv_ms)), 3),
                                       "snr_db_reduced_vs_fir_64_crops": round(snr, 2)}
            r["speedup_wall_vs_full_rate_then_fir"] = round(t / r["seconds_wall"], 3)
            del y
        except RuntimeError as e:                                 # (no convolution kernel for the shape: say so, keep the rest)
            r["full_rate_then_fir"] = {"error": str(e)[:300]}
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="streams", choices=("streams", "single"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--period", type=int, default=37)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--window", type=int, default=48000, help="at the full rate; a multiple of 4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.window % 4 or a.reps < 1:
        ap.error("--window must be a multiple of 4 and --reps at least 1")
    h = Handle(device_id=0)
    if a.workload == "streams":
        files, what = synth_stream_files(h, a.streams, a.stream_hops)
    else:
        files, what = single_stream_file(h, a.hops, a.period)
    res = run(h, files, what, a.crops, a.window, a.reps)
    h.close()
    print(json.dumps({a.workload: res}), flush=True)
    if a.out:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out["tool"] = "tools/store_reduced_bench.py"
        out.setdefault("args", {})[a.workload] = {k: v for k, v in vars(a).items() if k != "out"}
        out[a.workload] = res
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
