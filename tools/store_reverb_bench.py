"""
Reverberation of crops of resident 48 kHz `.pac` files as float32 tensors on an MI355X, on the `streams` corpus of
tools/store_reduced_bench.py (256 stereo streams of 600 hops): 8192 one-second items, every convolved term with one of 256
synthetic room impulse responses (exponentially decaying noise, 0.5 s at the output rate), drawn per item.  Three routes take
turns in one process, call after call:
  reverb  PacStore.decode_window(ir_index=) (decode_window_sum for the mixture): mrc_pac_store_decode_window_reverb, one call
  torch   what a user did before the call existed: PacStore.decode_window float32 of every convolved term WITH its pre-roll
          (start - (taps - 1), window + taps - 1), torch.fft.rfft of it and of the item's response at the next power of two, the
          product, irfft, the slice of the last `window` samples, and for the mixture a + g * b with b one more decode_window
  dry     the reverb call with every ir_index = -1 (the speeds path, unchanged): the cost of the stage by difference
Cases: `16k_mid` -- one term at 16 kHz (rate_divisor=2, resample=(2, 3), mix="mid"); `16k_mid_mixture` -- speech through a room
over dry noise at a drawn gain; `full_stereo` -- one term at full rate, both channels.  After a warm-up round, per route the
median over the timed rounds of the wall seconds, their interquartile spread, the device time per stage (PacStore.stats() and
reverb_ms(); the torch route's FFT expression by events read after its one final synchronisation) and the peak of
torch.cuda.max_memory_allocated.  Nothing here decides a ratio in advance: the JSON holds what was measured.
  timeout -k 10 1100 python tools/store_reverb_bench.py --out profiles/store_reverb_bench.json
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
from mrcaudiocodec_amd.store import MS_NAMES, REVERB_BLOCK, PacStore                  # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

CASES = {
    "16k_mid": dict(K=1, window=16000, rate=16000, channels=1, D=2, resample=(2, 3), kw=dict(rate_divisor=2, mix="mid")),
    "16k_mid_mixture": dict(K=2, window=16000, rate=16000, channels=1, D=2, resample=(2, 3), kw=dict(rate_divisor=2, mix="mid")),
    "full_stereo": dict(K=1, window=48000, rate=48000, channels=2, D=1, resample=None, kw=dict(channels=2)),
}


def synth_rirs(n, taps, seed=3):
    """n room responses of `taps` taps: the direct path 1.0, then noise decaying by 60 dB over the response"""
    rng = np.random.default_rng(seed)
    env = 10.0 ** (-3.0 * np.arange(taps) / taps)
    h = rng.standard_normal((n, taps)) * env * 0.1
    h[:, 0] = 1.0
    return h


def run_case(store, name, case, crops, reps, n_irs):
    import torch
    dev = torch.device("cuda", 0)
    K, window, kw, D = case["K"], case["window"], case["kw"], case["D"]
    taps = case["rate"] // 2
    bank = synth_rirs(n_irs, taps)
    store.set_impulse_responses(list(bank))
    rng = np.random.default_rng(31)
    n_files = len(store)
    speech = rng.integers(0, n_files, crops)
    noise = (speech + 1 + rng.integers(0, n_files - 1, crops)) % n_files
    ratio = case["resample"] or (1, 1)
    inside = lambda f: np.asarray(store.n_samples_resampled(*ratio, D), np.int64)[f]
    s_starts = taps + (rng.random(crops) * (inside(speech) - window - taps)).astype(np.int64)      # the pre-roll inside the file too
    n_starts = (rng.random(crops) * (inside(noise) - window)).astype(np.int64)
    gains = 10.0 ** (rng.uniform(-20.0, 0.0, crops) / 20.0)
    g_dev = torch.from_numpy(gains.astype(np.float32)).to(dev)
    irs = rng.integers(0, n_irs, crops)
    irs_dev = torch.from_numpy(irs).to(dev)
    n_fft = 1 << int(np.ceil(np.log2(window + taps - 1)))       # (what wraps round lands in the taps - 1 samples that are cut off)
    bank_f = torch.fft.rfft(torch.from_numpy(bank.astype(np.float32)).to(dev), n_fft)               # [n_irs][n_fft / 2 + 1], once
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kept = {}

    def library(ir_index):
        if K == 1:
            out = store.decode_window(speech, s_starts, window, dtype=torch.float32, resample=case["resample"], ir_index=ir_index, **kw)
        else:
            out = store.decode_window_sum(np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1),
                                          np.stack([np.ones(crops), gains], 1), window, dtype=torch.float32, resample=case["resample"],
                                          ir_index=np.stack([ir_index, np.full(crops, -1)], 1), **kw)
        return out, [dict(store.stats(), reverb=store.reverb_ms())], None

    def route_reverb():
        out, st, _ = library(irs)
        kept["reverb"] = out[:64].clone()
        return st, None

    def route_dry():
        out, st, _ = library(np.full(crops, -1))
        return st, None

    def route_torch():
        sts = []
        x = store.decode_window(speech, s_starts - (taps - 1), window + taps - 1, dtype=torch.float32, resample=case["resample"], **kw)
        sts.append(dict(store.stats(), reverb={"forward": 0.0, "fold": 0.0}))
        ev[0].record()
        y = torch.fft.irfft(torch.fft.rfft(x, n_fft) * bank_f[irs_dev][:, None, :], n_fft)[..., taps - 1:taps - 1 + window]
        if K == 2:
            b = store.decode_window(noise, n_starts, window, dtype=torch.float32, resample=case["resample"], **kw)
            sts.append(dict(store.stats(), reverb={"forward": 0.0, "fold": 0.0}))
            y = y + g_dev[:, None, None] * b
        else:
            y = y.contiguous()
        ev[1].record()
        torch.cuda.synchronize(dev)
        kept["torch"] = y[:64].clone()
        return sts, ev[0].elapsed_time(ev[1])

    routes = (("reverb", route_reverb), ("torch", route_torch), ("dry", route_dry))
    for _, fn in routes:                                         # warm-up round: workspaces, the filter's upload, rocFFT's plans
        fn()
    wall, sts, peak, expr = ({r: [] for r, _ in routes} for _ in range(4))
    for _ in range(reps):
        for r, fn in routes:
            kept.pop(r, None)
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            st, torch_ms = fn()
            wall[r].append(time.perf_counter() - t0)
            peak[r].append(torch.cuda.max_memory_allocated(dev) - before)
            sts[r].append(st)
            if torch_ms is not None:
                expr[r].append(torch_ms)
    res = {"K": K, "items": crops, "window": window, "out_shape": [crops, case["channels"], window], "impulse_responses": n_irs,
           "taps": taps, "reverb_block": REVERB_BLOCK, "torch_fft_points": n_fft,
           "arguments": dict({k: v for k, v in kw.items()}, resample=None if case["resample"] is None else list(case["resample"])),
           "rounds_timed": reps, "routes": {}}
    for r, _ in routes:
        ms = {k: round(float(np.median([sum(s["ms"][k] for s in call) for call in sts[r]])), 3) for k in MS_NAMES}
        for k in ("forward", "fold"):
            ms["reverb_" + k] = round(float(np.median([sum(s["reverb"][k] for s in call) for call in sts[r]])), 3)
        last = sts[r][-1]
        q25, q75 = np.percentile(wall[r], [25, 75])
        res["routes"][r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_all": [round(v, 5) for v in wall[r]],
                            "spread_seconds": {"interquartile": round(float(q75 - q25), 5), "range": round(float(max(wall[r]) - min(wall[r])), 5)},
                            "device_ms": ms, "library_calls": len(last), "peak_torch_bytes": int(np.median(peak[r])),
                            "stats": {k: sum(s[k] for s in last) for k in last[0] if k not in ("ms", "reverb")}}
    res["routes"]["torch"]["torch_device_ms"] = round(float(np.median(expr["torch"])), 3)
    a, t, d = (res["routes"][r] for r in ("reverb", "torch", "dry"))
    res["stage_seconds_by_difference"] = round(a["seconds_wall"] - d["seconds_wall"], 5)
    res["torch_wall_over_reverb_wall"] = round(t["seconds_wall"] / a["seconds_wall"], 3)
    x, y = kept["reverb"].double(), kept["torch"].double()
    res["agreement_64_items"] = {"max_abs_difference": float((x - y).abs().max()), "max_abs_value": float(x.abs().max())}
    print("%s: reverb %.5f s (forward %.3f ms, fold %.3f ms), torch %.5f s (its FFT expression %.3f ms), dry %.5f s; peak %d vs %d MiB" % (
        name, a["seconds_wall"], a["device_ms"]["reverb_forward"], a["device_ms"]["reverb_fold"], t["seconds_wall"], t["torch_device_ms"],
        d["seconds_wall"], a["peak_torch_bytes"] >> 20, t["peak_torch_bytes"] >> 20), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--irs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = a.cases.split(",")
    if a.reps < 1 or a.streams < 2 or a.irs < 1 or any(n not in CASES for n in names):
        ap.error("--reps and --irs at least 1, --streams at least 2, --cases among %s" % ",".join(CASES))
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "cases": {}}
    for n in names:
        res["cases"][n] = run_case(store, n, CASES[n], a.crops, a.reps, a.irs)
        if a.out:                                                # (kept case by case: a long run leaves what it has measured)
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/store_reverb_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}, f, indent=1)
    store.close()
    h.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
