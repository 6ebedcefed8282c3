"""
Random one-second crops of resident 48 kHz `.pac` files read at 16 kHz, as float32 tensors [crops][2][16000] on an MI355X,
on the `streams` corpus of tools/store_reduced_bench.py (256 stereo streams of 600 hops, 8192 crops).  Three routes take
turns in one process, call after call, so that none of them has the device to itself at another moment than the others:
  a  PacStore.decode_window(rate_divisor=2, resample=(2, 3))   half-rate synthesis from the MDCT lines, then the polyphase
     resampler on the planes (what store.resample_plan(48000, 16000) says)
  b  PacStore.decode_window(rate_divisor=1, resample=(1, 3))   full-rate synthesis, the resampler on the planes
  c  PacStore.decode_window at full rate as float32 [crops][2][48000], then torch.nn.functional.conv1d with the library's
     own taps for 1 / 3 (store.resample_taps, as float32) and stride 3: what a user did before the call existed
The full-rate starts are multiples of 12, so that all three read the same second (a's samples sit half a full-rate sample
after b's and c's: the half-rate signal's own offset).  After a warm-up round, per route the median over the timed rounds of
the wall seconds of the whole route and the device time of its stages (PacStore.stats(): plan_upload, unpack, synthesis,
window_out, which is resample_out_kernel for a and b; for c also the conv1d alone, by events).  How far the routes agree on
the inside of 64 crops is recorded too (informative: c rounds to float32 before the filter; a cuts the band at 12 kHz first and its samples lie
half a full-rate sample from b's, which alone bounds their agreement on wide-band content: white noise limited to 7.6 kHz
and shifted by that much is 10.8 dB from itself).  Nothing here decides a ratio in advance: the JSON holds what was measured.
  timeout -k 10 900 python tools/store_resample_bench.py --out profiles/store_resample_bench.json
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
from mrcaudiocodec_amd.store import MS_NAMES, PacStore, resample_plan, resample_taps  # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402


def run(h, files, what, crops, reps, rate_in=48000, rate_out=16000):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    store = PacStore(h, files)
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - rate_in)).astype(np.int64) // 12 * 12     # wholly inside their files
    out_starts = starts // 3
    plan = resample_plan(rate_in, rate_out)
    assert plan == (2, 2, 3), plan
    W3, taps3 = resample_taps(1, 3)
    fir = torch.from_numpy(taps3[0].astype(np.float32)).to(dev).view(1, 1, 2 * W3)
    outs = {r: torch.empty((crops, 2, rate_out), dtype=torch.float32, device=dev) for r in "ab"}
    full = torch.empty((crops, 2, rate_in), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kept = {}

    def route_a():
        store.decode_window(which, out_starts, rate_out, channels=2, dtype=torch.float32, out=outs["a"], rate_divisor=2, resample=(2, 3))
        return store.stats(), None

    def route_b():
        store.decode_window(which, out_starts, rate_out, channels=2, dtype=torch.float32, out=outs["b"], rate_divisor=1, resample=(1, 3))
        return store.stats(), None

    def route_c():
        store.decode_window(which, starts, rate_in, channels=2, dtype=torch.float32, out=full)
        st = store.stats()
        ev0.record()
        y = F.conv1d(full.view(crops * 2, 1, rate_in), fir, stride=3, padding=W3 - 1)   # out n reads full[3 n - W + 1 + j]
        ev1.record()
        torch.cuda.synchronize(dev)
        kept["c"] = y.view(crops, 2, -1)[:64].clone()
        return st, ev0.elapsed_time(ev1)

    routes = (("a", route_a), ("b", route_b), ("c", route_c))
    for _, fn in routes:                                         # warm-up round: workspaces, the filters' upload, conv1d's kernel
        fn()
    wall = {r: [] for r, _ in routes}
    sts = {r: [] for r, _ in routes}
    conv = []
    for _ in range(reps):
        for r, fn in routes:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st, conv_ms = fn()
            wall[r].append(time.perf_counter() - t0)
            sts[r].append(st)
            if conv_ms is not None:
                conv.append(conv_ms)
    about = {"a": "rate_divisor=2, resample=(2, 3)", "b": "rate_divisor=1, resample=(1, 3)",
             "c": "decode_window at full rate as float32, then conv1d with the library's 1 / 3 taps (%d, float32), stride 3" % (2 * W3)}
    res = {"workload": what, "files": len(files), "crops": crops, "rate_in": rate_in, "rate_out": rate_out, "rounds_timed": reps,
           "out_shape": [crops, 2, rate_out], "resample_plan": list(plan), "routes": {}}
    for r, _ in routes:
        ms = {k: round(float(np.median([s["ms"][k] for s in sts[r]])), 3) for k in MS_NAMES}
        res["routes"][r] = {"what": about[r], "seconds_wall": round(float(np.median(wall[r])), 5),
                            "seconds_all": [round(v, 5) for v in wall[r]], "device_ms": ms,
                            "device_ms_total": round(sum(ms.values()), 3),
                            "stats": {k: v for k, v in sts[r][-1].items() if k != "ms"}}
    res["routes"]["c"]["conv1d_device_ms"] = round(float(np.median(conv)), 3)
    res["routes"]["c"]["device_ms_total"] = round(res["routes"]["c"]["device_ms_total"] + res["routes"]["c"]["conv1d_device_ms"], 3)
    c_wall = res["routes"]["c"]["seconds_wall"]
    for r in "ab":
        res["routes"][r]["wall_of_route_c_over_this"] = round(c_wall / res["routes"][r]["seconds_wall"], 3)
    inside = slice(64, -64)
    sig = {r: outs[r][:64, :, inside].double() for r in "ab"}
    sig["c"] = kept["c"][:, :, inside].double()
    snr = lambda x, y: round(float(10 * torch.log10((y * y).sum() / ((x - y) ** 2).sum())), 2)
    res["agreement_snr_db_64_crops"] = {"b_vs_c": snr(sig["b"], sig["c"]), "a_vs_b_half_a_full_rate_sample_apart": snr(sig["a"], sig["b"])}
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 1:
        ap.error("--reps at least 1")
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    res = run(h, files, what, a.crops, a.reps)
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        out = {"tool": "tools/store_resample_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
