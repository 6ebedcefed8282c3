"""
Mixtures of crops of resident 48 kHz `.pac` files as float32 tensors on an MI355X, on the `streams` corpus of
tools/store_reduced_bench.py (256 stereo streams of 600 hops): every item is a crop plus K - 1 crops of other files at drawn
gains.  Two routes take turns in one process, call after call, so that neither has the device to itself at another moment
than the other:
  sum    PacStore.decode_window_sum: one call, the terms folded from the float64 planes into the one output tensor
  torch  what a user did before the call existed: K PacStore.decode_window calls in float32 and a + g[:, None, None] * b
         (+ ... for K > 2) in torch
Cases: `16k_mid` -- one second at 16 kHz (rate_divisor=2, resample=(2, 3), mix="mid"), K = 2, 8192 items; `full_stereo_k2` and
`full_stereo_k4` -- one second at full rate, both channels.  Both routes allocate their tensors inside the timed call.  After a
warm-up round, per route the median over the timed rounds of the wall seconds of the whole route, the device time of the
stages (PacStore.stats(): plan_upload, unpack, synthesis, window_out -- summed over the K calls of the torch route, which
also has its torch expression alone, by events) and the peak of torch.cuda.max_memory_allocated (the library's own workspace
-- staging, parsed chunks, planes -- is not torch's and is the same size per term in both routes).  The condition recorded is
only that the sum route's median wall time is not above the torch route's by more than the torch route's own run-to-run
spread (the interquartile range of its timed rounds; the whole range is recorded beside it).  How far the routes agree on 64
items is recorded too (informative: the torch route rounds every term to float32 before it adds).  Nothing here decides a
ratio in advance: the JSON holds what was measured.
  timeout -k 10 900 python tools/store_sum_bench.py --out profiles/store_sum_bench.json
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
from store_bench import synth_stream_files                                            # noqa: E402

CASES = {
    "16k_mid": dict(K=2, window=16000, channels=1, kw=dict(rate_divisor=2, resample=(2, 3), mix="mid")),
    "full_stereo_k2": dict(K=2, window=48000, channels=2, kw=dict(channels=2)),
    "full_stereo_k4": dict(K=4, window=48000, channels=2, kw=dict(channels=2)),
}


def run_case(store, name, case, crops, reps):
    import torch
    dev = torch.device("cuda", 0)
    K, window, kw = case["K"], case["window"], case["kw"]
    rng = np.random.default_rng(23)
    n_files = len(store)
    first = rng.integers(0, n_files, crops)
    files = np.stack([first] + [(first + 1 + rng.integers(0, n_files - 1, crops)) % n_files for _ in range(K - 1)], 1)   # other files
    scale = window / 48000.0                                     # a file's length in the call's output samples over its own
    starts = (rng.random((crops, K)) * (store.n_samples[files] * scale - window)).astype(np.int64)   # wholly inside their files
    gains = np.concatenate([np.ones((crops, 1)), 10.0 ** (rng.uniform(-20.0, 0.0, (crops, K - 1)) / 20.0)], 1)
    g_dev = torch.from_numpy(gains.astype(np.float32)).to(dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kept = {}

    def route_sum():
        out = store.decode_window_sum(files, starts, gains, window, dtype=torch.float32, **kw)
        kept["sum"] = out[:64].clone()
        return [store.stats()], None

    def route_torch():
        sts, xs = [], []
        for k in range(K):
            xs.append(store.decode_window(files[:, k], starts[:, k], window, dtype=torch.float32, **kw))
            sts.append(store.stats())
        ev0.record()
        out = xs[0]
        for k in range(1, K):
            out = out + g_dev[:, k, None, None] * xs[k]
        ev1.record()
        torch.cuda.synchronize(dev)
        kept["torch"] = out[:64].clone()
        return sts, ev0.elapsed_time(ev1)

    routes = (("sum", route_sum), ("torch", route_torch))
    for _, fn in routes:                                         # warm-up round: workspaces, the filter's upload, torch's kernels
        fn()
    wall, sts, peak, expr = ({r: [] for r, _ in routes} for _ in range(4))
    for _ in range(reps):
        for r, fn in routes:
            kept.pop(r, None)
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            st, expr_ms = fn()
            wall[r].append(time.perf_counter() - t0)
            peak[r].append(torch.cuda.max_memory_allocated(dev) - base)
            sts[r].append(st)
            if expr_ms is not None:
                expr[r].append(expr_ms)
    res = {"K": K, "items": crops, "window": window, "out_shape": [crops, case["channels"], window],
           "arguments": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}, "rounds_timed": reps, "routes": {}}
    for r, _ in routes:
        ms = {k: round(float(np.median([sum(s["ms"][k] for s in call) for call in sts[r]])), 3) for k in MS_NAMES}
        last = sts[r][-1]
        res["routes"][r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_all": [round(v, 5) for v in wall[r]],
                            "device_ms": ms, "device_ms_total": round(sum(ms.values()), 3),
                            "peak_torch_bytes": int(np.median(peak[r])),
                            "stats": {k: sum(s[k] for s in last) for k in last[0] if k != "ms"}}
    t = res["routes"]["torch"]
    t["expression_device_ms"] = round(float(np.median(expr["torch"])), 3)
    t["device_ms_total"] = round(t["device_ms_total"] + t["expression_device_ms"], 3)
    q25, q75 = np.percentile(wall["torch"], [25, 75])
    res["torch_spread_seconds"] = {"interquartile": round(float(q75 - q25), 5), "range": round(float(max(wall["torch"]) - min(wall["torch"])), 5)}
    res["sum_wall_minus_torch_wall_seconds"] = round(res["routes"]["sum"]["seconds_wall"] - t["seconds_wall"], 5)
    res["sum_not_above_torch_by_more_than_its_spread"] = bool(res["sum_wall_minus_torch_wall_seconds"] <= float(q75 - q25))
    res["torch_wall_over_sum_wall"] = round(t["seconds_wall"] / res["routes"]["sum"]["seconds_wall"], 3)
    a, b = kept["sum"].double(), kept["torch"].double()
    res["agreement_64_items"] = {"max_abs_difference": float((a - b).abs().max()), "max_abs_value": float(a.abs().max())}
    print("%s: sum %.5f s, torch %.5f s (spread %.5f s), peak %d vs %d MiB" % (
        name, res["routes"]["sum"]["seconds_wall"], t["seconds_wall"], q75 - q25, res["routes"]["sum"]["peak_torch_bytes"] >> 20,
        t["peak_torch_bytes"] >> 20), flush=True)
    return res


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
    if a.reps < 1 or a.streams < 2 or any(n not in CASES for n in names):
        ap.error("--reps at least 1, --streams at least 2, --cases among %s" % ",".join(CASES))
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "cases": {n: run_case(store, n, CASES[n], a.crops, a.reps) for n in names}}
    store.close()
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        out = {"tool": "tools/store_sum_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
