"""
Mono crops of a resident stereo corpus on an MI355X: PacStore.decode_window(mix="mid") against what a user did before the
call existed -- the two-channel float32 call followed by 0.5 * (x[:, 0] + x[:, 1]) in torch -- in one process, on the
workload of tools/store_bench.py: 256 stereo streams of 600 hops (synth.c3_stereo, encoded by the chained stream-mode call),
8192 random one-second crops, the same crops for every route, at D = 1, 2 and 4 (window = 48000 / D reduced samples, start =
the full-rate start / D; the full-rate starts are multiples of 4, so that every D reads the same second).
Per D and route, after a warm-up call of each, the two routes taking turns, the median over the timed calls of the wall
seconds (the torch mean included in the two-channel route, synchronised) and of the device time of the call's four stages (plan_upload, unpack, synthesis,
window_out: PacStore.stats()), and the call's counts.  The ratios mid / two-channel of the wall time and of every stage are
recorded; the expectation from the work counts is about one half for synthesis and window_out and one for unpack.  The two
routes' results are compared on every crop (max |difference|, informative: both are float32 roundings of values that differ
by float64 rounding).  mix="left" is measured once, at D = 1, for the record.
  timeout -k 10 900 python tools/store_mix_bench.py --out profiles/store_mix_bench.json
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


def alternate(fns, reps):
    """a warm-up call of each route, then reps rounds in which the routes take turns (what else runs on the machine then
    meets them alike) -> per route its record"""
    for fn in fns.values():
        fn()
    ts, sts = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            sts[k].append(fn())
            ts[k].append(time.perf_counter() - t0)
    return {k: record(ts[k], sts[k]) for k in fns}


def record(ts, sts):
    t = float(np.median(ts))
    ms = {k: round(float(np.median([s["ms"][k] for s in sts])), 3) for k in MS_NAMES}
    return {"seconds_wall": round(t, 5), "seconds_all": [round(v, 5) for v in ts], "device_ms": ms,
            "device_ms_total": round(sum(ms.values()), 3), "stats": {k: v for k, v in sts[-1].items() if k != "ms"}}


def run(h, files, what, crops, window, reps):
    import torch
    dev = torch.device("cuda", 0)
    store = PacStore(h, files)
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - window)).astype(np.int64) // 4 * 4   # wholly inside their files
    res = {"workload": what, "files": len(files), "crops": crops, "window_full_rate": window, "calls_timed": reps,
           "rate_divisor": {}}
    for D in (1, 2, 4):
        w = window // D
        two = torch.empty((crops, 2, w), dtype=torch.float32, device=dev)
        one = torch.empty((crops, 1, w), dtype=torch.float32, device=dev)
        mean = torch.empty((crops, w), dtype=torch.float32, device=dev)

        def two_then_mean():
            store.decode_window(which, starts // D, w, channels=2, dtype=torch.float32, out=two, rate_divisor=D)
            st = store.stats()
            torch.add(two[:, 0], two[:, 1], out=mean)
            mean.mul_(0.5)
            torch.cuda.synchronize(dev)
            return st

        def mix(name):
            def call():
                store.decode_window(which, starts // D, w, dtype=torch.float32, out=one, rate_divisor=D, mix=name)
                return store.stats()
            return call
        r = dict({"window": w}, **alternate({"two_channel_then_torch_mean": two_then_mean, "mid": mix("mid")}, reps))
        a, b = r["mid"], r["two_channel_then_torch_mean"]
        r["mid_over_two_channel"] = dict({"seconds_wall": round(a["seconds_wall"] / b["seconds_wall"], 3)},
                                         **{k: round(a["device_ms"][k] / b["device_ms"][k], 3) for k in MS_NAMES})
        r["max_abs_difference_of_the_routes"] = float((one[:, 0] - mean).abs().max())
        r["max_abs_value"] = float(mean.abs().max())
        if D == 1:
            r.update(alternate({"left": mix("left")}, reps))
            r["left_is_channel_0_of_the_two_channel_call"] = bool(torch.equal(one[:, 0], two[:, 0]))
        res["rate_divisor"][str(D)] = r
        del two, one, mean
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--window", type=int, default=48000, help="at the full rate; a multiple of 4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.window % 4 or a.reps < 1:
        ap.error("--window must be a multiple of 4 and --reps at least 1")
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    res = run(h, files, what, a.crops, a.window, a.reps)
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/store_mix_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"},
                       "streams": res}, f, indent=1)


if __name__ == "__main__":
    main()
