"""
Routed windows of resident 48 kHz `.pac` files as float32 tensors on an MI355X, on the corpus and by the method of
tools/store_reverb_bench.py (256 stereo streams of 600 hops; 8192 one-second items at 16 kHz mid: rate_divisor=2,
resample=(2, 3), mix="mid"; synthetic room responses of 8000 taps): the routes of a case take turns in one process, call after
call, and after a warm-up round the JSON holds per route the median over the timed rounds of the wall seconds, their
interquartile range, the device time per stage (PacStore.stats(), reverb_ms()), route_info() and the peak of
torch.cuda.max_memory_allocated.
  array_4, array_8     one term through the C microphones of a room drawn per item (the bank room-major, store.array_routes):
      routed     PacStore.decode_window_routed, one call, the channel group chosen by the library (MRC_OPT_STORE_ROUTE_GROUP 0)
      routed_g1  the same call with one channel per workgroup: the parent's kernel shape with a channel index
      routed_g2  the same call with two channels per workgroup, which load a shared source's spectra once
      calls      what a user did before: C x PacStore.decode_window(ir_index=) and torch.cat
  mixture_targets      channel 0 speech through a room over dry noise, channel 1 the dry speech, channel 2 the noise alone:
      routed / routed_g1 / routed_g2 as above; calls: decode_window_sum(ir_index=), decode_window, decode_window_sum of the noise term
Every case records whether the routed tensors equal the calls' bit for bit, and the fold's device time PER CHANNEL of the
routed routes beside reverb_fold_kernel's for one channel in the same run (the calls route's fold time per call).
Nothing here decides a ratio in advance: the JSON holds what was measured.
  timeout -k 10 1100 python tools/store_route_bench.py --out profiles/store_route_bench.json
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
from mrcaudiocodec_amd import Handle, _lib                                            # noqa: E402
from mrcaudiocodec_amd.store import MS_NAMES, REVERB_BLOCK, ROUTE_NONE, PacStore, array_routes   # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402
from store_reverb_bench import synth_rirs                                             # noqa: E402

KW = dict(rate_divisor=2, mix="mid", resample=(2, 3))
WINDOW, RATE, TAPS = 16000, 16000, 8000
CASES = {"array_4": 4, "array_8": 8, "mixture_targets": 3}


def run_case(h, store, name, crops, reps, n_rooms):
    import torch
    dev = torch.device("cuda", 0)
    C = CASES[name]
    array = name.startswith("array")
    n_irs = n_rooms * C if array else n_rooms
    store.set_impulse_responses(list(synth_rirs(n_irs, TAPS)))
    rng = np.random.default_rng(31)
    n_files = len(store)
    speech = rng.integers(0, n_files, crops)
    noise = (speech + 1 + rng.integers(0, n_files - 1, crops)) % n_files
    inside = lambda f: np.asarray(store.n_samples_resampled(2, 3, 2), np.int64)[f]
    s_starts = TAPS + (rng.random(crops) * (inside(speech) - WINDOW - TAPS)).astype(np.int64)
    n_starts = (rng.random(crops) * (inside(noise) - WINDOW)).astype(np.int64)
    gains = 10.0 ** (rng.uniform(-20.0, 0.0, crops) / 20.0)
    rooms = rng.integers(0, n_rooms, crops)
    kept = {}
    if array:
        route_gains, route_irs = array_routes(rooms, C)
        files, starts, offsets = speech, s_starts, np.arange(crops + 1, dtype=np.int64)
    else:
        files, starts = np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1)
        offsets = None
        route_irs = np.empty((crops, 2, 3), np.int32)
        route_irs[:, 0], route_irs[:, 1] = np.stack([rooms, np.full(crops, -1), np.full(crops, ROUTE_NONE)], 1), (-1, ROUTE_NONE, -1)
        route_gains = np.ones((crops, 2, 3))
        route_gains[:, 1] = gains[:, None]
    stat = lambda: dict(store.stats(), reverb=store.reverb_ms())

    def routed(group):
        def fn():
            h.set_option(_lib.MRC_OPT_STORE_ROUTE_GROUP, group)
            out = store.decode_window_routed(files, starts, route_gains, route_irs, WINDOW, item_offsets=offsets, dtype=torch.float32, **KW)
            kept["routed"] = out
            return [dict(stat(), route_info=store.route_info())]
        return fn

    def calls():
        sts, parts = [], []
        if array:
            for c in range(C):
                parts.append(store.decode_window(speech, s_starts, WINDOW, dtype=torch.float32, ir_index=route_irs[:, c], **KW))
                sts.append(stat())
        else:
            parts.append(store.decode_window_sum(files, starts, np.stack([np.ones(crops), gains], 1), WINDOW, dtype=torch.float32,
                                                 ir_index=np.stack([rooms, np.full(crops, -1)], 1), **KW))
            sts.append(stat())
            no_room = lambda: dict(store.stats(), reverb={"forward": 0.0, "fold": 0.0})      # (reverb_ms is the last reverb call's)
            parts.append(store.decode_window(speech, s_starts, WINDOW, dtype=torch.float32, **KW))
            sts.append(no_room())
            parts.append(store.decode_window_sum(noise[:, None], n_starts[:, None], gains[:, None], WINDOW, dtype=torch.float32, **KW))
            sts.append(no_room())
        kept["calls"] = torch.cat(parts, 1)
        torch.cuda.synchronize(dev)
        return sts

    default_group = h.get_option(_lib.MRC_OPT_STORE_ROUTE_GROUP)
    routes = (("routed", routed(default_group)), ("routed_g1", routed(1)), ("routed_g2", routed(2)), ("calls", calls))
    for _, fn in routes:                                         # warm-up round: workspaces, the filter's upload
        fn()
    equal = bool(torch.equal(kept["routed"], kept["calls"]))
    wall, sts, peak = ({r: [] for r, _ in routes} for _ in range(3))
    for _ in range(reps):
        for r, fn in routes:
            kept.clear()
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            st = fn()
            wall[r].append(time.perf_counter() - t0)
            peak[r].append(torch.cuda.max_memory_allocated(dev) - before)
            sts[r].append(st)
    h.set_option(_lib.MRC_OPT_STORE_ROUTE_GROUP, default_group)
    res = {"items": crops, "window": WINDOW, "channels": C, "out_shape": [crops, C, WINDOW], "impulse_responses": n_irs, "taps": TAPS,
           "reverb_block": REVERB_BLOCK, "route_group": default_group, "arguments": dict(KW, resample=list(KW["resample"])),
           "rounds_timed": reps, "routed_equals_calls_bit_for_bit": equal, "routes": {}}
    for r, _ in routes:
        total = lambda key, sub=None: [sum((s[key][sub] if sub else s[key]) for s in call) for call in sts[r]]
        ms = {k: round(float(np.median(total("ms", k))), 3) for k in MS_NAMES}
        fold = total("reverb", "fold")
        ms["reverb_forward"], ms["reverb_fold"] = round(float(np.median(total("reverb", "forward"))), 3), round(float(np.median(fold)), 3)
        last = sts[r][-1]
        q25, q75 = np.percentile(wall[r], [25, 75])
        f25, f75 = np.percentile(fold, [25, 75])
        res["routes"][r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_all": [round(v, 5) for v in wall[r]],
                            "spread_seconds": {"interquartile": round(float(q75 - q25), 5), "range": round(float(max(wall[r]) - min(wall[r])), 5)},
                            "device_ms": ms, "fold_ms_interquartile": round(float(f75 - f25), 3), "library_calls": len(last),
                            "peak_torch_bytes": int(np.median(peak[r])),
                            "stats": {k: sum(s[k] for s in last) for k in last[0] if k not in ("ms", "reverb", "route_info")}}
        if "route_info" in last[0]:
            res["routes"][r]["route_info"] = last[0]["route_info"]
    a, g1, g2, c = (res["routes"][r] for r in ("routed", "routed_g1", "routed_g2", "calls"))
    res["calls_wall_over_routed_wall"] = round(c["seconds_wall"] / a["seconds_wall"], 3)
    res["wall_gain_seconds"] = round(c["seconds_wall"] - a["seconds_wall"], 5)
    res["sum_of_interquartile_ranges_seconds"] = round(c["spread_seconds"]["interquartile"] + a["spread_seconds"]["interquartile"], 5)
    if array:                                                    # the fold per channel: every channel is wet here
        res["fold_ms_per_channel"] = {"routed": round(a["device_ms"]["reverb_fold"] / C, 3), "routed_g1": round(g1["device_ms"]["reverb_fold"] / C, 3),
                                      "routed_g2": round(g2["device_ms"]["reverb_fold"] / C, 3),
                                      "reverb_fold_kernel_one_channel": round(c["device_ms"]["reverb_fold"] / C, 3),
                                      "interquartile_per_channel": {"routed": round(a["fold_ms_interquartile"] / C, 3),
                                                                    "routed_g1": round(g1["fold_ms_interquartile"] / C, 3),
                                                                    "routed_g2": round(g2["fold_ms_interquartile"] / C, 3),
                                                                    "calls": round(c["fold_ms_interquartile"] / C, 3)}}
    print("%s: routed %.5f s (group option %d; fold %.3f ms), one channel per workgroup %.5f s (fold %.3f ms), two %.5f s (fold %.3f ms), "
          "calls %.5f s (fold %.3f ms); equal %s; peak %d vs %d MiB" % (
                                 name, a["seconds_wall"], default_group, a["device_ms"]["reverb_fold"], g1["seconds_wall"],
                                 g1["device_ms"]["reverb_fold"], g2["seconds_wall"], g2["device_ms"]["reverb_fold"], c["seconds_wall"],
                                 c["device_ms"]["reverb_fold"], equal,
                                 a["peak_torch_bytes"] >> 20, c["peak_torch_bytes"] >> 20), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = a.cases.split(",")
    if a.reps < 1 or a.streams < 2 or a.rooms < 1 or any(n not in CASES for n in names):
        ap.error("--reps and --rooms at least 1, --streams at least 2, --cases among %s" % ",".join(CASES))
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "cases": {}}
    for n in names:
        res["cases"][n] = run_case(h, store, n, a.crops, a.reps, a.rooms)
        if a.out:                                                # (kept case by case: a long run leaves what it has measured)
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/store_route_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}, f, indent=1)
    store.close()
    h.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
