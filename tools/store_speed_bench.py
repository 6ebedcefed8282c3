"""
Speed perturbation of crops of resident 48 kHz `.pac` files as float32 tensors on an MI355X, on the `streams` corpus of
tools/store_reduced_bench.py (256 stereo streams of 600 hops): every item is read at 0.9x, 1.0x or 1.1x, drawn uniformly per
item.  Two routes take turns in one process, call after call, so that neither has the device to itself at another moment
than the other:
  speeds  PacStore.decode_window(speed_factors=, speed_index=) (decode_window_sum for the mixture): one call, one plan, one
          output kernel (resample_multi_sum_out_kernel, natural lane map)
  calls   what a user did before the call existed: one PacStore.decode_window(resample=) call per speed on its subset of the
          items, index_copy_ of each result into the one float32 tensor, and for the mixture a + g * b in torch with b one more
          call at speed 1
Cases: `16k_mid` -- one second at 16 kHz (rate_divisor=2, resample=(2, 3), mix="mid"), 8192 items, the ratios 20 / 27, 2 / 3 and
20 / 33; `full_stereo` -- one second at full rate, both channels, the ratios 10 / 9, 1 and 10 / 11; `16k_mid_mixture` -- two
terms, speech at a drawn speed over noise at speed 1 at a drawn gain.  Both routes allocate their tensors inside the timed
call.  After a warm-up round, per route the median over the timed rounds of the wall seconds of the whole route, the device
time of the stages (PacStore.stats(): plan_upload, unpack, synthesis, window_out, summed over the calls of the `calls` route,
which also has its torch scatter and expression alone, by events read after the route's one final synchronisation; the
route waits only there, as a user's code would), slabs, and the peak of torch.cuda.max_memory_allocated.  Parse and
synthesis are the same work in both routes; what the one call saves is calls, synchronisations and the scatter, what it may
cost is the natural lane map in the output kernel.  Recorded beside each route: the other route's run-to-run spread (the
interquartile range of its timed rounds), and whether the one call's output stage exceeds the sum of the calls' output
stages by more than that spread.  `output_stage_by_ratio` takes the output stage apart: ALL items of the one-term cases at ONE
ratio of the list, through the speeds call (resample_multi_sum_out_kernel, natural map) and through the single-ratio call
(resample_out_kernel with the layout resample_lds_layout picks for that ratio, window_out_kernel for the unit ratio), the
median device time of the output kernel alone, beside the LDS layout each uses.  Nothing here decides a ratio in advance: the
JSON holds what was measured.
  timeout -k 10 900 python tools/store_speed_bench.py --out profiles/store_speed_bench.json
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
from mrcaudiocodec_amd.store import MS_NAMES, PacStore, speed_ratios                  # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

SPEEDS = [(9, 10), (1, 1), (11, 10)]
CASES = {
    "16k_mid": dict(K=1, window=16000, channels=1, D=2, resample=(2, 3), kw=dict(rate_divisor=2, mix="mid")),
    "full_stereo": dict(K=1, window=48000, channels=2, D=1, resample=None, kw=dict(channels=2)),
    "16k_mid_mixture": dict(K=2, window=16000, channels=1, D=2, resample=(2, 3), kw=dict(rate_divisor=2, mix="mid")),
}


def run_case(store, name, case, crops, reps):
    import torch
    dev = torch.device("cuda", 0)
    K, window, kw, D = case["K"], case["window"], case["kw"], case["D"]
    ratios = speed_ratios(case["resample"], SPEEDS)
    base = speed_ratios(case["resample"], [(1, 1)])[0]
    rng = np.random.default_rng(29)
    n_files = len(store)
    speech = rng.integers(0, n_files, crops)
    noise = (speech + 1 + rng.integers(0, n_files - 1, crops)) % n_files
    index = rng.integers(0, len(SPEEDS), crops)
    inside = lambda f, r: np.asarray(store.n_samples_resampled(*r, D), np.int64)[f]
    length = np.empty(crops, np.int64)
    for r, ratio in enumerate(ratios):                           # a file's length in the item's own output samples
        length[index == r] = inside(speech[index == r], ratio)
    s_starts = (rng.random(crops) * (length - window)).astype(np.int64)       # wholly inside their files
    n_starts = (rng.random(crops) * (inside(noise, base) - window)).astype(np.int64)
    gains = 10.0 ** (rng.uniform(-20.0, 0.0, crops) / 20.0)
    g_dev = torch.from_numpy(gains.astype(np.float32)).to(dev)
    sel = [np.flatnonzero(index == r) for r in range(len(SPEEDS))]
    sel_dev = [torch.from_numpy(s).to(dev) for s in sel]
    rs = lambda ratio: None if ratio[0] == ratio[1] else ratio
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(len(SPEEDS) + 1)]   # a pair per torch step
    kept = {}

    def route_speeds():
        if K == 1:
            out = store.decode_window(speech, s_starts, window, dtype=torch.float32, resample=case["resample"], speed_factors=SPEEDS,
                                      speed_index=index, **kw)
        else:
            out = store.decode_window_sum(np.stack([speech, noise], 1), np.stack([s_starts, n_starts], 1),
                                          np.stack([np.ones(crops), gains], 1), window, dtype=torch.float32, resample=case["resample"],
                                          speed_factors=SPEEDS + [(1, 1)], speed_index=np.stack([index, np.full(crops, 3)], 1), **kw)
        kept["speeds"] = out[:64].clone()
        return [store.stats()], None

    def route_calls():
        # as a user would write it: each scatter is queued behind its call and overlaps the next call's planning on the host;
        # the route waits once, at its end, and the events are read after that
        sts, used = [], []
        out = torch.empty((crops, case["channels"], window), dtype=torch.float32, device=dev)
        for r, ratio in enumerate(ratios):
            x = store.decode_window(speech[sel[r]], s_starts[sel[r]], window, dtype=torch.float32, resample=rs(ratio), **kw)
            sts.append(store.stats())
            ev[r][0].record()
            out.index_copy_(0, sel_dev[r], x)
            ev[r][1].record()
            used.append(ev[r])
        if K == 2:
            b = store.decode_window(noise, n_starts, window, dtype=torch.float32, resample=rs(base), **kw)
            sts.append(store.stats())
            ev[-1][0].record()
            out = out + g_dev[:, None, None] * b
            ev[-1][1].record()
            used.append(ev[-1])
        torch.cuda.synchronize(dev)
        kept["calls"] = out[:64].clone()
        return sts, sum(a.elapsed_time(b) for a, b in used)

    routes = (("speeds", route_speeds), ("calls", route_calls))
    for _, fn in routes:                                         # warm-up round: workspaces, the filters' uploads, torch's kernels
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
    res = {"K": K, "items": crops, "window": window, "out_shape": [crops, case["channels"], window], "speeds": [list(s) for s in SPEEDS],
           "ratios": [list(r) for r in ratios], "items_per_speed": [int(s.size) for s in sel],
           "arguments": dict({k: v for k, v in kw.items()}, resample=None if case["resample"] is None else list(case["resample"])),
           "rounds_timed": reps, "routes": {}}
    iqr = {}
    for r, _ in routes:
        ms = {k: round(float(np.median([sum(s["ms"][k] for s in call) for call in sts[r]])), 3) for k in MS_NAMES}
        last = sts[r][-1]
        q25, q75 = np.percentile(wall[r], [25, 75])
        iqr[r] = float(q75 - q25)
        res["routes"][r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_all": [round(v, 5) for v in wall[r]],
                            "spread_seconds": {"interquartile": round(iqr[r], 5), "range": round(float(max(wall[r]) - min(wall[r])), 5)},
                            "device_ms": ms, "device_ms_total": round(sum(ms.values()), 3), "library_calls": len(last),
                            "peak_torch_bytes": int(np.median(peak[r])),
                            "stats": {k: sum(s[k] for s in last) for k in last[0] if k != "ms"}}
    c, s = res["routes"]["calls"], res["routes"]["speeds"]
    c["torch_device_ms"] = round(float(np.median(expr["calls"])), 3)
    c["device_ms_total"] = round(c["device_ms_total"] + c["torch_device_ms"], 3)
    s["other_route_spread_seconds"], c["other_route_spread_seconds"] = round(iqr["calls"], 5), round(iqr["speeds"], 5)
    res["speeds_wall_minus_calls_wall_seconds"] = round(s["seconds_wall"] - c["seconds_wall"], 5)
    res["calls_wall_over_speeds_wall"] = round(c["seconds_wall"] / s["seconds_wall"], 3)
    res["output_stage_ms"] = {"speeds": s["device_ms"]["window_out"], "calls_summed": c["device_ms"]["window_out"]}
    res["speeds_output_stage_exceeds_calls_by_more_than_their_spread"] = bool(
        (s["device_ms"]["window_out"] - c["device_ms"]["window_out"]) * 1e-3 > iqr["calls"])
    if K == 1:                                                   # the output stage ratio by ratio: every item at that one ratio
        res["output_stage_by_ratio"] = {}
        for r, ratio in enumerate(ratios):
            starts_r = (rng.random(crops) * (inside(speech, ratio) - window)).astype(np.int64)
            one, single = [], []
            for _ in range(1 + max(3, reps // 2)):
                store.decode_window(speech, starts_r, window, dtype=torch.float32, resample=case["resample"], speed_factors=SPEEDS,
                                    speed_index=np.full(crops, r), **kw)
                one.append(store.stats()["ms"]["window_out"])
                store.decode_window(speech, starts_r, window, dtype=torch.float32, resample=rs(ratio), **kw)
                single.append(store.stats()["ms"]["window_out"])
            res["output_stage_by_ratio"]["%d/%d" % ratio] = {"speeds_call_ms": round(float(np.median(one[1:])), 3),
                                                             "single_ratio_call_ms": round(float(np.median(single[1:])), 3)}
        print("%s: output stage by ratio %s" % (name, json.dumps(res["output_stage_by_ratio"])), flush=True)
    a, b = kept["speeds"].double(), kept["calls"].double()
    res["agreement_64_items"] = {"max_abs_difference": float((a - b).abs().max()), "max_abs_value": float(a.abs().max())}
    print("%s: speeds %.5f s, calls %.5f s (spreads %.5f, %.5f s), output stage %.3f vs %.3f ms, peak %d vs %d MiB" % (
        name, s["seconds_wall"], c["seconds_wall"], iqr["speeds"], iqr["calls"], s["device_ms"]["window_out"], c["device_ms"]["window_out"],
        s["peak_torch_bytes"] >> 20, c["peak_torch_bytes"] >> 20), flush=True)
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
        out = {"tool": "tools/store_speed_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
