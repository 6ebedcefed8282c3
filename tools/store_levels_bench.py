"""
Block energies of a resident corpus on an MI355X: PacStore.block_energy (mrc_pac_store_block_energy: the sum of squares of
every block's decoded MDCT lines, no inverse transform) against the only route there was without it -- decode_window of the
whole files as float32, in slabs, then squares and per-tile sums in torch -- in one process, the two routes taking turns, on
the workloads of tools/store_bench.py built from their seeds: `streams`, 256 stereo files of 600 hops, and `single`, the
65 536-hop stereo stream.  Per workload, rate divisor (1, 2, 4) and mix (every channel, mid): after a warm-up call of each
route the median over the timed calls of the wall seconds of both, the device time of the levels call by stage
(plan_upload, unpack, the energy kernel in the synthesis slot: PacStore.stats()) and its counts, the host time of building the
LevelMap, and the largest difference in dB between the two routes' RMS level of the one-second windows 0, 1, 2, ... s of every
file (the level map spreads a block's energy over its tile; the decoded route sums the samples) and of the files' totals (the
decoded route lacks what lies in the MDCT's delay, which decode_window drops).  The decoded route's wall time is split into
its decode_window calls and the rest (torch).  Profiler off.
  timeout -k 10 900 python tools/store_levels_bench.py --workload streams --out profiles/store_levels_bench.json
  timeout -k 10 900 python tools/store_levels_bench.py --workload single --out profiles/store_levels_bench.json
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
from mrcaudiocodec_amd.store import PacStore                                          # noqa: E402
from decode_bench import single_stream_file                                           # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

STAGES = ("plan_upload", "unpack", "synthesis")


def decoded_route(store, m, D, mix, piece, batch):
    """every file through decode_window as float32 in pieces of `piece` samples, `batch` pieces per call, squared and
    summed in float64 on the device -> per file the cumulative energy [channels][n + 1] (a tensor), from which the tile
    sums and any window's energy are differences"""
    import torch
    ns = store.n_samples_at(D)
    items = [(f, s) for f in range(len(store)) for s in range(0, int(ns[f]), piece)]
    parts = [[] for _ in range(len(store))]
    spent = {"decode_window_seconds": 0.0, "decode_window_device_ms": 0.0}
    for i in range(0, len(items), batch):
        fs, ss = zip(*items[i:i + batch])
        t0 = time.perf_counter()
        x = store.decode_window(fs, ss, piece, dtype=torch.float32, rate_divisor=D, mix=mix)
        spent["decode_window_seconds"] += time.perf_counter() - t0
        spent["decode_window_device_ms"] += sum(store.stats()["ms"].values())
        x = x.double().square_()
        for j, f in enumerate(fs):
            parts[f].append(x[j])
    out = []
    for f in range(len(store)):
        n = int(ns[f])
        sq = torch.cat(parts[f], dim=1)[:, :n]
        parts[f] = None
        cum = torch.zeros((sq.shape[0], n + 1), dtype=torch.float64, device=sq.device)
        for c in range(sq.shape[0]):                                 # (row by row: torch scans one long row far faster than two)
            torch.cumsum(sq[c], dim=0, out=cum[c, 1:])
        edges = torch.from_numpy(np.clip(m.tiles(f), 0, n).astype(np.int64)).to(sq.device)     # (whole numbers here)
        tiles = cum[:, edges[1:]] - cum[:, edges[:-1]]
        out.append((cum, tiles))
    torch.cuda.synchronize()
    return out, spent


def run(h, files, what, reps, piece, batch, rate):
    import torch
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "blocks": int(store.n_blocks.sum()), "samples_per_channel": int(store.n_samples.sum()),
           "calls_timed": reps, "cases": {}}
    for D in (1, 2, 4):
        for mix in (None, "mid"):
            store._levels.clear()
            t0 = time.perf_counter()
            m = store.levels(D, mix)
            first = time.perf_counter() - t0
            t = {"levels": [], "map": [], "decoded": []}
            sts = []
            dec, _ = decoded_route(store, m, D, mix, piece // D, batch)            # warm-up of the other route
            spent = []
            for _ in range(reps):
                t0 = time.perf_counter()
                off, blocks, energy = store.block_energy(D, mix)
                t["levels"].append(time.perf_counter() - t0)
                sts.append(store.stats())
                store._levels.clear()
                t0 = time.perf_counter()
                m = store.levels(D, mix)
                t["map"].append(time.perf_counter() - t0 - t["levels"][-1])       # (the second call's library time taken as the first's)
                t0 = time.perf_counter()
                dec, sp = decoded_route(store, m, D, mix, piece // D, batch)
                t["decoded"].append(time.perf_counter() - t0)
                spent.append(sp)
            # the two routes' one-second windows
            w, worst, total_rel = rate // D, 0.0, 0.0
            for f in range(len(files)):
                n = int(store.n_samples_at(D)[f])
                starts = np.arange(0, n - w + 1, w, dtype=np.int64)
                if not starts.size:
                    continue
                cum = dec[f][0].cpu().numpy()
                true = (cum[:, starts + w] - cum[:, starts]).T
                est = m.window_energy(np.full(len(starts), f), starts, w)[:, :true.shape[1]]
                both = (true > 0) & (est > 0)
                worst = max(worst, float(np.abs(10 * np.log10(est[both] / true[both])).max()))
                total_rel = max(total_rel, float(np.abs(m.total_energy(f) - cum[:, -1]).max() / cum[:, -1].max()))
            med = lambda v: round(float(np.median(v)), 5)
            ms = {k: round(float(np.median([s["ms"][k] for s in sts])), 3) for k in STAGES}
            r = {"first_call_seconds": round(first, 5), "levels_seconds_wall": med(t["levels"]), "level_map_seconds_host": med(t["map"]),
                 "decoded_route_seconds_wall": med(t["decoded"]), "levels_seconds_all": [round(v, 5) for v in t["levels"]],
                 "decoded_route_seconds_all": [round(v, 5) for v in t["decoded"]],
                 "decoded_route_decode_window_seconds": med([sp["decode_window_seconds"] for sp in spent]),
                 "decoded_route_decode_window_device_ms": round(float(np.median([sp["decode_window_device_ms"] for sp in spent])), 3),
                 "device_ms": {"plan_upload": ms["plan_upload"], "unpack": ms["unpack"], "block_energy_kernel": ms["synthesis"]},
                 "stats": {k: v for k, v in sts[-1].items() if k != "ms"},
                 "decoded_over_levels_wall": round(med(t["decoded"]) / med(t["levels"]), 2),
                 "one_second_windows_max_db_difference": round(worst, 4),
                 "file_total_max_relative_difference": float("%.3g" % total_rel)}
            res["cases"]["D=%d,%s" % (D, mix or "each")] = r
            print(json.dumps({"D": D, "mix": mix, **r}), flush=True)
            del dec
            torch.cuda.empty_cache()
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="streams", choices=("streams", "single"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--period", type=int, default=37)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--piece", type=int, default=1 << 20, help="samples per decoded piece at the full rate")
    ap.add_argument("--batch", type=int, default=16, help="pieces per decode_window call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    if a.workload == "streams":
        files, what = synth_stream_files(h, a.streams, a.stream_hops)
    else:
        files, what = single_stream_file(h, a.hops, a.period)
    res = run(h, files, what, a.reps, a.piece, a.batch, h.cfg.sample_rate)
    h.close()
    if a.out:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out["tool"] = "tools/store_levels_bench.py"
        out.setdefault("args", {})[a.workload] = {k: v for k, v in vars(a).items() if k != "out"}
        out[a.workload] = res
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
