"""
Encode to a target noise-to-mask ratio (mrc_encode_chained_target_nmr_pac) on the README's single-stream workload: ONE stereo
stream of --hops hops (tools/single_stream_bench.make_stream: noise floor + tone, a burst every 37th hop; shapes from the
transient detector), host to host, with ladders of 4 and 8 rates.
  new    Handle.encode_chained_pac_target_nmr: PCM in, the chosen file and every rung's NMR out;
  old    the route it replaces, on the entry points that existed before: Handle.encode_chained_pac_ladder (all R files to
         the host), then Handle.pac_nmr on the R files against the shared source.
Every case is warmed up once, then timed --reps times (>= 7): wall clock around the call(s), the median taken, with the
library's device-event times beside it (mrc_get_target_ms: phase A + prep, scan, NMR, pack + gather; mrc_get_chain_ms and
mrc_get_nmr_ms for the old route).  The two bars of the report: wall_new < wall_old at both R, and the NMR device time at
R = 8 below twice that at R = 4 (the mask terms and the threshold pass are shared by the rungs).
usage: python tools/target_nmr_bench.py [--hops 65536] [--reps 7] [--out profiles/target_nmr_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrcaudiocodec_amd import Handle, transient               # noqa: E402
from single_stream_bench import make_stream                   # noqa: E402

LADDERS = {4: (1.5, 2.86, 4.0, 8.0), 8: (1.5, 2.0, 2.86, 3.5, 4.0, 5.0, 6.0, 8.0)}
TARGET_PARTS = ("phase_a_prep", "scan", "nmr", "pack_gather")


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    pcm = make_stream(a.hops, 37)
    shapes = transient.block_shape_array(h, pcm)
    shapes = shapes[:np.nonzero(shapes[:, 2] == 1024)[0][-1] + 1]
    ns = int(shapes[:, 2].sum())
    end = int(shapes[-1].sum())
    src = np.ascontiguousarray(pcm[:, 1024:end])
    left, right = pcm[0][None], pcm[1][None]
    report = {"what": "mrc_encode_chained_target_nmr_pac host to host against the ladder call followed by mrc_pac_nmr on its "
                      "files; wall ms around the call(s), device ms from the library's events; median / min / max over reps "
                      "after one warm-up",
              "workload": "ONE stereo stream of %d hops, %d blocks (%d short / transition)" %
                          (a.hops, len(shapes), int((shapes[:, 1] + shapes[:, 2] != 2048).sum())),
              "source_bytes": int(src.nbytes), "reps": a.reps}
    for R, rates in LADDERS.items():
        def new():
            r = h.encode_chained_pac_target_nmr(left, right, [shapes], rates, target, num_samples=[ns])[0]
            return r, h.target_ms()

        def old():
            rs = h.encode_chained_pac_ladder(left, right, [shapes], rates, num_samples=[ns])
            ms_chain = h.chain_ms()
            files = [r["bytes"] for r in rs]
            res = h.pac_nmr(files, [src] * len(files))
            return (files, res), np.concatenate([ms_chain, h.nmr_ms()])

        target = np.inf
        (files, res), _ = old()                                       # warm-up of the old route; its values pick the target
        tot = [r["nmr_total_db"] for r in res]
        target = 0.5 * (tot[R // 2 - 1] + tot[R // 2])               # a rung in the middle of the ladder is chosen
        got, _ = new()                                                # warm-up of the new call
        same = (got["data"] == files[got["chosen"]].tobytes() and list(got["nmr_total_db"]) == tot and
                list(got["nmr_max_db"]) == [r["nmr_max_db"] for r in res])
        walls = {"new": [], "old": []}
        dev = {"new": [], "old": []}
        for _ in range(a.reps):                                       # interleaved: drift hits both alike
            for name, fn in (("new", new), ("old", old)):
                t0 = time.perf_counter()
                _, ms = fn()
                walls[name].append((time.perf_counter() - t0) * 1e3)
                dev[name].append(ms)
        dn, do = np.array(dev["new"]), np.array(dev["old"])
        report["R%d" % R] = {
            "rates": list(rates), "target_nmr_total_db": target, "chosen": got["chosen"], "met": got["met"],
            "nmr_total_db": tot, "pac_bytes": [len(f) for f in files], "equal_to_old_route": bool(same),
            "new": {"wall_ms": spread(walls["new"]),
                    "device_ms": {k: spread(dn[:, i]) for i, k in enumerate(TARGET_PARTS)}},
            "old": {"wall_ms": spread(walls["old"]),
                    "chain_device_ms": {k: spread(do[:, i]) for i, k in enumerate(("phase_a_prep", "scan", "pack", "all"))},
                    "nmr_device_ms": {k: spread(do[:, 4 + i]) for i, k in enumerate(("h2d", "unpack", "source_analysis", "nmr_and_d2h"))}},
        }
        rep = report["R%d" % R]
        rep["wall_new_over_old"] = round(rep["new"]["wall_ms"]["median"] / rep["old"]["wall_ms"]["median"], 4)
        rep["wall_bar_met"] = rep["new"]["wall_ms"]["median"] < rep["old"]["wall_ms"]["median"]
        print(json.dumps({"R%d" % R: rep}), flush=True)
    ratio = report["R8"]["new"]["device_ms"]["nmr"]["median"] / report["R4"]["new"]["device_ms"]["nmr"]["median"]
    report["nmr_device_ms_R8_over_R4"] = round(ratio, 4)
    report["mask_sharing_bar_met"] = ratio < 2.0
    print(json.dumps({k: report[k] for k in ("nmr_device_ms_R8_over_R4", "mask_sharing_bar_met")}), flush=True)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
