"""
Constant-quality VBR (mrc_encode_vbr_nmr_pac) against the budgeted chained encode, host to host.
  single   the README's single-stream workload: ONE stereo stream of --hops hops (tools/single_stream_bench.make_stream),
           at ceilings 0 and -6 dB;
  batch    --streams stereo streams of --batch-hops hops each (12 blocks per stream without transients), ceiling 0 dB.
Routes, interleaved in every repetition so that drift hits them alike:
  vbr      Handle.encode_vbr_nmr_pac, with mrc_get_vbr_ms (phase A + source analysis, allocator, pack);
  chained  Handle.encode_chained_pac at the handle's rate (2.86 bits per sample), with mrc_get_chain_ms;
  target   (single only) Handle.encode_chained_pac_target_nmr over a ladder with an infinite target: every rung's size and NMR
           -- the rung nearest in size to each VBR file is what its quality is compared with.
Every route is warmed up once, then timed --reps times (>= 7): wall clock around the call, the median taken.  File sizes,
nmr_total_db, nmr_max_db and disturbed_blocks of every file are reported (the chained file's by mrc_pac_nmr).
usage: python tools/vbr_bench.py [--hops 65536] [--streams 8192] [--batch-hops 12] [--reps 7] [--out profiles/vbr_bench.json]
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

LADDER = (1.0, 1.5, 2.0, 2.86, 3.5, 4.0, 5.0, 6.0)
VBR_PARTS = ("phase_a_source_analysis", "allocator", "pack", "all")
CHAIN_PARTS = ("phase_a_prep", "scan", "pack", "all")


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def timed(routes, reps):
    walls = {k: [] for k in routes}
    dev = {k: [] for k in routes}
    for k, fn in routes.items():
        fn()                                                          # warm-up
    for _ in range(reps):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            ms = fn()
            walls[k].append((time.perf_counter() - t0) * 1e3)
            dev[k].append(ms)
    return walls, dev


def quality(rs):
    return {"bytes": int(sum(len(r["data"]) for r in rs)), "nmr_total_db": [r["nmr_total_db"] for r in rs][:4],
            "nmr_max_db": [r["nmr_max_db"] for r in rs][:4], "disturbed_blocks": int(sum(r["disturbed_blocks"] for r in rs)),
            "capped_bands": int(sum(r.get("capped_bands", 0) for r in rs)), "n_blocks": int(sum(r["n_blocks"] for r in rs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--batch-hops", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    report = {"what": "mrc_encode_vbr_nmr_pac against mrc_encode_chained_stream_pac (2.86 bits per sample), host to host; wall "
                      "ms around the call, device ms from the library's events; median / min / max over reps after one "
                      "warm-up, routes interleaved", "reps": a.reps}

    # ---- one long stream
    pcm = make_stream(a.hops, 37)
    shapes = transient.block_shape_array(h, pcm)
    shapes = shapes[:np.nonzero(shapes[:, 2] == 1024)[0][-1] + 1]
    ns = int(shapes[:, 2].sum())
    src = np.ascontiguousarray(pcm[:, 1024:int(shapes[-1].sum())])
    left, right = pcm[0][None], pcm[1][None]
    keep = {}

    def vbr(db):
        def run():
            keep[db] = h.encode_vbr_nmr_pac(left, right, [shapes], db, num_samples=[ns])
            return h.vbr_ms()
        return run

    def chained():
        keep["chained"] = h.encode_chained_pac(left, right, [shapes], num_samples=[ns])
        return h.chain_ms()

    walls, dev = timed({"vbr_0db": vbr(0.0), "vbr_-6db": vbr(-6.0), "chained": chained}, a.reps)
    lad = h.encode_chained_pac_target_nmr(left, right, [shapes], LADDER, np.inf, num_samples=[ns])[0]
    lad_bytes = [len(f["bytes"]) for f in h.encode_chained_pac_ladder(left, right, [shapes], LADDER, num_samples=[ns])]
    chained_file = keep["chained"]["bytes"].tobytes()
    meas = h.pac_nmr([chained_file], [src])[0]
    single = {"workload": "ONE stereo stream of %d hops, %d blocks (%d short / transition)" %
                          (a.hops, len(shapes), int((shapes[:, 1] + shapes[:, 2] != 2048).sum())),
              "chained": {"wall_ms": spread(walls["chained"]),
                          "device_ms": {k: spread(np.array(dev["chained"])[:, i]) for i, k in enumerate(CHAIN_PARTS)},
                          "bytes": len(chained_file), **{k: meas[k] for k in ("nmr_total_db", "nmr_max_db", "disturbed_blocks", "n_blocks")}},
              "ladder": {"rates": list(LADDER), "bytes": lad_bytes, "nmr_total_db": [float(v) for v in lad["nmr_total_db"]],
                         "nmr_max_db": [float(v) for v in lad["nmr_max_db"]],
                         "disturbed_blocks": [int(v) for v in lad["disturbed_blocks"]]}}
    for db, key in ((0.0, "vbr_0db"), (-6.0, "vbr_-6db")):
        q = quality(keep[db])
        near = int(np.argmin([abs(b - q["bytes"]) for b in lad_bytes]))
        single[key] = {"wall_ms": spread(walls[key]),
                       "device_ms": {k: spread(np.array(dev[key])[:, i]) for i, k in enumerate(VBR_PARTS)},
                       "bits_per_sample": keep[db][0]["coded_bits"] / (2.0 * ns), **q,
                       "wall_over_chained": round(float(np.median(walls[key]) / np.median(walls["chained"])), 4),
                       "nearest_rung": {"rate": LADDER[near], "bytes": lad_bytes[near], "nmr_total_db": float(lad["nmr_total_db"][near]),
                                        "nmr_max_db": float(lad["nmr_max_db"][near]), "disturbed_blocks": int(lad["disturbed_blocks"][near])}}
    report["single"] = single
    print(json.dumps({"single": single}), flush=True)

    # ---- many short streams
    one = make_stream(a.batch_hops, 1 << 30)                          # (no bursts: long blocks only)
    rng = np.random.default_rng(7)
    n = one.shape[1]
    L = np.empty((a.streams, n), np.int16)
    R = np.empty((a.streams, n), np.int16)
    for s in range(a.streams):                                        # the same content at a gain per stream
        g = 0.25 + 0.75 * rng.random()
        L[s], R[s] = (one[0] * g).astype(np.int16), (one[1] * g).astype(np.int16)
    bshape = np.array([(i * 1024, 1024, 1024) for i in range(a.batch_hops)], np.int64)
    bshapes, bns = [bshape] * a.streams, [a.batch_hops * 1024] * a.streams

    def bvbr():
        keep["bvbr"] = h.encode_vbr_nmr_pac(L, R, bshapes, 0.0, num_samples=bns)
        return h.vbr_ms()

    def bchained():
        keep["bchained"] = h.encode_chained_pac(L, R, bshapes, num_samples=bns)
        return h.chain_ms()

    walls, dev = timed({"vbr_0db": bvbr, "chained": bchained}, a.reps)
    batch = {"workload": "%d stereo streams of %d long blocks" % (a.streams, a.batch_hops),
             "vbr_0db": {"wall_ms": spread(walls["vbr_0db"]),
                         "device_ms": {k: spread(np.array(dev["vbr_0db"])[:, i]) for i, k in enumerate(VBR_PARTS)}, **quality(keep["bvbr"])},
             "chained": {"wall_ms": spread(walls["chained"]),
                         "device_ms": {k: spread(np.array(dev["chained"])[:, i]) for i, k in enumerate(CHAIN_PARTS)},
                         "bytes": int(keep["bchained"]["total"])}}
    batch["vbr_0db"]["wall_over_chained"] = round(float(np.median(walls["vbr_0db"]) / np.median(walls["chained"])), 4)
    report["batch"] = batch
    print(json.dumps({"batch": batch}), flush=True)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
