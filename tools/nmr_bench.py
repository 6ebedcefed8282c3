"""
Noise-to-mask ratio (mrc_pac_nmr) of the README's single-stream workload: ONE stereo stream of --hops hops
(tools/single_stream_bench.make_stream: noise floor + tone, a burst every 37th hop; shapes from the transient detector),
encoded by the chained call, then measured.
  (a) one_file:         the 2.86 bits-per-sample file, one call; the chained encode of the same stream for scale;
  (b) ladder_one_call:  the four files of a 1.5 / 2.86 / 4 / 8 ladder in ONE call against one shared source;
  (c) ladder_4_calls:   the same four files in four calls;
  (d) numpy_restatement: tests/nmr_restatement.py on a --slice-hop slice of the 2.86 file, for context (seconds per hop).
Every case is warmed up once, then timed --reps times: wall clock around the call(s) and the library's device-event time
(mrc_get_nmr_ms: H2D, unpack, source analysis, NMR kernels + D2H).  Writes the JSON to --out.
usage: python tools/nmr_bench.py [--hops 65536] [--reps 5] [--out profiles/nmr_bench.json]
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
from mrcaudiocodec_amd import Handle, pacfile, transient      # noqa: E402
from single_stream_bench import make_stream                   # noqa: E402

RATES = (1.5, 2.86, 4.0, 8.0)
PARTS = ("h2d", "unpack", "source_analysis", "nmr_and_d2h")


def spread(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice-hops", type=int, default=256)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--only-one-file", action="store_true", help="(profiling) one warm-up and one timed one-file call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    pcm = make_stream(a.hops, 37)
    shapes = transient.block_shape_array(h, pcm)
    last = np.nonzero(shapes[:, 2] == 1024)[0][-1]
    shapes = shapes[:last + 1]
    ns = int(shapes[:, 2].sum())
    src = np.ascontiguousarray(pcm[:, 1024:])                     # the WAV's own samples (no prior hop)
    files = pacfile.encode_stream_ladder(h, pcm, shapes, RATES, num_samples=ns)
    report = {"what": "mrc_pac_nmr host to host (bytes + int16 source in, summaries out); wall ms around the call(s), device "
                      "ms from mrc_get_nmr_ms (h2d, unpack, source analysis, NMR kernels + d2h; summed over separate calls); "
                      "median / min / max over reps after one warm-up",
              "workload": "ONE stereo stream of %d hops, %d blocks (%d short / transition), encoded by the chained call" %
                          (a.hops, len(shapes), int((shapes[:, 1] + shapes[:, 2] != 2048).sum())),
              "reps": a.reps, "rates": list(RATES), "pac_bytes": [len(f) for f in files]}
    if a.only_one_file:
        h.pac_nmr(files[1], src)
        h.pac_nmr(files[1], src)
        print(json.dumps({"one_file_device_ms": dict(zip(PARTS, map(float, h.nmr_ms())))}), flush=True)
        h.close()
        return

    # the chained encode of the same stream at 2.86, for scale
    enc = lambda: h.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], num_samples=[ns])
    enc()
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        enc()
        walls.append((time.perf_counter() - t0) * 1e3)
    report["chained_encode_2.86"] = {"wall_ms": spread(walls)}

    def case(fn, n_calls):
        walls, dev, out = [], [], None
        fn()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, ms = fn()
            walls.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms)
        dev = np.array(dev)
        return out, {"calls": n_calls, "wall_ms": spread(walls),
                     "device_ms": {k: spread(list(dev[:, i])) for i, k in enumerate(PARTS)}}

    def one():
        r = h.pac_nmr(files[1], src)
        return r, h.nmr_ms()

    def ladder_one():
        r = h.pac_nmr(files, [src] * len(files))
        return r, h.nmr_ms()

    def ladder_four():
        rs, ms = [], np.zeros(4)
        for f in files:
            rs += h.pac_nmr(f, src)
            ms += h.nmr_ms()
        return rs, ms

    r1, report["one_file"] = case(one, 1)
    report["one_file"]["result"] = r1[0]
    report["one_file"]["wall_over_chained_encode"] = round(report["one_file"]["wall_ms"]["median"] /
                                                          report["chained_encode_2.86"]["wall_ms"]["median"], 4)
    print(json.dumps({"one_file": report["one_file"]}), flush=True)
    rl, report["ladder_one_call"] = case(ladder_one, 1)
    report["ladder_one_call"]["results"] = rl
    r4, report["ladder_4_calls"] = case(ladder_four, 4)
    report["ladder_results_equal"] = all(x == y for x, y in zip(rl, r4)) and rl[1] == r1[0]
    print(json.dumps({k: report[k] for k in ("ladder_one_call", "ladder_4_calls", "ladder_results_equal")}), flush=True)

    if not a.skip_numpy:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import nmr_restatement as nr
        sub_shapes = shapes[:np.nonzero(np.cumsum(shapes[:, 1]) >= a.slice_hops * 1024)[0][0]]
        last = np.nonzero(sub_shapes[:, 2] == 1024)[0][-1]
        sub_shapes = sub_shapes[:last + 1]
        n_sub = int(sub_shapes[:, 2].sum())
        sub_pcm = np.ascontiguousarray(pcm[:, :n_sub + 1024])
        buf = pacfile.encode_stereo_stream(h, sub_pcm, sub_shapes, num_samples=n_sub)
        t0 = time.perf_counter()
        want = nr.restate(buf, sub_pcm[:, 1024:])
        sec = time.perf_counter() - t0
        got = h.pac_nmr(buf, np.ascontiguousarray(sub_pcm[:, 1024:]))[0]
        report["numpy_restatement"] = {"hops": a.slice_hops, "blocks": int(want["n_blocks"]), "seconds": round(sec, 3),
                                       "ms_per_hop": round(sec * 1e3 / a.slice_hops, 3),
                                       "nmr_total_db_numpy": want["nmr_total_db"], "nmr_total_db_gpu": got["nmr_total_db"]}
        print(json.dumps({"numpy_restatement": report["numpy_restatement"]}), flush=True)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
