"""
Rate ladder: one chained call at R bit rates (mrc_encode_chained_ladder_pac) against R one-rate chained calls
(mrc_encode_chained_stream_pac on one handle per rate), host int16 PCM in, .pac bytes out.
  (a) single_stream: ONE stereo stream of --hops hops (tools/single_stream_bench.make_stream: noise floor + tone, a burst
      every 37th hop; shapes from the transient detector) at R = 1, 2, 4, 8;
  (b) stream_mode:   8192 stereo streams x 12 long blocks + Close() at R = 4.
Every case is warmed up once, then timed --reps times: wall clock around the call(s) and the library's device-event time
(mrc_get_chain_ms: phase A + prep, serial scan, pack, whole call), summed over the separate calls.  Reports median, min and
max, checks the ladder's bytes against the separate calls', and writes the JSON to --out.
usage: python tools/ladder_bench.py [--hops 65536] [--reps 5] [--out profiles/ladder_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mrcaudiocodec_amd import Handle, transient      # noqa: E402
from single_stream_bench import make_stream           # noqa: E402

LADDER = (1.0, 2.0, 2.86, 4.0, 1.5, 3.5, 5.0, 6.5)


def spread(v):
    v = sorted(v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def run_case(handles, ladder_h, left, right, shapes, rates, reps, num_samples):
    kw = dict(num_samples=num_samples)

    def separate():
        t0 = time.perf_counter()
        outs, ms = [], np.zeros(4)
        for r in rates:
            outs.append(handles[r].encode_chained_pac(left, right, shapes, **kw))
            ms += handles[r].chain_ms()
        return time.perf_counter() - t0, ms, outs

    def ladder():
        t0 = time.perf_counter()
        outs = ladder_h.encode_chained_pac_ladder(left, right, shapes, rates, **kw)
        return time.perf_counter() - t0, ladder_h.chain_ms(), outs

    res = {}
    for name, fn in (("separate_calls", separate), ("ladder", ladder)):
        fn()                                                       # warm-up: buffers grown, code loaded
        walls, dev = [], []
        for _ in range(reps):
            w, ms, outs = fn()
            walls.append(w * 1e3)
            dev.append(ms)
        dev = np.array(dev)
        res[name] = {"wall_ms": spread(walls), "device_ms": {k: spread(list(dev[:, i])) for i, k in
                                                             enumerate(("phase_a_and_prep", "serial_scan", "pack", "whole"))}}
        res[name]["_outs"] = outs
    sep, lad = res["separate_calls"].pop("_outs"), res["ladder"].pop("_outs")
    res["bytes_equal"] = all(a["bytes"].tobytes() == b["bytes"].tobytes() and np.array_equal(a["stream_offset"], b["stream_offset"])
                             and np.array_equal(a["reservoir_out"], b["reservoir_out"]) for a, b in zip(sep, lad))
    res["pac_bytes"] = [int(o["total"]) for o in lad]
    res["wall_ratio_ladder_over_separate"] = round(res["ladder"]["wall_ms"]["median"] / res["separate_calls"]["wall_ms"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    handles = {r: Handle(device_id=0, target_bits_per_sample=r) for r in LADDER}
    ladder_h = Handle(device_id=0)
    report = {"what": "rate ladder (one mrc_encode_chained_ladder_pac call) vs one mrc_encode_chained_stream_pac call per rate; "
                      "host int16 PCM -> host .pac bytes; wall ms around the call(s), device ms from mrc_get_chain_ms (summed "
                      "over the separate calls); median / min / max over reps after one warm-up", "reps": a.reps}
    # (a) single stream
    pcm = make_stream(a.hops, 37)
    shapes = transient.block_shape_array(ladder_h, pcm)
    last = np.nonzero(shapes[:, 2] == 1024)[0][-1]
    shapes = shapes[:last + 1]
    ns = [int(shapes[:, 2].sum())]
    single = {"workload": "ONE stereo stream of %d hops, %d blocks (%d short / transition)" %
                          (a.hops, len(shapes), int((shapes[:, 1] + shapes[:, 2] != 2048).sum()))}
    for R in (1, 2, 4, 8):
        rates = LADDER[:R]
        single["R=%d" % R] = dict(rates=list(rates), **run_case(handles, ladder_h, pcm[0][None], pcm[1][None], [shapes], rates,
                                                                  a.reps, ns))
        single["R=%d" % R]["ladder_scan_us_per_block"] = round(single["R=%d" % R]["ladder"]["device_ms"]["serial_scan"]["median"]
                                                                * 1e3 / len(shapes), 4)
        print(json.dumps({("single_stream R=%d" % R): {k: v for k, v in single["R=%d" % R].items()}}), flush=True)
    report["single_stream"] = single
    # (b) stream mode
    rng = np.random.default_rng(5)
    nS, nB = a.streams, 12
    left = np.zeros((nS, (nB + 1) * 1024), np.int16)
    right = np.zeros((nS, (nB + 1) * 1024), np.int16)
    left[:, 1024:] = np.clip(np.rint(rng.normal(0, 0.1 * 32767, (nS, nB * 1024))), -32767, 32767)
    right[:, 1024:] = np.clip(np.rint(0.6 * left[:, 1024:] + rng.normal(0, 0.05 * 32767, (nS, nB * 1024))), -32767, 32767)
    sh = np.stack([np.arange(nB, dtype=np.int64) * 1024, np.full(nB, 1024, np.int64), np.full(nB, 1024, np.int64)], axis=1)
    rates = LADDER[:4]
    report["stream_mode"] = dict(workload="%d stereo streams x %d long blocks + Close()" % (nS, nB), rates=list(rates),
                                 **run_case(handles, ladder_h, left, right, [sh] * nS, rates, a.reps, [nB * 1024] * nS))
    print(json.dumps({"stream_mode R=4": report["stream_mode"]}), flush=True)
    for hd in list(handles.values()) + [ladder_h]:
        hd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
