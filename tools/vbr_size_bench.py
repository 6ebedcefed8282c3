"""
Constant-quality VBR to a file size: the one-call search (mrc_encode_vbr_size_pac) against the same bisection driven from
Python over mrc_encode_vbr_nmr_pac -- the only way to get it before the call existed -- in one process, on the same grid and
targets, host to host.
  single   ONE stereo stream of --hops hops (tools/single_stream_bench.make_stream);
  batch    --streams stereo streams of --batch-hops long blocks each, the same content at a gain per stream.
The target of every stream is --bits-per-sample as bytes (cli.vbr_size_target_bytes).  Routes, interleaved in every repetition:
  one_call     Handle.encode_vbr_size_pac, with mrc_get_vbr_size_ms (phase A + source analysis, profile, probes, final pick +
               pack, sum) and the probe counts;
  python_loop  pacfile.bisect_ceiling's rule with Handle.encode_vbr_nmr_pac as bytes(i): per round one call per distinct
               ceiling over the streams that probe it, and the chosen files from the last call that made them.
The two must return identical bytes; the run fails otherwise.  Also: the device time of one vbr_alloc_kernel pass over the
same blocks (mrc_get_vbr_ms of a plain VBR call at the median chosen ceiling) beside the time of one probe round.
Every route is warmed up once, then timed --reps times: wall clock around the route, median / min / max.
usage: python tools/vbr_size_bench.py [--hops 65536] [--streams 8192] [--batch-hops 12] [--reps 5] [--out profiles/vbr_size_bench.json]
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
from mrcaudiocodec_amd import Handle, cli, pacfile, transient  # noqa: E402
from single_stream_bench import make_stream                   # noqa: E402

SIZE_PARTS = ("phase_a_source_analysis", "profile", "probes", "final_pick_pack", "all")


def spread(v):
    v = sorted(float(x) for x in v)
    return {"median": round(float(np.median(v)), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def python_loop(h, left, right, shapes, ns, targets, grid):
    """the rule of pacfile.bisect_ceiling for all streams at once, bytes(i) from the existing call"""
    n_streams = len(shapes)
    db = pacfile.ceiling_grid(*grid)
    lo, hi = np.zeros(n_streams, np.int64), np.full(n_streams, grid[2] - 1, np.int64)
    active = np.ones(n_streams, bool)
    files, at = [None] * n_streams, np.full(n_streams, -1, np.int64)
    calls = 0
    first = True
    while active.any():
        probe = np.where(first, hi, (lo + hi) // 2)
        for i in np.unique(probe[active]):
            sel = np.nonzero(active & (probe == i))[0]
            rs = h.encode_vbr_nmr_pac(left[sel], None if right is None else right[sel], [shapes[s] for s in sel], float(db[i]),
                                      num_samples=[ns[s] for s in sel])
            calls += 1
            for s, r in zip(sel, rs):
                files[s], at[s] = r["data"], i
                fits = len(r["data"]) <= targets[s]
                if first:
                    active[s] = fits
                elif fits:
                    hi[s] = i
                else:
                    lo[s] = i + 1
        first = False
        active &= lo < hi
    for i in np.unique(hi[at != hi]):                                 # the chosen file where the last probe was another
        sel = np.nonzero((at != hi) & (hi == i))[0]
        rs = h.encode_vbr_nmr_pac(left[sel], None if right is None else right[sel], [shapes[s] for s in sel], float(db[i]),
                                  num_samples=[ns[s] for s in sel])
        calls += 1
        for s, r in zip(sel, rs):
            files[s] = r["data"]
    return files, hi, calls


def workload(h, name, left, right, shapes, ns, bps, grid, reps):
    n_streams = len(shapes)
    hdr = len(pacfile.header(h.cfg, 2, ns[0]))
    targets = [cli.vbr_size_target_bytes(bps, hdr, int(sum(int(b) for (_, _, b) in sh)), 2, 2 * (len(sh) + 1)) for sh in shapes]
    keep = {}

    def one_call():
        keep["one"] = h.encode_vbr_size_pac(left, right, shapes, targets, *grid, num_samples=ns)
        return h.vbr_size_ms()

    def loop():
        keep["loop"] = python_loop(h, left, right, shapes, ns, targets, grid)
        return None

    routes = {"one_call": one_call, "python_loop": loop}
    walls, dev = {k: [] for k in routes}, []
    for fn in routes.values():
        fn()                                                          # warm-up
    for _ in range(reps):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            ms = fn()
            walls[k].append((time.perf_counter() - t0) * 1e3)
            if ms is not None:
                dev.append(ms)
    one, (files, chosen, calls) = keep["one"], keep["loop"]
    same = all(r["data"] == f for r, f in zip(one, files)) and [r["chosen"] for r in one] == [int(c) for c in chosen]
    rounds = max(r["probes"] for r in one)
    mid_db = float(np.median([r["chosen_db"] for r in one]))
    h.encode_vbr_nmr_pac(left, right, shapes, mid_db, num_samples=ns)
    alloc_ms = [float(h.encode_vbr_nmr_pac(left, right, shapes, mid_db, num_samples=ns) and h.vbr_ms()[1]) for _ in range(reps)]
    dev = np.array(dev)
    probes_ms = float(np.median(dev[:, 2]))
    rep = {"workload": name, "bits_per_sample_target": bps, "grid_lo_step_n": list(grid), "identical_bytes": bool(same),
           "one_call": {"wall_ms": spread(walls["one_call"]), "device_ms": {k: spread(dev[:, i]) for i, k in enumerate(SIZE_PARTS)},
                        "probe_rounds": int(rounds), "probes_per_stream": spread([r["probes"] for r in one]),
                        "met": int(sum(r["met"] for r in one)), "streams": n_streams,
                        "bytes": int(sum(len(r["data"]) for r in one)), "target_bytes": int(sum(targets)),
                        "chosen_db": spread([r["chosen_db"] for r in one])},
           "python_loop": {"wall_ms": spread(walls["python_loop"]), "library_calls": int(calls)},
           "python_loop_over_one_call": round(float(np.median(walls["python_loop"]) / np.median(walls["one_call"])), 3),
           "probe_round_ms": round(probes_ms / rounds, 4),
           "vbr_alloc_kernel_pass_ms": spread(alloc_ms), "alloc_ceiling_db": mid_db,
           "alloc_pass_over_probe_round": round(float(np.median(alloc_ms)) / (probes_ms / rounds), 3)}
    print(json.dumps({name: rep}), flush=True)
    if not same:
        raise SystemExit("the one-call search and the Python-driven bisection returned different bytes")
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--batch-hops", type=int, default=12)
    ap.add_argument("--bits-per-sample", type=float, default=2.86)
    ap.add_argument("--grid", default="-30:0.25:256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lo, step, n = a.grid.split(":")
    grid = (float(lo), float(step), int(n))
    h = Handle(device_id=0)
    report = {"what": "mrc_encode_vbr_size_pac against the same bisection driven from Python over mrc_encode_vbr_nmr_pac, host to "
                      "host, one process; wall ms around the route, device ms from the library's events; median / min / max over "
                      "reps after one warm-up, routes interleaved", "reps": a.reps}
    pcm = make_stream(a.hops, 37)
    shapes = transient.block_shape_array(h, pcm)
    shapes = shapes[:np.nonzero(shapes[:, 2] == 1024)[0][-1] + 1]
    report["single"] = workload(h, "single: ONE stereo stream of %d hops, %d blocks" % (a.hops, len(shapes)), pcm[0][None], pcm[1][None],
                                [shapes], [int(shapes[:, 2].sum())], a.bits_per_sample, grid, a.reps)
    one = make_stream(a.batch_hops, 1 << 30)                          # (no bursts: long blocks only)
    rng = np.random.default_rng(7)
    L = np.empty((a.streams, one.shape[1]), np.int16)
    R = np.empty((a.streams, one.shape[1]), np.int16)
    for s in range(a.streams):                                        # the same content at a gain per stream
        g = 0.25 + 0.75 * rng.random()
        L[s], R[s] = (one[0] * g).astype(np.int16), (one[1] * g).astype(np.int16)
    bshape = np.array([(i * 1024, 1024, 1024) for i in range(a.batch_hops)], np.int64)
    report["batch"] = workload(h, "batch: %d stereo streams of %d long blocks" % (a.streams, a.batch_hops), L, R,
                               [bshape] * a.streams, [a.batch_hops * 1024] * a.streams, a.bits_per_sample, grid, a.reps)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
