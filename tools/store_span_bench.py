"""
Rows of pieces and placed events from resident 48 kHz `.pac` files as float32 tensors on an MI355X, on the `streams` corpus of
tools/store_reduced_bench.py (256 stereo streams of 600 hops), at 16 kHz mid (rate_divisor=2, resample=(2, 3), mix="mid").  In
each workload two routes take turns in one process, call after call, so that neither has the device to itself at another moment
than the other:
  concat   8192 rows of 4 s, each of eight 0.5 s pieces of random files at random places.
           spans   PacStore.decode_window_sum(span_first=, span_len=): one call of 8 terms per row (store.concat_spans)
           calls   what a user did before: eight PacStore.decode_window calls of 0.5 s, one per piece position, and torch.cat
  event    8192 rows of 4 s of background with a 0.5 s event from the middle of another file at a drawn place, faded over 5 ms.
           spans   one call of two terms, the event's span its 0.5 s
           today   PacStore.decode_window_sum of the same two terms without spans: it CANNOT crop the event, which plays on to
                   the end of the row (another signal), and its file is parsed and synthesised under the whole window -- recorded
                   as what it is, the cost of the nearest thing the existing call can do
After a warm-up round, per route the median over the timed rounds of the wall seconds of the whole route with the interquartile
range, the device time of the stages (PacStore.stats(), summed over a route's calls; the torch.cat alone by events), chunks
parsed, slabs and the peak of torch.cuda.max_memory_allocated.  Checked from the statistics, not the clock: in `concat` the one
call parses no more chunks than the eight calls together; in `event` the event terms' chunks are those of 0.5 s windows, not of
4 s ones (the event terms alone through each).  No ratio is decided in advance: the JSON holds what was measured.
  timeout -k 10 900 python tools/store_span_bench.py --out profiles/store_span_bench.json
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
from mrcaudiocodec_amd.store import MS_NAMES, PacStore, concat_spans                  # noqa: E402
from store_bench import synth_stream_files                                            # noqa: E402

KW = dict(rate_divisor=2, mix="mid", resample=(2, 3))
WINDOW, PIECE, PIECES, FADE = 64000, 8000, 8, 80


def timed(routes, reps):
    """routes: [(name, fn -> (list of stats dicts, torch ms or None))] taking turns -> per route the record"""
    import torch
    dev = torch.device("cuda", 0)
    for _, fn in routes:                                             # warm-up round: workspaces, the filter's upload, torch's kernels
        fn()
    wall, sts, peak, extra = ({r: [] for r, _ in routes} for _ in range(4))
    for _ in range(reps):
        for r, fn in routes:
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            st, torch_ms = fn()
            wall[r].append(time.perf_counter() - t0)
            peak[r].append(torch.cuda.max_memory_allocated(dev) - before)
            sts[r].append(st)
            extra[r].append(0.0 if torch_ms is None else torch_ms)
    out = {}
    for r, _ in routes:
        ms = {k: round(float(np.median([sum(s["ms"][k] for s in call) for call in sts[r]])), 3) for k in MS_NAMES}
        last = sts[r][-1]
        q25, q75 = np.percentile(wall[r], [25, 75])
        out[r] = {"seconds_wall": round(float(np.median(wall[r])), 5), "seconds_all": [round(v, 5) for v in wall[r]],
                  "spread_seconds": {"interquartile": round(float(q75 - q25), 5), "range": round(float(max(wall[r]) - min(wall[r])), 5)},
                  "device_ms": ms, "torch_device_ms": round(float(np.median(extra[r])), 3),
                  "device_ms_total": round(sum(ms.values()) + float(np.median(extra[r])), 3), "library_calls": len(last),
                  "peak_torch_bytes": int(np.median(peak[r])), "stats": {k: sum(s[k] for s in last) for k in last[0] if k != "ms"}}
    return out


def run_concat(store, rows, reps):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    n = np.asarray(store.n_samples_resampled(2, 3, 2), np.int64)
    files = rng.integers(0, len(store), (rows, PIECES))
    src = (rng.random((rows, PIECES)) * (n[files] - PIECE)).astype(np.int64)
    starts, first, length, fin, fout = concat_spans(np.full((rows, PIECES), PIECE), src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kept = {}

    def route_spans():
        out = store.decode_window_sum(files, starts, np.ones((rows, PIECES)), WINDOW, dtype=torch.float32, span_first=first, span_len=length, **KW)
        kept["spans"] = out[:64].clone()
        return [store.stats()], None

    def route_calls():
        parts, sts = [], []
        for j in range(PIECES):
            parts.append(store.decode_window(files[:, j], src[:, j], PIECE, dtype=torch.float32, **KW))
            sts.append(store.stats())
        ev[0].record()
        out = torch.cat(parts, dim=2)
        ev[1].record()
        torch.cuda.synchronize(dev)
        kept["calls"] = out[:64].clone()
        return sts, ev[0].elapsed_time(ev[1])

    res = {"rows": rows, "window": WINDOW, "pieces": PIECES, "piece": PIECE, "arguments": dict(KW, resample=list(KW["resample"])),
           "rounds_timed": reps, "routes": timed((("spans", route_spans), ("calls", route_calls)), reps)}
    s, c = res["routes"]["spans"], res["routes"]["calls"]
    res["equal_64_rows"] = bool(torch.equal(kept["spans"], kept["calls"]))
    res["spans_parses_no_more_chunks_than_the_eight_calls"] = bool(s["stats"]["chunks_parsed"] <= c["stats"]["chunks_parsed"])
    res["calls_wall_over_spans_wall"] = round(c["seconds_wall"] / s["seconds_wall"], 3)
    print("concat: spans %.5f s, calls %.5f s; chunks %d vs %d; slabs %d vs %d; peak %d vs %d MiB; equal %s" % (
        s["seconds_wall"], c["seconds_wall"], s["stats"]["chunks_parsed"], c["stats"]["chunks_parsed"], s["stats"]["slabs"], c["stats"]["slabs"],
        s["peak_torch_bytes"] >> 20, c["peak_torch_bytes"] >> 20, res["equal_64_rows"]), flush=True)
    return res


def run_event(store, rows, reps):
    import torch
    rng = np.random.default_rng(37)
    n = np.asarray(store.n_samples_resampled(2, 3, 2), np.int64)
    back = rng.integers(0, len(store), rows)
    event = (back + 1 + rng.integers(0, len(store) - 1, rows)) % len(store)
    b_starts = (rng.random(rows) * (n[back] - WINDOW)).astype(np.int64)
    p = n[event] // 2 - PIECE // 2                                   # the event: 0.5 s from the middle of its file
    at = rng.integers(0, WINDOW - PIECE + 1, rows)                   # ... at a drawn place in the row
    gains = np.stack([np.ones(rows), 10.0 ** (rng.uniform(-10.0, 10.0, rows) / 20.0)], 1)
    files, starts = np.stack([back, event], 1), np.stack([b_starts, p - at], 1)
    spans = dict(span_first=np.stack([np.zeros(rows, np.int64), at], 1), span_len=np.stack([np.full(rows, WINDOW), np.full(rows, PIECE)], 1),
                 fade_in=np.stack([np.zeros(rows, np.int64), np.full(rows, FADE)], 1), fade_out=np.stack([np.zeros(rows, np.int64), np.full(rows, FADE)], 1))

    def route_spans():
        store.decode_window_sum(files, starts, gains, WINDOW, dtype=torch.float32, **spans, **KW)
        return [store.stats()], None

    def route_today():
        store.decode_window_sum(files, starts, gains, WINDOW, dtype=torch.float32, **KW)
        return [store.stats()], None

    res = {"rows": rows, "window": WINDOW, "event": PIECE, "fade": FADE, "arguments": dict(KW, resample=list(KW["resample"])),
           "rounds_timed": reps, "routes": timed((("spans", route_spans), ("today", route_today)), reps)}
    # the event terms alone: through the spans call, through 0.5 s windows and through 4 s windows
    one = np.arange(rows + 1)
    store.decode_window_sum(event, p - at, np.ones(rows), WINDOW, item_offsets=one, dtype=torch.float32, span_first=at,
                            span_len=np.full(rows, PIECE), **KW)
    chunks_spans = store.stats()["chunks_parsed"]
    store.decode_window(event, p, PIECE, dtype=torch.float32, **KW)
    chunks_half = store.stats()["chunks_parsed"]
    store.decode_window(event, p - at, WINDOW, dtype=torch.float32, **KW)
    chunks_whole = store.stats()["chunks_parsed"]
    res["event_terms_chunks"] = {"spans_call": chunks_spans, "half_second_windows": chunks_half, "four_second_windows": chunks_whole}
    res["event_terms_chunks_are_those_of_half_a_second"] = bool(chunks_spans == chunks_half < chunks_whole)
    s, t = res["routes"]["spans"], res["routes"]["today"]
    res["today_wall_over_spans_wall"] = round(t["seconds_wall"] / s["seconds_wall"], 3)
    print("event: spans %.5f s, today's uncropped call %.5f s; chunks %d vs %d (event terms alone: %d, 0.5 s windows %d, 4 s windows %d)" % (
        s["seconds_wall"], t["seconds_wall"], s["stats"]["chunks_parsed"], t["stats"]["chunks_parsed"], chunks_spans, chunks_half, chunks_whole),
        flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 1 or a.streams < 2 or a.rows < 64:
        ap.error("--reps at least 1, --streams at least 2, --rows at least 64")
    h = Handle(device_id=0)
    files, what = synth_stream_files(h, a.streams, a.stream_hops)
    store = PacStore(h, files)
    res = {"workload": what, "files": len(files), "concat": run_concat(store, a.rows, a.reps), "event": run_event(store, a.rows, a.reps)}
    store.close()
    h.close()
    print(json.dumps(res), flush=True)
    if a.out:
        out = {"tool": "tools/store_span_bench.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "streams": res}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if not (res["concat"]["spans_parses_no_more_chunks_than_the_eight_calls"] and res["event"]["event_terms_chunks_are_those_of_half_a_second"]
            and res["concat"]["equal_64_rows"]):
        raise SystemExit("store_span_bench: a check on the statistics failed, see the JSON")


if __name__ == "__main__":
    main()
