"""
Random one-second crops of resident `.pac` files as a float32 tensor on the device, two ways on an MI355X, in the same run:
  store    PacStore.decode_window (mrc_pac_store_decode_window): the files uploaded once, a call parses and synthesises only
           the blocks its crops overlap and writes [crop][channel][time] where it is wanted;
  files    the only route without the store: Handle.decode_pac_pcm16 of the files (whole files, host to host), the crops
           sliced on the host, torch.from_numpy(...).to(device).
Workloads:
  streams  256 stereo streams of 600 hops (synth.c3_stereo, a seed pair per stream), encoded by the chained stream-mode call
  single   the 65 536-hop stereo stream of tools/single_stream_bench.py (bursts every 37 hops)
Per workload: wall seconds of both routes (median of the timed repeats after a warm-up; the files route split into decode,
slice and upload), the device time of the store's call by phase and its stats, the device time of the whole-file decode, the
store's upload (once) and whether the two routes agree (the int16 crops, array_equal).
One workload per process, each under its own time limit, the second only if the first ended well:
  timeout -k 10 900 python tools/store_bench.py --workload streams --out profiles/store_bench.json && \\
  timeout -k 10 900 python tools/store_bench.py --workload single --out profiles/store_bench.json
(a run adds its workload to the file and keeps the other's).
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
from mrcaudiocodec_amd import ChainSchedule, Handle, synth                           # noqa: E402
from mrcaudiocodec_amd.store import PacStore                                          # noqa: E402
from decode_bench import single_stream_file, timed                                    # noqa: E402

HOP = 1024


def synth_stream_files(h, n_streams, hops):
    pcm = np.zeros((n_streams, 2, (hops + 1) * HOP), np.int16)
    for s in range(n_streams):
        pcm[s] = np.rint(synth.c3_stereo(hops, seed_l=1000 + 2 * s, seed_r=1001 + 2 * s) * 32767.5).clip(-32767, 32767)
    pcm[:, :, :HOP] = 0
    one = np.array([(i * HOP, HOP, HOP) for i in range(hops)], dtype=np.int64)
    r = h.encode_chained_pac(np.ascontiguousarray(pcm[:, 0]), np.ascontiguousarray(pcm[:, 1]), ChainSchedule([one] * n_streams),
                             num_samples=np.full(n_streams, hops * HOP, dtype=np.uint32))
    data, offs = r["bytes"], r["stream_offset"]
    return [data[offs[s]:offs[s + 1]].tobytes() for s in range(n_streams)], \
        "%d stereo files x %d chained joint long blocks + Close() (synth.c3_stereo)" % (n_streams, hops)


def files_route(h, files, which, starts, window, dev, parts):
    import torch
    t0 = time.perf_counter()
    whole = h.decode_pac_pcm16(files, interleaved=False)                 # [nCh][samples] per file
    t1 = time.perf_counter()
    batch = np.empty((len(which), whole[0].shape[0], window), np.int16)
    for k, (f, s) in enumerate(zip(which, starts)):
        batch[k] = whole[f][:, s:s + window]
    t2 = time.perf_counter()
    out = torch.from_numpy(batch).to(dev)
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    parts.append((t1 - t0, t2 - t1, t3 - t2))
    return out


def run(h, files, what, crops, window, reps, files_reps):
    import torch
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    store = PacStore(h, files)
    t_upload = time.perf_counter() - t0
    rng = np.random.default_rng(17)
    which = rng.integers(0, len(files), crops)
    starts = (rng.random(crops) * (store.n_samples[which] - window)).astype(np.int64)      # wholly inside their files
    out = torch.empty((crops, 2, window), dtype=torch.float32, device=dev)

    def crop_call():
        store.decode_window(which, starts, window, channels=2, dtype=torch.float32, out=out)
        return store.stats()
    t_store, ts_store, st = timed(crop_call, reps)
    res = {"workload": what, "files": len(files), "pac_bytes": int(sum(len(f) for f in files)),
           "samples_per_channel": int(store.n_samples.sum()), "crops": crops, "window": window,
           "store": {"upload_seconds_once": round(t_upload, 4), "device_bytes": int(store.device_bytes),
                     "seconds_wall": round(t_store, 5), "seconds_all": [round(t, 5) for t in ts_store],
                     "device_ms": {k: round(v, 3) for k, v in st["ms"].items()},
                     "device_ms_total": round(sum(st["ms"].values()), 3),
                     "stats": {k: v for k, v in st.items() if k != "ms"}}}
    if files_reps > 0:
        parts = []
        t_files, ts_files, got = timed(lambda: files_route(h, files, which, starts, window, dev, parts), files_reps)
        ms = h.decode_ms()
        mid = np.median(np.array(parts[1:]), axis=0)
        res["files_route"] = {"seconds_wall": round(t_files, 5), "seconds_all": [round(t, 5) for t in ts_files],
                              "seconds_decode_slice_upload": [round(float(v), 5) for v in mid],
                              "decode_device_ms": {"h2d": round(float(ms[0]), 3), "unpack": round(float(ms[1]), 3),
                                                   "synthesis": round(float(ms[2]), 3), "d2h": round(float(ms[3]), 3)},
                              "decode_device_ms_total": round(float(ms.sum()), 3)}
        res["speedup_wall"] = round(t_files / t_store, 2)
        codes = store.decode_window(which, starts, window, channels=2, dtype=torch.int16)
        res["array_equal"] = bool(torch.equal(codes, got))
    store.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="streams", choices=("streams", "single"))
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-hops", type=int, default=600)
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--period", type=int, default=37)
    ap.add_argument("--crops", type=int, default=8192)
    ap.add_argument("--window", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--files-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    if a.workload == "streams":
        files, what = synth_stream_files(h, a.streams, a.stream_hops)
    else:
        files, what = single_stream_file(h, a.hops, a.period)
    res = run(h, files, what, a.crops, a.window, a.reps, a.files_reps)
    h.close()
    print(json.dumps({a.workload: res}), flush=True)
    if a.out:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out["tool"] = "tools/store_bench.py"
        out.setdefault("args", {})[a.workload] = {k: v for k, v in vars(a).items() if k != "out"}
        out[a.workload] = res
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
