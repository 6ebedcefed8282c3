"""
`.pac` -> 16-bit PCM, host to host, two ways on an MI355X:
  present  pacfile.decode_pac_pcm16 per file (C++ chunk parser on host threads, fixed-stride arrays uploaded per block
           shape, decode_kernel per shape, planar int16 back) + the host transpose to WAV order that cli.wav_bytes does;
  device   Handle.decode_pac_pcm16 on all files in ONE call (mrc_decode_pac_pcm16: bytes cross PCIe once, chunk parsing,
           Huffman decoding, synthesis and the interleaved codes on the device).
Workloads:
  single   the 65 536-hop stereo stream of tools/single_stream_bench.py (bursts every 37 hops), encoded once by the chained call
  streams  the encoder's stream-mode set (as bench.py's stream_mode_leg builds it): 8 192 stereo files x 12 long blocks + Close()
Reports per workload: Msamples/s host to host (median of the timed repeats after a warm-up), the device split of the new call
(mrc_get_decode_ms), the share of chunks per Huffman table, and whether the timed outputs of both paths are array_equal.
usage: python tools/decode_bench.py [--workloads single,streams] [--reps 5] [--present-reps 2] [--out file.json]
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
from mrcaudiocodec_amd import ChainSchedule, Handle, pacfile, synth, transient      # noqa: E402
from single_stream_bench import make_stream                                          # noqa: E402

HOP = 1024


def single_stream_file(h, hops, period):
    pcm = make_stream(hops, period)
    shapes = transient.block_shapes(h, synth.pcm_to_float(pcm))
    while shapes and shapes[-1][2] != HOP:
        shapes.pop()
    r = h.encode_chained_pac(pcm[0][None], pcm[1][None], [shapes], num_samples=[sum(b for (_, _, b) in shapes)])
    n_switched = sum(1 for (_, a, b) in shapes if a + b != 2 * HOP)
    return [r["bytes"].tobytes()], "one stereo stream, %d hops, %d blocks (%d short / transition) + Close()" % (
        hops, len(shapes), n_switched)


def stream_mode_files(h, n_streams, n_blocks):
    import torch
    dev = torch.device("cuda", 0)
    gs = torch.Generator(device=dev)
    gs.manual_seed(7)                                            # bench.py stream_mode_leg's content
    pl = torch.clamp(torch.round(torch.randn((n_streams, (n_blocks + 1) * HOP), generator=gs, device=dev,
                                             dtype=torch.float64) * 3000), -32767, 32767)
    pl[:, :HOP] = 0
    pr = torch.clamp(torch.round(0.7 * pl + 0.3 * torch.roll(pl, 17, dims=1)), -32767, 32767)
    pr[:, :HOP] = 0
    pl, pr = pl.to(torch.int16).cpu().numpy(), pr.to(torch.int16).cpu().numpy()
    one = np.array([(i * HOP, HOP, HOP) for i in range(n_blocks)], dtype=np.int64)
    r = h.encode_chained_pac(pl, pr, ChainSchedule([one] * n_streams),
                             num_samples=np.full(n_streams, n_blocks * HOP, dtype=np.uint32))
    data, offs = r["bytes"], r["stream_offset"]
    return [data[offs[s]:offs[s + 1]].tobytes() for s in range(n_streams)], \
        "%d stereo files x %d chained joint long blocks + Close()" % (n_streams, n_blocks)


def table_shares(files):
    counts = {}
    for f in files:
        _, _, _, off = pacfile.read_header(f)
        raw = np.frombuffer(f, np.uint8)
        for c in pacfile.scan_chunks(f, off):
            t = int(raw[c + 4]) >> 4
            counts[t] = counts.get(t, 0) + 1
    total = sum(counts.values())
    name = {0: "percussive", 1: "silence", 2: "speech", 3: "tonal", 15: "raw"}
    return {"chunks": total, "share": {name.get(t, str(t)): round(n / total, 4) for t, n in sorted(counts.items())}}


def present_path(h, files):
    return [np.ascontiguousarray(pacfile.decode_pac_pcm16(h, f).T) for f in files]     # + cli.wav_bytes' transpose


def timed(fn, reps, warm=None):
    (warm or fn)()                                               # warm-up: buffers, shapes
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, out


def run(h, name, files, what, reps, present_reps):
    t_dev, ts_dev, got = timed(lambda: h.decode_pac_pcm16(files), reps)
    ms = h.decode_ms()
    n_values = sum(g.size for g in got)
    res = {"workload": what, "files": len(files), "pac_bytes": sum(len(f) for f in files), "pcm_values": n_values,
           "huffman_tables": table_shares(files),
           "device_call": {"seconds_host_to_host": round(t_dev, 5), "seconds_all": [round(t, 5) for t in ts_dev],
                           "Msamples_s": round(n_values / t_dev / 1e6, 2),
                           "device_ms": {"h2d": round(float(ms[0]), 3), "unpack": round(float(ms[1]), 3),
                                         "synthesis": round(float(ms[2]), 3), "d2h": round(float(ms[3]), 3)}}}
    if present_reps > 0:
        t_old, ts_old, want = timed(lambda: present_path(h, files), present_reps, lambda: present_path(h, files[:4]))
        res["present_path"] = {"seconds_host_to_host": round(t_old, 5), "seconds_all": [round(t, 5) for t in ts_old],
                               "Msamples_s": round(n_values / t_old / 1e6, 2)}
        res["speedup"] = round(t_old / t_dev, 2)
        res["array_equal"] = bool(len(want) == len(got) and all(np.array_equal(a, b) for a, b in zip(want, got)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="single,streams")
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--period", type=int, default=37)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--present-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h = Handle(device_id=0)
    out = {"tool": "tools/decode_bench.py",          # what was measured (where the result is written is not part of it)
           "args": {k: v for k, v in vars(a).items() if k != "out"}}
    for w in a.workloads.split(","):
        t0 = time.perf_counter()
        if w == "single":
            files, what = single_stream_file(h, a.hops, a.period)
        elif w == "streams":
            files, what = stream_mode_files(h, a.streams, a.blocks)
        else:
            raise SystemExit("unknown workload %r" % w)
        t_enc = time.perf_counter() - t0
        out[w] = run(h, w, files, what, a.reps, a.present_reps)
        out[w]["encode_seconds"] = round(t_enc, 2)
        print(json.dumps({w: out[w]}), flush=True)
    h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
