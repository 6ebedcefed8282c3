"""
Mono `.pac` encoding measured on the GPU box (the chained call with pcm_right == NULL):
  single   ONE mono stream of `--hops` hops with bursts, block shapes from the transient detector: the one chained call,
           resident (mrc_dev_encode_chained_pac) and host to host (mrc_encode_chained_stream_pcm16_pac), against the
           block-at-a-time loop (pacfile.encode_mono_stream_per_block) on a prefix of `--loop-blocks` blocks;
  many     `--streams` mono files of `--blocks` long blocks each (+ Close()) in one resident call;
  with mrc_get_chain_ms's split (phase A + preparation / serial scan / packing) for each chained leg.
usage: python tools/mono_bench.py [--hops 65536] [--loop-blocks 256] [--streams 8192] [--blocks 12] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrcaudiocodec_amd import ChainSchedule, Handle, pacfile, synth, transient      # noqa: E402
from mrcaudiocodec_amd.batch import StreamEncoder                                  # noqa: E402

HOP = 1024


def make_stream(hops, period, seed=42):
    """mono int16 [1][(hops+1)*1024]: noise floor + tone, a burst of 128 samples every `period`-th hop."""
    rng = np.random.default_rng(seed)
    n = hops * HOP
    x = rng.normal(0.0, 0.02 * 32767, n) + 0.2 * 32767 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 48000)
    for h in range(period - 1, hops, period):
        x[h * HOP:h * HOP + 128] = rng.normal(0.0, 0.5 * 32767, 128)
    pcm = np.zeros((1, (hops + 1) * HOP), np.int16)
    pcm[0, HOP:] = np.clip(np.rint(x), -32767, 32767)
    return pcm


def split(ms):
    return {"phase_a_and_prep": round(float(ms[0]), 3), "serial_scan": round(float(ms[1]), 3), "pack": round(float(ms[2]), 3),
            "all": round(float(ms[3]), 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=65536)
    ap.add_argument("--loop-blocks", type=int, default=256)
    ap.add_argument("--period", type=int, default=37)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    h = Handle(device_id=0)
    enc = StreamEncoder(handle=h)
    dev = enc.device
    # ---- one long stream
    pcm = make_stream(a.hops, a.period)
    t0 = time.perf_counter()
    shapes = transient.block_shape_array(h, pcm)
    t_det = time.perf_counter() - t0
    last = len(shapes)
    while last > 0 and shapes[last - 1, 2] != HOP:
        last -= 1
    shapes = shapes[:last]
    n_short = int((shapes[:, 1] + shapes[:, 2] != 2 * HOP).sum())
    samples = float(shapes[:, 2].sum())
    # before: the per-block loop on a prefix ending with a long block
    k = min(a.loop_blocks, len(shapes))
    while k > 1 and shapes[k - 1, 2] != HOP:
        k -= 1
    pre = [tuple(v) for v in shapes[:k].tolist()]
    x = synth.pcm_to_float(pcm[0])
    pacfile.encode_mono_stream_per_block(h, x, pre[:1])                                  # warm-up
    t0 = time.perf_counter()
    ref = pacfile.encode_mono_stream_per_block(h, x, pre)
    t_loop = time.perf_counter() - t0
    loop_samples = float(sum(b for (_, _, b) in pre))
    same = h.encode_chained_pac(pcm, None, [pre], num_samples=[int(loop_samples)])["bytes"].tobytes() == ref
    # after, host to host
    best = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = h.encode_chained_pac(pcm, None, [shapes], num_samples=[int(samples)])
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, h.chain_ms(), r["total"])
    dt_host, ms_host, total = best
    # after, resident
    t = torch.from_numpy(pcm).to(dev)
    sched = ChainSchedule([shapes])
    r = enc.encode_chained_pac(t, None, sched, num_samples=[int(samples)])
    out_buf = torch.empty((int(r["total"]) + 4096,), dtype=torch.uint8, device=dev)
    res_same = r["bytes"].cpu().numpy().tobytes() == h.encode_chained_pac(pcm, None, [shapes], num_samples=[int(samples)])["bytes"].tobytes()
    best = None
    for _ in range(a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        enc.encode_chained_pac(t, None, sched, num_samples=[int(samples)], out=out_buf)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, h.chain_ms())
    dt_res, ms_res = best
    loop_rate = loop_samples / t_loop / 1e6
    single = {
        "workload": "one mono 48 kHz stream, %d hops, burst every %d hops; %d blocks (%d short / transition) from the "
                    "transient detector" % (a.hops, a.period, len(shapes), n_short),
        "before_per_block_loop": {"blocks": len(pre), "ms_per_block": round(1e3 * t_loop / len(pre), 4),
                                  "Msamples_s": round(loop_rate, 3)},
        "after_chained_resident": {"seconds": round(dt_res, 5), "Msamples_s": round(samples / dt_res / 1e6, 3),
                                   "device_ms": split(ms_res),
                                   "serial_scan_us_per_item": round(1e3 * float(ms_res[1]) / (len(shapes) + 1), 3)},
        "after_chained_host_to_host": {"seconds": round(dt_host, 5), "Msamples_s": round(samples / dt_host / 1e6, 3),
                                       "device_ms": split(ms_host), "pac_bytes": int(total)},
        "speedup_resident_vs_loop": round(samples / dt_res / 1e6 / loop_rate, 1),
        "speedup_host_to_host_vs_loop": round(samples / dt_host / 1e6 / loop_rate, 1),
        "prefix_bytes_equal_per_block_loop": bool(same),
        "resident_bytes_equal_host": bool(res_same),
        "detector_seconds": round(t_det, 4),
    }
    del t, out_buf
    # ---- many short files
    nS, nT = a.streams, a.blocks
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pl = torch.clamp(torch.round(torch.randn((nS, (nT + 1) * HOP), generator=g, device=dev, dtype=torch.float64) * 3000),
                     -32767, 32767)
    pl[:, :HOP] = 0
    ssl = pl.to(torch.int16).contiguous()
    del pl
    one = np.array([(i * HOP, HOP, HOP) for i in range(nT)], dtype=np.int64)
    sched = ChainSchedule([one] * nS)
    ns = np.full(nS, nT * HOP, dtype=np.uint32)
    r = enc.encode_chained_pac(ssl, None, sched, num_samples=ns)                      # warm-up: buffers
    out_buf = torch.empty((int(r["total"]) + 4096,), dtype=torch.uint8, device=dev)
    ts, ms = [], None
    for _ in range(max(3, a.reps)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = enc.encode_chained_pac(ssl, None, sched, num_samples=ns, out=out_buf)
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
        if ms is None or ts[-1] == min(ts):
            ms = h.chain_ms()
    dt = float(np.median(ts))
    many = {"workload": "%d mono streams x %d chained long blocks + Close(), int16 PCM resident in HBM -> complete .pac "
                        "files in HBM" % (nS, nT),
            "Msamples_s": round(nS * nT * HOP / dt / 1e6, 3), "seconds_per_call": round(dt, 5), "device_ms": split(ms),
            "Msamples_s_device_time_only": round(nS * nT * HOP / (float(ms[3]) * 1e-3) / 1e6, 3),
            "pac_bytes_per_block": round(r["total"] / (nS * nT), 1)}
    out = {"single_stream": single, "stream_mode": many}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    h.close()


if __name__ == "__main__":
    main()
