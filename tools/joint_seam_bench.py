"""
The per-block seam: wall time of one mrc_encode_joint call on ONE long joint block (the small-batch path of encode_host,
~0.08 ms per call), where an added HIP call or allocation per encode would show.  200 calls to warm up, then the median,
minimum and maximum over `--batches` batches of `--calls` calls each.  MRC_HIP_LIBRARY selects another build of the
library (mrcaudiocodec_amd/_lib.py), so that two builds can be run alternately.
usage: python tools/joint_seam_bench.py [--batches 15] [--calls 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrcaudiocodec_amd import LIB_PATH, Handle, synth      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    h = Handle()
    s = synth.c3_stereo(2)
    left, right = s[0][None, :2048].copy(), s[1][None, 1024:3072].copy()
    for _ in range(200):
        h.encode_joint(left, right, 1024, 1024)
    per = []
    for _ in range(args.batches):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            h.encode_joint(left, right, 1024, 1024)
        per.append((time.perf_counter() - t0) / args.calls * 1e3)
    h.close()
    print(json.dumps({"lib": LIB_PATH, "encode_joint_n1_ms_per_call": {
        "median": round(float(np.median(per)), 5), "min": round(min(per), 5), "max": round(max(per), 5),
        "batches": args.batches, "calls_per_batch": args.calls}}))


if __name__ == "__main__":
    main()
