"""
Record what the store's window calls give and refuse on the cases of tests/store_rows_cases.py: per successful case the sha256
of the output's bytes, its shape and the call's statistics (of reverb_ms and stft_ms only whether they are positive), per
refused case the status and the words of mrc_last_error.  Needs a GPU.

    MRC_HIP_LIBRARY=<library of the commit to record> python tools/record_store_rows.py out.npz

tests/golden/store_rows_parent.npz is this tool's output for the library of the commit BEFORE the window calls were given one
request, one check and three loops over row ranges (that commit's csrc under this tree's binding: the C ABI is the same):
DESIGN.md, "The window calls: request, check, loops".  The file also holds the bytes of the four `.pac` files the cases
read, so that the test needs no encoder.  With two arguments the tool compares two such files instead.  Where a later change
of a kernel legitimately moves the bits of a reverberated or transformed row, record again with that commit's parent's rows
checked first.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make_files():
    """setting B's stereo Huffman, stereo raw and mono files and the mono file's last block alone"""
    import settings_kit as SK
    import store_rows_cases as cases
    from mrcaudiocodec_amd import pacfile as ppac
    sid, cfg = cases.SID, SK.config(cases.SID)
    mono = SK.oracle_file(sid, 1, True)["data"]
    ix = ppac.index(mono, cfg)
    one_block = mono[:int(ix["chunk_offset"][0, 0])] + mono[int(ix["chunk_offset"][-1, 0]):]
    return [SK.oracle_file(sid, 2, True)["data"], SK.oracle_file(sid, 2, False)["data"], mono, one_block]


def record(path):
    import store_rows_cases as cases
    from mrcaudiocodec_amd import _lib
    files = make_files()
    got = cases.run_all(files)
    np.savez_compressed(path, results=np.array(json.dumps(got, sort_keys=True)),
                        **{"file%d" % i: np.frombuffer(bytes(b), np.uint8) for i, b in enumerate(files)})
    print("recorded %d successful and %d refused cases from %s -> %s" % (len(got["success"]), len(got["refused"]), _lib.LIB_PATH, path))


def compare(pa, pb):
    from store_rows_cases import load
    (fa, a), (fb, b) = load(pa), load(pb)
    bad = [] if fa == fb else ["files"]
    for part in ("success", "refused"):
        bad += ["%s: %s" % (part, k) for k in sorted(set(a[part]) | set(b[part])) if a[part].get(k) != b[part].get(k)]
    print("%s vs %s: %s" % (pa, pb, "the same" if not bad else "DIFFERENT: %s" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    record(sys.argv[1])
