"""
Record what the masking stage gives for the frames of tests/test_gpu_smr_overflow.py (tests/smr_overflow_inputs.py): smr and
band peaks of every frame, mono and as the four units of a joint frame, each frame in a call of its own from int16 PCM, and the
count of node chunks a mono frame sends back to the sorted sweep.  Needs a GPU.

    MRC_HIP_LIBRARY=<library of the commit to record> python tools/record_smr_overflow.py out.npz

tests/golden/smr_overflow_parent.npz is this tool's output for the library of the commit BEFORE the band contenders' bounds
were made cheap (that commit's kernels under this tree's C ABI, which only adds the entry point the tool calls): DESIGN.md
section 4, "Cheap bounds for the band contenders".  With two arguments the tool compares instead: the bytes of every array of
two such files.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def record(path):
    import torch
    from mrcaudiocodec_amd import Handle, _lib
    import smr_overflow_inputs as I
    h = Handle(device_id=0)
    dev = I.Device(torch, h)
    labs = I.all_labels()
    mono, joint = dev.singles(False, "int16", labs), dev.singles(True, "int16", labs)
    sent = dev.sent_back(labs)
    h.close()
    np.savez_compressed(path, labels=np.array(labs), smr_mono=mono["smr"], band_peak_mono=mono["band_peak"],
                        smr_joint=joint["smr"], band_peak_joint=joint["band_peak"], ms_switch=joint["ms_switch"],
                        sent_back_mono=sent)
    print("recorded %d frames from %s -> %s (chunks sent back: %s)" % (len(labs), _lib.LIB_PATH, path, sent.tolist()))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [k for k in a.files if k not in b.files or a[k].tobytes() != b[k].tobytes()]
    print("%s vs %s: %s" % (pa, pb, "all %d arrays byte-identical" % len(a.files) if not bad else "DIFFERENT: %s" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    record(sys.argv[1])
