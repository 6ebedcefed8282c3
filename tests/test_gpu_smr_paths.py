"""
GPU tests of every masking-kernel instantiation launch_smr (csrc/mrc_kernels_smr.hip) can start, on content that reaches the
branches the kernel chooses from the data: slope nodes, nodes with chunks sent back to the sorted sweep, the whole-unit sorted
sweep (slope range too wide, fewer than 32 maskers, more than the block length's ceiling), units without a masker, and masker
counts at the capacity of the scans (the flat comb: every second FFT bin a strict peak).  tests/test_smr_paths_cpu.py proves on
the CPU that the corpus (smr_content.corpus: 16 pairs of a content and a channel relation, 8 blocks each, per block shape) reaches
each of them among the L/R units and among the M/S units.

  instantiation                                   reached here by
  <.,.,256,1024,1> mono long (own unit)           encode_mono, StreamEncoder at (1024, 1024)
  <.,.,256,1024,2> joint long, switch known       encode_joint, StreamEncoder at (1024, 1024)
  <.,.,256,1024,0> long, thresholds out           Handle.smr(want_thresh=True) on L, R, M, S
  <.,.,256,576,1> / <.,.,256,576,0>               encode_mono / encode_joint, smr at (1024, 128) and (128, 1024)
  smr_short_kernel, modes 1 and 2                 encode_mono / encode_joint at (128, 128)
  <.,.,128,128,1> / <.,.,128,128,0>               the same with MRC_OPT_SENSITIVITY (and smr with thresholds)
  <.,.,256,0,0> any other length                  a handle with n_mdct_lines = 512, n_short = 256 at (512, 512) and (512, 256)
  EXACT = true                                    MRC_OPT_EXACT_SPREAD, joint and mono, two frames per pair

Every threshold and SMR is within 1e-9 dB of the oracle's, every integer of an encode equals the oracle's, and calls of 1 and of
5 blocks are bit for bit the rows of the call that holds the whole corpus of a shape (128 blocks: the batch kernels).  That the
sent-back branch RAN in the joint and the transition instantiations is read from the device's own count.

A differing integer here is a finding, not a near-tie, unless the frame's thresholds agree and the certificate counts a near-edge
decision in it; no pair of the corpus needed another seed for that.
"""
import numpy as np
import pytest

from oracle import fast
import smr_content as C
import smr_paths_restatement as R

pytestmark = pytest.mark.gpu
DB_ATOL = 1e-9                                        # the project's bound (tests/test_gpu_parity.py)
DEFAULT_SHAPES = [(1024, 1024), (1024, 128), (128, 1024), (128, 128)]
GENERIC_SHAPES = [(512, 512), (512, 256)]
GENERIC = dict(n_mdct_lines=512, n_short=256)
INT_KEYS = ("overall_scale", "ms_switch", "bit_alloc", "scale_factor", "mantissa", "reservoir_out")
OPT_EXACT_SPREAD, OPT_SENSITIVITY = 1, 5
EXACT_FRAMES = (1, 6)                                 # the two frames per pair of the exact-spread case


@pytest.fixture(scope="module")
def handles():
    from mrcaudiocodec_amd import Handle
    hs = {1024: Handle(device_id=0), 512: Handle(device_id=0, **GENERIC)}
    yield hs
    for hd in hs.values():
        hd.close()


def _lines_of(ab):
    return 512 if ab in GENERIC_SHAPES else 1024


_ref = {}


def ref(ab):
    """the corpus at a shape and the oracle's results for it, computed once: joint and mono (left channel) encodes, the four
    signals' blocks and masked thresholds (the SMRs are the joint encode's: fast.smr_batch per signal)"""
    if ab not in _ref:
        a, b = ab
        c = C.corpus(a, b)
        params = dict(nMDCTLines=_lines_of(ab))
        left, right = c["left"], c["right"]
        sigs = [left, right, (left + right) / 2.0, (left - right) / 2.0]
        _ref[ab] = dict(c, sigs=sigs, joint=fast.encode_joint_batch(left, right, a, b, params=params),
                        mono=fast.encode_mono_batch(left, a, b, params=params),
                        thr=[fast.masked_threshold_batch(x, (a + b) // 2, 48000) for x in sigs])
    return _ref[ab]


_acc = {}


def accounts(ab):
    if ab not in _acc:
        c = C.corpus(*ab)
        _acc[ab] = R.joint_accounts(c["left"], c["right"], ab[0], ab[1], _lines_of(ab))[1]
    return _acc[ab]


def _same_ints(got, want, idx, what):
    for k in INT_KEYS:
        if k in got:
            g = np.squeeze(np.asarray(got[k])).astype(np.int64)
            w = np.squeeze(np.asarray(want[k])[idx]).astype(np.int64)
            bad = np.argwhere(g != w)
            assert bad.size == 0, "%s %s: %d entries differ from the oracle's, first at %s" % (what, k, len(bad), bad[0])


def _same_rows(small, big, idx, what):
    for k in small:
        assert np.array_equal(small[k], big[k][idx]), "%s %s: not the rows of the large call" % (what, k)


@pytest.mark.parametrize("ab", DEFAULT_SHAPES + GENERIC_SHAPES)
def test_thresholds_and_smrs_of_the_four_signals(handles, ab):
    a, b = ab
    r = ref(ab)
    h = handles[_lines_of(ab)]
    for s, name in enumerate("LRMS"):
        smr, thr = h.smr(r["sigs"][s], a, b, want_thresh=True)
        dt, ds = np.abs(thr - r["thr"][s]).max(axis=1), np.abs(smr - r["joint"]["smr"][:, s]).max(axis=1)
        print(ab, name, "largest difference: threshold %.2e dB, SMR %.2e dB" % (dt.max(), ds.max()))
        for lab in r["labels"]:
            assert dt[r["rows"][lab]].max() <= DB_ATOL, (ab, name, lab, "threshold", dt[r["rows"][lab]])
            assert ds[r["rows"][lab]].max() <= DB_ATOL, (ab, name, lab, "SMR", ds[r["rows"][lab]])


_big = {}


def _whole(handles, ab, joint):
    """the whole corpus of a shape in one call (more than 64 blocks: the batch kernels, not the few-block path)"""
    key = (ab, joint)
    if key not in _big:
        r = ref(ab)
        h = handles[_lines_of(ab)]
        assert len(r["left"]) > 64
        _big[key] = h.encode_joint(r["left"], r["right"], *ab) if joint else h.encode_mono(r["left"], *ab)
    return _big[key]


@pytest.mark.parametrize("joint", [True, False], ids=["joint", "mono"])
@pytest.mark.parametrize("ab", DEFAULT_SHAPES + GENERIC_SHAPES)
def test_encodes_of_1_5_and_all_blocks(handles, ab, joint):
    r = ref(ab)
    h = handles[_lines_of(ab)]
    want = r["joint" if joint else "mono"]
    big = _whole(handles, ab, joint)
    _same_ints(big, want, np.arange(len(r["left"])), "%s all" % (ab,))
    for lab in r["labels"]:
        first = r["rows"][lab].start
        for n in (1, 5):                              # (5 joint blocks: 20 units, fewer frames than XCDs x signals in some slots)
            idx = np.arange(first + C.N_FRAMES - n, first + C.N_FRAMES)        # the LAST n (frame 0 of a pair is half silent)
            got = (h.encode_joint(r["left"][idx], r["right"][idx], *ab) if joint else h.encode_mono(r["left"][idx], *ab))
            _same_rows(got, big, idx, "%s %s n=%d" % (ab, lab, n))
            _same_ints(got, want, idx, "%s %s n=%d" % (ab, lab, n))


def _stream_encode(torch, enc, ab, left, right, n, stride, offsets):
    a, b = ab
    lines = torch.full((n * (4 if right is not None else 1) * ((a + b) // 2),), float("nan"), dtype=torch.float64, device="cuda:0")
    out = enc.encode(a, b, left, right, n, stride, offsets, lines_out=lines, fresh=True)
    torch.cuda.synchronize()
    assert not torch.isnan(lines).any()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("ab", [(1024, 1024), (1024, 128), (128, 128)])
def test_the_same_frames_as_int16_pcm_on_the_device(handles, ab):
    """StreamEncoder.encode on int16 PCM tensors that end with the last block: the hop-overlapped stream (blocks a stride apart)
    and shuffled offsets[], joint -- and at the long shape mono too (the mono long kernel's own front end)"""
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=handles[1024])
    r = ref(ab)
    starts = r["starts"]
    stride, n = int(starts[1] - starts[0]), len(starts)
    assert np.array_equal(starts, starts[0] + stride * np.arange(n))
    end = int(starts[-1]) + ab[0] + ab[1]
    for lab in r["labels"]:
        idx = np.arange(r["rows"][lab].start, r["rows"][lab].stop)
        pcm = r["pcm"][lab][:, int(starts[0]):end]
        dl, dr = (torch.from_numpy(pcm[c].copy()).to("cuda:0") for c in range(2))
        order = np.random.default_rng(len(lab)).permutation(n)
        offs = torch.tensor((starts[order] - starts[0]).astype(np.int64), device="cuda:0")
        for right, want in ((dr, r["joint"]),) + (((None, r["mono"]),) if ab == (1024, 1024) else ()):
            _same_ints(_stream_encode(torch, enc, ab, dl, right, n, stride, None), want, idx, "%s %s stream" % (ab, lab))
            _same_ints(_stream_encode(torch, enc, ab, dl, right, n, 0, offs), want, idx[order], "%s %s offsets" % (ab, lab))


@pytest.mark.parametrize("ab", DEFAULT_SHAPES)
def test_with_the_sensitivity_certificate_on(handles, ab):
    """MRC_OPT_SENSITIVITY: short blocks go through smr_kernel<., ., 128, 128, .> instead of smr_short_kernel; every shape keeps its
    integers.  Pair by pair (8 blocks: 32 joint units), so that the device's count of node chunks sent back can be held against
    the restatement's: at least its chunks at 4 x tol or more among the evaluated units' chunks the kernel does not skip (the
    step), and zero where no such chunk comes near the tolerance (bound <= tol / 2: the flat comb and the impulse pair among
    them, whose evaluated units do not take the nodes at all)."""
    r = ref(ab)
    h = handles[1024]
    acc = accounts(ab)
    have_nodes = (ab[0] + ab[1]) // 2 in R.CEILING
    h.set_option(OPT_SENSITIVITY, 1)
    try:
        sent = {}
        for lab in r["labels"]:
            idx = np.arange(r["rows"][lab].start, r["rows"][lab].stop)
            h.sensitivity(reset=True)
            got = h.encode_joint(r["left"][idx], r["right"][idx], *ab)
            sens = h.sensitivity(reset=True)
            _same_ints(got, r["joint"], idx, "%s %s joint, certificate on" % (ab, lab))
            assert sens["blocks_examined"] == len(idx), sens
            units = [acc[f][s] for f in idx for s in range(4) if acc[f][s]["evaluated"]]
            least = sum(R.sent_chunks(u) for u in units)
            quiet = all(not u["nodes"] or u["chunk_ratio"][u["needed"]].max() <= R.CLEAN_BELOW for u in units)
            sent[lab] = (sens["node_chunks_sent_back"], least)
            assert sens["node_chunks_sent_back"] >= least, (ab, lab, sens, least)
            if quiet or not have_nodes:
                assert sens["node_chunks_sent_back"] == 0, (ab, lab, sens)
            _same_ints(h.encode_mono(r["left"][idx], *ab), r["mono"], idx, "%s %s mono, certificate on" % (ab, lab))
        print(ab, "node chunks sent back (device, restatement's least):", sent)
        if have_nodes:
            assert sent["step-apart"][1] >= 8 and sent["step-same"][1] >= 8           # (the restatement's count is not trivial)
            assert all(sent[lab][0] == 0 for lab in ("comb-apart", "sparse-same", "tone-rsilent", "noise-mix"))
    finally:
        h.set_option(OPT_SENSITIVITY, 0)


@pytest.mark.parametrize("ab", DEFAULT_SHAPES + GENERIC_SHAPES)
def test_with_the_exact_spread(handles, ab):
    """MRC_OPT_EXACT_SPREAD (the reference's own per-pair expression with pow): two frames per pair, joint and mono"""
    r = ref(ab)
    h = handles[_lines_of(ab)]
    idx = np.concatenate([r["rows"][lab].start + np.array(EXACT_FRAMES) for lab in r["labels"]])
    h.set_option(OPT_EXACT_SPREAD, 1)
    try:
        joint = h.encode_joint(r["left"][idx], r["right"][idx], *ab)
        mono = h.encode_mono(r["left"][idx], *ab)
    finally:
        h.set_option(OPT_EXACT_SPREAD, 0)
    _same_ints(joint, r["joint"], idx, "%s joint, exact spread" % (ab,))
    _same_ints(mono, r["mono"], idx, "%s mono, exact spread" % (ab,))
