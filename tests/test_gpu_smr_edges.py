"""
GPU tests of smr_kernel at the edges of a launch: batches of n = 1, 2, 9 and 257 long frames -- one workgroup, fewer
workgroups than XCDs, an odd count, more than one workgroup per CU slot -- of mono int16 PCM, mono float64 samples and
joint stereo, each read two ways:

  * as a hop-overlapped stream whose PCM tensor holds exactly (n + 1) * 1024 samples, so that the last unit's last sample
    is the last one of the allocation (whatever the kernel requests early or ahead must stay inside it);
  * through explicit offsets[] in shuffled order (units whose neighbours in the launch are not their neighbours in time).

A frame's codes depend on its own samples only (reservoir_in = 0), so every output of a batch must equal BIT FOR BIT the
same frames encoded one at a time, in any order and layout -- and every integer the oracle's.  The content is the
white noise of BASELINE config C2 (synth._gauss_pcm / c3_stereo): its frames have about 257 tonal maskers, on both sides
of the 256 at which the kernel's node terms take a second round (asserted from the oracle's peak count).  One case of
(1024, 128) transition blocks covers the other instantiations that share the kernel's body.
Everything goes through the C ABI (mrc_dev_encode_ex with a lines buffer).
"""
import numpy as np
import pytest

from oracle import fast

pytestmark = pytest.mark.gpu
HOP = 1024
N_MAX = 257
COUNTS = (1, 2, 9, 257)
SEED = 77
INT_KEYS = ("overall_scale", "ms_switch", "bit_alloc", "scale_factor", "mantissa", "reservoir_out")


def _oracle_peaks(blocks):
    """tonal maskers per block as psychoac.py:151-162 counts them (the expressions of fast.masked_threshold_batch)"""
    N = blocks.shape[1]
    X = np.fft.fft(np.multiply(blocks, fast._hann(N)), axis=-1)
    XI = 4. * (np.abs(X) ** 2.) / ((N ** 2.) * (3. / 8.))
    last = N // 2 - 100
    c = XI[:, 1:last - 1]
    return ((c > XI[:, 0:last - 2]) & (c > XI[:, 2:last])).sum(axis=1)


@pytest.fixture(scope="module")
def h():
    from mrcaudiocodec_amd import Handle
    hd = Handle(device_id=0)
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def corpus():
    """int16 codes of N_MAX hops of noise behind the zero hop (mono: the left channel), their float64 samples, and the
    oracle's encode of all N_MAX frames, mono and joint -- computed once; a batch of n frames is its first n."""
    from mrcaudiocodec_amd import synth
    g1 = synth._gauss_pcm(SEED, N_MAX * HOP, 0.1)
    g2 = synth._gauss_pcm(SEED + 1, N_MAX * HOP, 0.1)
    even = (np.arange(N_MAX * HOP) // HOP) % 2 == 0                  # (c3_stereo's mix: M/S wins on even hops, L/R on odd)
    r = np.clip(np.rint(np.where(even, 0.8 * g1 + 0.2 * g2, 0.1 * g2)), -32767, 32767)
    z = np.zeros(HOP)
    l16 = np.concatenate([z, g1]).astype(np.int16)
    r16 = np.concatenate([z, r]).astype(np.int16)
    fl, fr = synth.pcm_to_float(l16), synth.pcm_to_float(r16)
    bl, br = np.array(fast.blocks_from_stream(fl, HOP)), np.array(fast.blocks_from_stream(fr, HOP))
    assert bl.shape == (N_MAX, 2 * HOP)
    return dict(l16=l16, r16=r16, fl=fl, fr=fr, bl=bl, br=br, mono=fast.encode_mono_batch(bl, HOP, HOP),
                joint=fast.encode_joint_batch(bl, br, HOP, HOP), peaks=_oracle_peaks(bl),
                peaks_joint=np.stack([_oracle_peaks(x) for x in (bl, br, (bl + br) / 2.0, (bl - br) / 2.0)], axis=1))


def _encode(torch, enc, a, b, left, right, n, stride, offsets):
    nsig = 4 if right is not None else 1
    lines = torch.full((n * nsig * ((a + b) // 2),), float("nan"), dtype=torch.float64, device="cuda:0")
    out = enc.encode(a, b, left, right, n, stride, offsets, lines_out=lines, fresh=True)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["lines"] = lines.cpu().numpy().reshape(n, nsig, (a + b) // 2)
    return res


def _device(torch, corpus, kind, samples):
    """(left, right) device tensors of exactly `samples` samples: own allocations, nothing behind the last sample"""
    if kind == "f64":
        return torch.from_numpy(corpus["fl"][:samples].copy()).to("cuda:0"), None
    left = torch.from_numpy(corpus["l16"][:samples].copy()).to("cuda:0")
    return left, (torch.from_numpy(corpus["r16"][:samples].copy()).to("cuda:0") if kind == "joint" else None)


_single = {}


def _one_at_a_time(torch, enc, corpus, kind):
    """every frame of the corpus encoded alone, from a tensor that holds its 2048 samples and nothing else"""
    if kind not in _single:
        rows = []
        for f in range(N_MAX):
            sl = slice(f * HOP, (f + 2) * HOP)
            if kind == "f64":
                dl, dr = torch.from_numpy(corpus["fl"][sl].copy()).to("cuda:0"), None
            else:
                dl = torch.from_numpy(corpus["l16"][sl].copy()).to("cuda:0")
                dr = torch.from_numpy(corpus["r16"][sl].copy()).to("cuda:0") if kind == "joint" else None
            rows.append(_encode(torch, enc, HOP, HOP, dl, dr, 1, HOP, None))
        _single[kind] = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    return _single[kind]


def _check_oracle(got, ref, n, order=None):
    idx = np.arange(n) if order is None else order
    for k in INT_KEYS:
        if k in got:
            want = np.asarray(ref[k])[idx]
            assert np.array_equal(np.squeeze(got[k]).astype(np.int64), np.squeeze(want).astype(np.int64)), k


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ["i16", "f64", "joint"])
def test_long_batches_equal_single_frames_and_the_oracle(h, corpus, kind, n):
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=h)
    # frames on both sides of 256 maskers (one frame is on one side: the first frame, half of it the zero hop, is below)
    pk = corpus["peaks_joint"][:n, 0] if kind == "joint" else corpus["peaks"][:n]
    if n == 1:
        assert pk[0] <= 256
    else:
        assert (pk <= 256).any() and (pk > 256).any(), pk
    if kind == "joint" and n >= 2:                                    # frames with L/R bands and with M/S bands
        sw = corpus["joint"]["ms_switch"][:n]
        assert (sw.min(axis=1) == 0).any() and (sw.max(axis=1) == 1).any()
    if kind == "joint" and n == N_MAX:                                # ... and an M signal beyond 256 maskers
        assert (corpus["peaks_joint"][:, 2] > 256).any()
    ref = corpus["joint" if kind == "joint" else "mono"]
    single = _one_at_a_time(torch, enc, corpus, kind)
    dl, dr = _device(torch, corpus, kind, (n + 1) * HOP)
    assert dl.numel() == (n + 1) * HOP
    # the hop-overlapped stream: its last unit ends with the allocation
    stream = _encode(torch, enc, HOP, HOP, dl, dr, n, HOP, None)
    assert not np.isnan(stream["lines"]).any()
    for k in stream:
        assert np.array_equal(stream[k], single[k][:n]), (kind, n, k)
    _check_oracle(stream, ref, n)
    # explicit offsets, shuffled
    order = np.random.default_rng(n).permutation(n)
    offs = torch.tensor(order.astype(np.int64) * HOP, device="cuda:0")
    shuffled = _encode(torch, enc, HOP, HOP, dl, dr, n, 0, offs)
    for k in shuffled:
        assert np.array_equal(shuffled[k], single[k][order]), (kind, n, k)
    _check_oracle(shuffled, ref, n, order)


@pytest.mark.parametrize("kind", ["i16", "f64", "joint"])
def test_transition_batches_equal_single_blocks_and_the_oracle(h, corpus, kind):
    # (1024, 128) blocks a hop apart (the shapes of a block-switched stream, batched by offsets): the transition
    # instantiation of the kernel; the tensor ends with the last block
    torch = pytest.importorskip("torch")
    from mrcaudiocodec_amd.batch import StreamEncoder
    enc = StreamEncoder(handle=h)
    a, b, n = 1024, 128, 9
    N = a + b
    samples = (n - 1) * HOP + N
    starts = np.arange(n) * HOP
    bl = np.stack([corpus["fl"][s:s + N] for s in starts])
    br = np.stack([corpus["fr"][s:s + N] for s in starts])
    ref = fast.encode_joint_batch(bl, br, a, b) if kind == "joint" else fast.encode_mono_batch(bl, a, b)
    dl, dr = _device(torch, corpus, kind, samples)
    assert dl.numel() == samples
    stream = _encode(torch, enc, a, b, dl, dr, n, HOP, None)
    assert not np.isnan(stream["lines"]).any()
    _check_oracle(stream, ref, n)
    order = np.random.default_rng(5).permutation(n)
    shuffled = _encode(torch, enc, a, b, dl, dr, n, 0, torch.tensor(starts[order].astype(np.int64), device="cuda:0"))
    _check_oracle(shuffled, ref, n, order)
    for f in range(n):
        one = _encode(torch, enc, a, b, dl[f * HOP:f * HOP + N].clone(), None if dr is None else dr[f * HOP:f * HOP + N].clone(),
                      1, HOP, None)
        for k in one:
            assert np.array_equal(one[k][0], stream[k][f]), (kind, f, k)
            assert np.array_equal(one[k][0], shuffled[k][int(np.nonzero(order == f)[0][0])]), (kind, f, k)
