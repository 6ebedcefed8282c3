"""
The mono `.pac` writer composed from oracle pieces (tests/mono_oracle.py: transient.block_shapes, codec.Encode /
EncodeNoHuff, pacfile.file_header / pack_block, Close()'s block) against the bytes the reference's own file layer wrote
for mono WAV files (tests/golden/ref_pac_mono.npz, tests/golden/make_golden_mono.py).  No GPU.
"""
import os

import numpy as np
import pytest

import mono_oracle as MO

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pac_mono.npz")


def _fixture():
    if not os.path.exists(FIXTURE):
        pytest.skip("tests/golden/ref_pac_mono.npz not generated (tests/golden/make_golden_mono.py)")
    return np.load(FIXTURE)


def _cases():
    if not os.path.exists(FIXTURE):
        return ["missing"]
    return [str(c) for c in np.load(FIXTURE)["cases"]]


@pytest.mark.parametrize("huffman", [True, False])
@pytest.mark.parametrize("case", _cases())
def test_oracle_mono_writer_reproduces_reference_bytes(case, huffman):
    g = _fixture()
    pcm, rate = g[case + "_pcm"], int(g[case + "_rate"])
    want = g[case + ("_pac" if huffman else "_pac_raw")].tobytes()
    got = MO.encode_wav_mono(MO.wav_bytes(pcm, rate), huffman)
    assert got[:4] == b"PAC " and int.from_bytes(got[8:10], "little") == 1          # nChannels = 1
    assert got == want


def test_fixture_covers_the_cases_the_mono_path_needs():
    g = _fixture()
    from oracle import codec, transient
    rates, shorts, padded = set(), 0, 0
    for case in g["cases"]:
        case = str(case)
        pcm, rate = g[case + "_pcm"], int(g[case + "_rate"])
        rates.add(rate)
        cp = codec.default_params(sampleRate=rate, nChannels=1)
        shapes = transient.block_shapes(MO.stream_of(pcm[0]), cp)
        shorts += sum(b == 128 for (_, _, b) in shapes)
        padded += pcm.shape[1] % 1024 == 0
        assert shapes[-1][2] == 1024
    assert rates == {44100, 48000} and shorts > 0 and padded > 0
