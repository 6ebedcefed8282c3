"""
GPU test of where the `.pac` readers say a bad chunk lies when it is NOT in the first file of the call: three short stereo
files (six long blocks and Close()'s block each, chained encode), one chunk's Huffman table id set to 4 in the second or
in the last file.  Whole-file decode, the noise-to-mask ratio and the store's windows (plain and mix) must all refuse with
code -1 and `file F: chunk at byte B: table id not in {0..3, 15}`, F the damaged file and B counted from that file's first
byte; a store window inside an undamaged file still decodes to the bits of the whole-file decode.
"""
import re

import numpy as np
import pytest

import chain_kit as kit
from chain_kit import handles_closed_after_module  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HOP = kit.HOP
BLOCKS = 6
REASON = re.escape("table id not in {0..3, 15}")


@pytest.fixture(scope="module")
def trio():
    """the three files, their sources and indices, and the whole-file decodes of the undamaged files (never written to)"""
    from mrcaudiocodec_amd import pacfile as ppac
    h = kit.handle()
    pcm = [kit.noise(BLOCKS, seed, 48000) for seed in (21, 22, 23)]
    shapes = [(i * HOP, HOP, HOP) for i in range(BLOCKS)]
    files = ppac.encode_stereo_streams(h, np.stack(pcm), [shapes] * 3)
    index = [ppac.index(f) for f in files]
    assert all(ix["n_channels"] == 2 and ix["n_blocks"] == BLOCKS + 1 for ix in index)
    assert len({len(f) for f in files}) == 3                       # (no two files start at a multiple of one length)
    whole = [np.ascontiguousarray(p) for p in h.decode_pac_pcm16(files, interleaved=False)]
    for w, ix in zip(whole, index):
        assert w.shape == (2, ix["n_samples"]) and ix["n_samples"] == (BLOCKS + 1) * HOP     # (Close()'s block counts)
        w.setflags(write=False)
    return dict(h=h, files=files, index=index, whole=whole, src=[np.ascontiguousarray(p[:, HOP:]) for p in pcm])


# (file, block, channel): a joint block of the second file; the right chunk of Close()'s block of the last file
@pytest.mark.parametrize("f,block,ch", [(1, 3, 0), (2, BLOCKS, 1)])
def test_a_bad_chunk_is_located_in_its_file(trio, f, block, ch):
    from mrcaudiocodec_amd import MrcError
    from mrcaudiocodec_amd.store import PacStore
    h, ix = trio["h"], trio["index"][f]
    byte = int(ix["chunk_offset"][block, ch])                      # counted from the file's first byte
    bad = bytearray(trio["files"][f])
    bad[byte + 4] = (bad[byte + 4] & 0x0F) | 0x40                  # table id 4
    files = list(trio["files"])
    files[f] = bytes(bad)
    where = r"file %d: chunk at byte %d: %s" % (f, byte, REASON)

    with pytest.raises(MrcError, match=r"mrc_decode_pac_pcm16: " + where) as e:
        h.decode_pac_pcm16(files)
    assert e.value.code == -1
    with pytest.raises(MrcError, match=r"mrc_pac_nmr: " + where) as e:
        h.pac_nmr(files, trio["src"])
    assert e.value.code == -1

    n = int(ix["n_samples"])
    with PacStore(h, files) as store:
        with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window: " + where) as e:
            store.decode_window([0, 1, 2], [0, 0, 0], n)           # one item per file, every chunk of each
        assert e.value.code == -1
        with pytest.raises(MrcError, match=r"mrc_pac_store_decode_window_mix: " + where) as e:
            store.decode_window([0, 1, 2], [0, 0, 0], n, mix="mid")
        assert e.value.code == -1
        for g in range(3):                                         # windows wholly inside the undamaged files
            if g != f:
                got = store.decode_window([g], [700], 3000)[0].cpu().numpy()
                assert np.array_equal(got, trio["whole"][g][:, 700:3700]), g
