"""
What the CPU tests of the store's Python front share: a PacStore that was never created -- no library, no device -- on
which every refusal made before a library call can be provoked.
"""
import numpy as np


class NoLibrary:
    """in place of the library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


class _Cfg:
    sample_rate, device_id = 48000, 0


class Handle:
    """in place of the store's handle: its configuration can be read, anything else fails the test"""
    cfg = _Cfg()

    def __getattr__(self, name):
        raise AssertionError("the handle was reached: %s" % name)


def husk(monkeypatch, n_channels=(2, 1), n_irs=0, handle=True):
    """a PacStore with `lib` replaced by NoLibrary: files of n_channels channels, 6144 samples and 7, 6, ... blocks each, a
    bank of n_irs impulse responses of 100 taps, no cached levels; handle=False: no handle at all (None)"""
    from mrcaudiocodec_amd import store
    monkeypatch.setattr(store, "lib", NoLibrary())
    s = store.PacStore.__new__(store.PacStore)
    n = len(n_channels)
    s._handle, s._s, s._levels = Handle() if handle else None, None, {}
    s.n_channels, s.n_samples = np.array(n_channels, np.int32), np.full(n, 6144, np.int64)
    s.n_blocks = np.arange(7, 7 - n, -1).astype(np.int64)
    s._ir_lengths = np.full(n_irs, 100, np.int64)
    return s
