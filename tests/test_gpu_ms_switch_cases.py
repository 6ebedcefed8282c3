"""
GPU tests of the M/S switch (ms_switch_direct_kernel, csrc/mrc_kernels.hip; the summation tree of mrc::ms_plan) on bands that
sit exactly on its 0.8 threshold (tests/ms_switch_cases.py): there the last ulp of sum|L^2 - R^2| and of sum|L^2 + R^2|
decides, so the kernel must add in np.sum's order -- eight strided accumulators, their fixed combine, the trailing lines,
the split of runs above 128 lines at a multiple of 8 -- and round l*l - r*r twice.  tests/test_ms_switch_cases_cpu.py shows
on the oracle alone that each such mistake in the order flips a tenth or more of these decisions, a contraction 3 % or more.

  a. Handle.ms_switch (mrc_ms_switch: its own plan for any table of 1..32 bands and at most 64 summation nodes): every band
     length 0..272 and lengths up to 2048, the codec's tables, every content family, batches that fill and do not fill a
     workgroup of four blocks; the refusal of a table with 65 nodes;
  b. mrc_dev_alloc_quant and mrc_dev_alloc_quant_chained, every joint configuration of tests/alloc_cases.py and the joint
     shapes of every setting of tests/settings_kit.py: the switch, and every integer behind it;
  c. mrc_dev_encode_ex, which computes its own lines: the switch it returns against the restated decision on the lines it
     returns (the oracle's MDCT differs from the kernel's in the last bits, which on a knife edge legitimately decide).

The yardstick is the oracle (oracle.fast.ms_switch_batch; in c `switch` of tests/ms_switch_cases.py, which the CPU test
pins to np.sum and to the oracle).  Every comparison is exact equality.
"""
import numpy as np
import pytest

import alloc_cases as ac
import ms_switch_cases as mc
import settings_kit as sk
from test_gpu_alloc_cases import Run, _assert_equal, _keys

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 4, 5, 9)                                    # a workgroup holds four blocks, one per wave
CANARY = -31000
TABLES = mc.all_tables()
_HANDLES = {}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def handle_of():
    """key -> Handle: a target bit rate at the default setting, or a setting id"""
    from mrcaudiocodec_amd import Handle

    def get(key):
        if key not in _HANDLES:
            kw = sk.handle_kwargs(key) if isinstance(key, str) else dict(target_bits_per_sample=key)
            _HANDLES[key] = Handle(device_id=0, **kw)
        return _HANDLES[key]
    yield get
    for hd in _HANDLES.values():
        hd.close()
    _HANDLES.clear()


# ------------------------------------------------------------------ a. the direct entry
@pytest.mark.parametrize("name", sorted(TABLES))
def test_direct_entry_equals_the_oracle(handle_of, name):
    hd = handle_of(2.86)
    n_lines = TABLES[name]
    for fam in mc.FAMILIES:
        L, R = mc.content(n_lines, fam)
        want = mc.oracle_switch(n_lines, fam)
        largest = None
        for n in sorted(set(min(n, len(L)) for n in BATCHES), reverse=True):
            got = hd.ms_switch(L[:n], R[:n], n_lines).astype(np.int64)
            assert got.shape == (n, len(n_lines))
            bad = np.argwhere(got != want[:n])
            assert bad.size == 0, "%s %s batch of %d: %d decisions differ from the oracle's, first at (block, band) %s, a band " \
                "of %d lines" % (name, fam, n, len(bad), bad[0], n_lines[bad[0][1]])
            if largest is None:
                largest = got
            assert np.array_equal(got, largest[:n]), (name, fam, n)   # a block's decisions do not depend on the batch


def test_direct_entry_refuses_a_table_of_65_nodes(handle_of):
    from mrcaudiocodec_amd import MrcError, _lib
    hd = handle_of(2.86)
    code, words = mc.REFUSAL
    L, R = mc.content(mc.REFUSED_TABLE, "third")
    with pytest.raises(MrcError) as e:
        hd.ms_switch(L[:4], R[:4], mc.REFUSED_TABLE)
    assert e.value.code == code and str(e.value) == "libmrc_hip error %d: %s" % (code, words)
    # ... before anything is done: the caller's output stays as it was
    nl = np.asarray(mc.REFUSED_TABLE, dtype=np.int32)
    l4, r4 = np.ascontiguousarray(L[:4]), np.ascontiguousarray(R[:4])
    out = np.full((4, len(nl)), CANARY, np.int32)
    rc = _lib.lib.mrc_ms_switch(hd._h, 4, len(nl), _lib._p(nl, _lib._i32p), _lib._p(l4, _lib._f64p), _lib._p(r4, _lib._f64p),
                                _lib._p(out, _lib._i32p))
    assert rc == code and _lib.lib.mrc_last_error(hd._h).decode() == words
    assert (out == CANARY).all()
    full = mc.direct_tables()["full_64_nodes"]               # one node fewer is served (and the handle still works)
    L, R = mc.content(full, "third")
    assert np.array_equal(hd.ms_switch(L[:4], R[:4], full), mc.oracle_switch(full, "third")[:4])


# ------------------------------------------------------------------ b. both back ends, every configuration
def _id(cfg):
    return ac.config_id(cfg[:4]) + ("-" + cfg[4] if len(cfg) > 4 else "")


def _chained_accepts(lay):
    """chain_shape_misfit of csrc/mrc_api_chain.cpp for a joint block"""
    return 2 * lay["nb"] <= 64 and 2 <= lay["max_mant"] <= 16 and lay["half"] % 4 == 0 and 2 * lay["half"] <= 2048


@pytest.mark.parametrize("cfg", mc.backend_configs(), ids=_id)
def test_back_ends_on_threshold_blocks(torch, handle_of, cfg):
    from mrcaudiocodec_amd import MrcError
    hd = handle_of(cfg[4] if len(cfg) > 4 else cfg[3])
    lay = ac.layout(cfg)
    assert np.array_equal(hd.bands(cfg[0], cfg[1]), lay["sfb"].nLines)
    c, want = mc.backend_cases(cfg)
    n = mc.BACKEND_BLOCKS
    on = want["ms_switch"].mean()
    assert 0.2 <= on <= 0.8, on                               # both outcomes, so both SMR pairs and both line pairs are coded
    for chained in (False, True):
        what = "%s %s" % (_id(cfg), "chained" if chained else "dev_alloc_quant")
        run = Run(torch, hd, cfg, c, n, chained)
        if chained and not _chained_accepts(lay):
            with pytest.raises(MrcError):
                run.call(c["reservoir"])
            continue
        got = run.call(c["reservoir"]).ints(what)
        _assert_equal(got, want, _keys(True), what + " vs oracle")


# ------------------------------------------------------------------ c. the encode entry that computes its own lines
@pytest.mark.parametrize("shape", [(1024, 1024), (128, 128), (1024, 128)], ids=lambda s: "%dx%d" % s)
def test_encode_entry_switches_on_its_own_lines(torch, handle_of, shape):
    from mrcaudiocodec_amd.batch import StreamEncoder
    a, b = shape
    n, N, half = 5, a + b, (a + b) // 2
    stride = a
    samples = (n - 1) * stride + N
    x = np.random.default_rng([31, a, b]).normal(0.0, 0.1, samples)
    hd = handle_of(2.86)
    left = torch.from_numpy(x).to("cuda:0")
    right = torch.from_numpy(x / 3.0).to("cuda:0")
    lines = torch.full((n * 4 * half,), float("nan"), dtype=torch.float64, device="cuda:0")
    out = StreamEncoder(handle=hd).encode(a, b, left, right, n, stride, None, lines_out=lines, fresh=True)
    torch.cuda.synchronize()
    lines = lines.cpu().numpy().reshape(n, 4, half)
    assert not np.isnan(lines).any()
    n_lines = [int(v) for v in hd.bands(a, b)]
    got = out["ms_switch"].cpu().numpy().astype(np.int64)
    want = mc.switch(lines[:, 0], lines[:, 1], n_lines)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%dx%d: %d decisions differ from np.sum's order on the call's own lines, first at %s" % (
        a, b, len(bad), bad[0])
    margin = mc.exact_margin(lines[:, 0], lines[:, 1], n_lines)
    assert (margin <= 1e-12).mean() >= 0.5, margin           # the case has not degenerated: these are knife edges
    assert 0 < got.sum() < got.size
