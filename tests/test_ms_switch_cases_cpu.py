"""
The yardstick of tests/test_gpu_ms_switch_cases.py, checked on the CPU against NumPy and the oracle alone (no kernel runs
here):

  1. `pairwise` of tests/ms_switch_cases.py IS the np.sum of the NumPy that is installed, bit for bit, on every band of every
     table and family -- if a NumPy ever sums in another order this test says so, not the GPU test;
  2. the restated decision equals oracle.fast.ms_switch_batch, and on the codec's own tables the reference module's
     oracle.ms_stereo.MSSwitchSFBands;
  3. the content does what it is there for: every band of the four knife-edge families lies within 1e-15 of the threshold in
     exact arithmetic, both decisions occur, and each way of getting the order or the rounding wrong flips a sizeable share
     of the decisions (the shares are printed: run with -s);
  4. beside the threshold (family `beside`, margin 1e-9) every variant and the exact decision agree with the oracle.
"""
import numpy as np
import pytest

from oracle import fast
from oracle.ms_stereo import MSSwitchSFBands

import ms_switch_cases as mc

TABLES = mc.all_tables()
CODEC = mc.codec_tables()

# variant -> (what it replaces in switch(), the least share of the oracle's decisions it must flip, the bands counted)
VARIANTS = {
    "sequential": (dict(sum=mc.sequential), 0.10, lambda n: n >= 8),
    "combine_left_to_right": (dict(sum=mc.combine_left_to_right), 0.10, lambda n: n >= 8),
    "tail_first": (dict(sum=mc.tail_first), 0.10, lambda n: (n >= 10) & (n % 8 >= 2)),
    "split_unrounded": (dict(sum=mc.split_unrounded), 0.10,
                        lambda n: np.array([mc.has_unrounded_split(int(v)) for v in n], dtype=bool)),
    "fused_terms": (dict(terms=mc.fused_terms), 0.03, lambda n: np.ones(len(n), dtype=bool)),
}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def test_the_tables_cover_what_they_should():
    direct = mc.direct_tables()
    lengths = [n for t in direct.values() for n in t]
    assert set(range(273)) | set(mc.BIG) <= set(lengths)
    packed = [t for k, t in direct.items() if k.startswith("packed")]
    every = list(range(273)) + list(mc.BIG)
    assert sorted(n for t in packed for n in t) == sorted(every)
    fewest = max(-(-sum(map(mc.nodes, every)) // mc.MAX_NODES), -(-len(every) // mc.MAX_BANDS))
    assert len(packed) == fewest                               # no packing of the two limits has fewer tables
    assert any(sum(map(mc.nodes, t)) == mc.MAX_NODES for t in direct.values())
    assert sum(map(mc.nodes, mc.REFUSED_TABLE)) == mc.MAX_NODES + 1 and len(mc.REFUSED_TABLE) <= mc.MAX_BANDS
    assert direct["one_line"] == (1,)
    assert [mc.nodes(n) for n in (0, 128, 129, 256, 257, 272, 363, 2048)] == [1, 1, 3, 3, 5, 7, 7, 31]
    assert not mc.has_unrounded_split(256) and mc.has_unrounded_split(363) and mc.has_unrounded_split(693)
    # the codec's tables: the four default shapes and every shape of every setting are among them
    for (sid, a, b) in mc.setting_shapes():
        assert tuple(int(v) for v in mc.codec_bands(sid, a, b).nLines) in CODEC.values()
    assert max(max(t) for t in CODEC.values()) == 363            # (longer bands: the direct tables only)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_pairwise_is_np_sum(name):
    n_lines = TABLES[name]
    for fam in mc.FAMILIES:
        L, R = mc.content(n_lines, fam)
        with np.errstate(all="ignore"):
            for x in mc.plain_terms(L, R):
                lo = 0
                for n in n_lines:
                    want = np.array([np.sum(row[lo:lo + n]) for row in x])
                    assert _same_bits(mc.pairwise(x[:, lo:lo + n]), want), (name, fam, lo, n)
                    lo += n


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_restated_switch_is_the_oracles(name):
    n_lines = TABLES[name]
    sfb = mc.codec_bands(*mc.codec_shapes()[name]) if name in CODEC else None
    for fam in mc.FAMILIES:
        L, R = mc.content(n_lines, fam)
        sw = mc.oracle_switch(n_lines, fam)                   # oracle.fast.ms_switch_batch
        assert sw.shape == (len(L), len(n_lines))
        assert np.array_equal(mc.switch(L, R, n_lines), sw), (name, fam)
        assert (sw[:, np.asarray(n_lines) == 0] == 0).all()
        if sfb is not None:
            with np.errstate(all="ignore"):
                assert np.array_equal(fast.ms_switch_batch(L[:4], R[:4], sfb), sw[:4])
                for i in range(len(L)):
                    assert MSSwitchSFBands(L[i], R[i], sfb) == list(sw[i]), (name, fam, i)
    sw = mc.oracle_switch(n_lines, "special")
    assert (sw[[0, 1, 2, 3]] == 0).all()                       # d == s == 0: not below
    longest = int(np.argmax(n_lines))
    assert (sw[[5, 6, 7], longest] == 0).all()                 # d NaN, or d == s == inf


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_content_sits_on_the_threshold_and_tells_the_orders_apart(name):
    n_lines = TABLES[name]
    n = np.asarray(n_lines)
    for fam in mc.EDGE_FAMILIES:
        L, R = mc.content(n_lines, fam)
        sw = mc.oracle_switch(n_lines, fam)
        margin = mc.exact_margin(L, R, n_lines)
        live = ~np.isnan(margin)                               # s > 0
        assert live[:, n > 0].all() and not live[:, n == 0].any()
        assert margin[live].max() <= 1e-15, (name, fam, margin[live].max())
        ones = sw[live].mean()
        report = ["%-18s %-6s blocks %4d  margin <= %.1e  ones %.3f" % (name, fam, len(L), margin[live].max(), ones)]
        assert 0.2 <= ones <= 0.8, (name, fam, ones)
        for v, (kw, least, counted) in VARIANTS.items():
            c = counted(n)
            if not c.any():                                    # no band of this table on which the variant can differ
                continue
            share = (mc.switch(L, R, n_lines, **kw) != sw)[:, c].mean()
            report.append("%s %.3f" % (v, share))
            assert share >= least, (name, fam, v, share)
        print("  ".join(report))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_beside_the_threshold_every_order_agrees(name):
    n_lines = TABLES[name]
    L, R = mc.content(n_lines, "beside")
    sw = mc.oracle_switch(n_lines, "beside")
    live = np.asarray(n_lines) > 0
    margin = mc.exact_margin(L, R, n_lines)[:, live]
    assert margin.min() > 1e-10 and margin.max() < 1e-8
    assert np.array_equal(mc.exact_switch(L, R, n_lines), sw)
    assert 0.2 <= sw[:, live].mean() <= 0.8
    for v, (kw, _, _) in VARIANTS.items():
        assert np.array_equal(mc.switch(L, R, n_lines, **kw), sw), (name, v)


def test_fused_terms_round_once():
    """the integer form of fused_terms against fractions.Fraction, line by line"""
    n_lines = TABLES["default_128x128"]
    for fam in mc.EDGE_FAMILIES + ("wide",):
        L, R = mc.content(n_lines, fam)
        d, s = mc.fused_terms(L[:2], R[:2])
        plain = mc.plain_terms(L[:2], R[:2])[0]
        want = np.array([[mc.fused_difference_by_fraction(float(l), float(r)) for l, r in zip(lr, rr)]
                         for lr, rr in zip(L[:2], R[:2])])
        assert _same_bits(d, want), fam
        assert (d != plain).any(), fam                         # ... and the second rounding does show
        assert (np.abs(s / mc.plain_terms(L[:2], R[:2])[1] - 1.0) <= 2.0 ** -52).all()
