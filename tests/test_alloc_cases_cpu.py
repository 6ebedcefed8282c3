"""
The crafted bit-allocation cases (tests/alloc_cases.py) reach what they are meant to reach: an instrumented copy of the
oracle's loop counts, per configuration, the cases that take each branch -- and returns what oracle.bitalloc.BitAlloc
returns on every case.  No GPU.
"""
import numpy as np
import pytest

import alloc_cases as ac
from oracle.bitalloc import BitAlloc

AT_LEAST = 20
EVERYWHERE = ("tie", "two_bit_negative", "retired_no_bits", "retired_full", "no_iteration", "all_retired", "negative_out")
INTEGER_BUDGETS = ("lines_equal_left", "left_zero_after_grant")


@pytest.mark.parametrize("cfg", ac.CONFIGS, ids=ac.config_id)
def test_cases_reach_every_branch_of_the_loop(cfg):
    lay, c, ref = ac.layout(cfg), ac.cases(cfg), ac.reference(cfg)
    n = len(c["reservoir"])
    assert n == len(ac.FAMILIES) * 72 and c["vectors"].shape == (n, lay["n_tot"])
    reached = dict.fromkeys(ac.EVENTS, 0)
    for i in range(n):
        bits, left, hit = ac.instrumented(c["budget"][i], ac.MAX_MANT, lay["n_tot"], lay["n_lines"], c["vectors"][i])
        want_bits, want_left = BitAlloc(c["budget"][i], ac.MAX_MANT, lay["n_tot"], lay["n_lines"], c["vectors"][i].copy())
        assert np.array_equal(bits, want_bits) and left == want_left, i
        assert np.array_equal(bits, ref["bit_alloc"][i].reshape(-1)) and left == ref["reservoir_out"][i], i
        for k in ac.EVENTS:
            reached[k] += hit[k] > 0
    for k in EVERYWHERE:
        assert reached[k] >= AT_LEAST, (k, reached)
    if float(cfg[3]).is_integer():
        assert float(lay["base"]).is_integer()
        for k in INTEGER_BUDGETS:
            assert reached[k] >= AT_LEAST, (k, reached)
    else:
        assert not float(lay["base"]).is_integer()


@pytest.mark.parametrize("cfg", ac.CONFIGS, ids=ac.config_id)
def test_inputs_are_what_the_entries_may_be_given(cfg):
    lay, c = ac.layout(cfg), ac.cases(cfg)
    assert np.isfinite(c["vectors"]).all() and np.abs(c["vectors"]).max() <= 1.1e5
    assert c["reservoir"].min() == -10 ** 6 and c["reservoir"].max() == 10 ** 6 and (c["reservoir"] == lay["fill"]).any()
    scaled = c["lines"] * np.ldexp(1.0, c["overall_scale"])[:, :, None]
    assert (np.abs(scaled) < 1.0).all() and set(np.unique(c["overall_scale"])) == {0, 3, 15}
    if cfg[2]:
        sw = c["ms_switch"]
        on = sw.astype(bool)
        sel = np.stack([~on, ~on, on, on], axis=1)
        assert np.isnan(c["smr"][~sel]).all() and np.isfinite(c["smr"][sel]).all()
        assert sw.all(axis=1).any() and (~on).all(axis=1).any() and ((sw.sum(axis=1) > 0) & (sw.sum(axis=1) < lay["nb"])).any()
    # band peaks on, one ulp under and one ulp over a power of two, and bands of zeros
    lo, hi = np.asarray(lay["sfb"].lowerLine), np.asarray(lay["sfb"].upperLine) + 1
    peak = np.stack([np.abs(c["coded"][:, 0, l:h]).max(axis=1) for l, h in zip(lo, hi)], axis=1)
    m, _ = np.frexp(peak)
    assert (peak == 0).any() and (m == 0.5).any() and (m == np.nextafter(0.5, 1)).any() and (m == np.nextafter(1.0, 0)).any()


def test_ulp_family_hands_near_ties_to_the_repair():
    """pairs of bands whose SMRs differ by less than 1e-12 modulo 6 without being equal: floor(s / 6) and s - 6 floor(s / 6)
    order them one way, the loop's own subtractions may order them the other"""
    for cfg in ac.CONFIGS:
        c = ac.cases(cfg)
        rows = c["vectors"][c["family"] == ac.FAMILIES.index("six_k_ulp")]
        near = 0
        for s in rows:
            d = s[:, None] - s[None, :]
            off = np.abs(d - 6.0 * np.rint(d / 6.0))
            near += int(((off > 0) & (off < 1e-12)).sum()) // 2
        assert near >= 20 * len(rows), (cfg, near)


def test_group_edge_ties_sit_where_the_argmax_groups_meet():
    for cfg in ac.CONFIGS:
        lay, c = ac.layout(cfg), ac.cases(cfg)
        gs = ac.group_size(lay["n_tot"])
        rows = c["vectors"][c["family"] == ac.FAMILIES.index("tie_group_edge")]
        for s in rows:
            top = np.flatnonzero(s == s.max())
            assert len(top) == 2 and top[1] == top[0] + 1 and top[1] % gs == 0, (cfg, top)
        rows = c["vectors"][c["family"] == ac.FAMILIES.index("tie_across_streams")]
        if cfg[2]:
            assert all(list(np.flatnonzero(s == s.max())) == [lay["nb"] - 1, lay["nb"]] for s in rows)


def test_streams_fill_and_drain():
    for cfg in ac.STREAM_CONFIGS:
        lay, c = ac.layout(cfg), ac.stream_cases(cfg)
        assert c["vectors"].shape[0] == ac.N_STREAMS * ac.STREAM_BLOCKS and ac.STREAM_BLOCKS > 264
        ref = ac.stream_reference(cfg, streams=[1, 3])
        ba = ref["bit_alloc"].reshape(2, ac.STREAM_BLOCKS, -1)
        drained = (lay["fill"] - lay["base"]) * ac.STREAM_BLOCKS > 10 ** 6      # (a short block spends too little for that)
        assert (ba[1, 0] == ac.MAX_MANT).all() and (ba[1, -1] == ac.MAX_MANT).all() != drained   # 10^6: every band full
        # -5000: below the budget of a mono block (no bits at first), recovered later
        assert ba[0, -1].any() and (cfg[2] or not ba[0, 0].any()) and ba[0, 0].sum() < ba[0, 1:].sum(axis=1).max()
