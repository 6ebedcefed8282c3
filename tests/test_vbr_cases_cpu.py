"""
The crafted VBR blocks (tests/vbr_cases.py) on the CPU: the restatement alone must take every branch of the rule often
enough for the GPU tests (tests/test_gpu_vbr_cases.py) to mean something, and no decision of it may hang on the last bits of
the arithmetic.
"""
import numpy as np
import pytest

import vbr_cases as vc
import vbr_restatement as vr


@pytest.mark.parametrize("cfg", vc.CONFIGS, ids=vc.config_id)
def test_every_branch_is_reached(cfg):
    """at least NEED cases of every branch the configuration can hold; the ones it cannot hold are named by
    vbr_cases.impossible (mono: no L/R pair, no M/S band; maxMantBits < 16: no step 17; maxMantBits 2 in mono: no interior state;
    only 192 kHz has bands without lines) and must indeed not occur"""
    ref, hit, imp = vc.reference(cfg), vc.branch_counts(cfg), vc.impossible(cfg)
    possible = {k: int(v) for k, v in hit.items() if k not in imp}
    low = min(possible, key=possible.get)
    print("%s: edges %d, blocks drawn again %d, smallest count %s = %d; %s" % (
        vc.config_id(cfg), ref["edges"], ref["redrawn"], low, possible[low], possible))
    assert ref["edges"] == 0
    for k in imp:
        assert hit[k] == 0, (k, hit[k])
    for k, v in possible.items():
        assert v >= vc.NEED, "%s: only %d cases of %s" % (vc.config_id(cfg), v, k)


@pytest.mark.parametrize("cfg", [(128, 128, True, "default"), (128, 128, False, "192k"), (128, 128, True, "H")], ids=vc.config_id)
def test_the_walk_without_a_ceiling_holds_every_walk(cfg):
    """the sequence of states is fixed by the signal: the walk at a ceiling is a prefix of the walk without one, and the
    stopping state is the first whose ratios meet the ceiling"""
    cs, ref = vc.cases(cfg), vc.reference(cfg)
    for i, blk in enumerate(ref["blocks"]):
        c = ref["ceilings"][cs["ceiling"][i]]
        for s in range(len(blk["trail"])):
            for j, trail in enumerate(blk["trail"][s]):
                full = blk["profile"]["trail"][s][j]
                assert full[:len(trail)] == trail or all(np.isnan(t[1]) for t in trail), (i, s, j)
                for t in trail[:-1]:
                    assert not all(r <= c for r in t[1:]), (i, s, j)


def test_the_planes_are_what_the_families_say():
    cfg = (1024, 1024, True, "default")
    cs, lay = vc.cases(cfg), vc.layout(cfg)
    scaled = cs["lines"] * np.ldexp(1.0, cs["overall_scale"])[:, :, None]
    assert (np.abs(scaled) < 1.0).all()
    kinds = set(cs["joint_kind"])
    assert kinds == set(vc.JOINT_KINDS)
    for i, k in enumerate(cs["joint_kind"]):
        if k == "s_equals_m":
            assert np.array_equal(cs["lines"][i, 2], cs["lines"][i, 3]) and cs["overall_scale"][i, 2] == cs["overall_scale"][i, 3]
    assert np.isinf(cs["T"]).any() and (cs["T"] == -30.0).any() and (cs["T"] == 200.0).any()
    assert set(np.unique(cs["ceiling"])) == set(range(2 + vc.N_FINITE))
    assert vr.candidates(lay["max_bits"]) == [0] + list(range(2, 17))
