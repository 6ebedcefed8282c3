"""
CPU proof of what the corpus of tests/test_gpu_smr_paths.py (smr_content.corpus) makes the masking kernels do, from the NumPy
account of the kernel's choices (tests/smr_paths_restatement.py) and the oracle's M/S switch.  A joint unit none of whose bands
the switch selects ends before its first load: only EVALUATED units count.

For the default handle's long and transition shapes there is, among the L/R units and among the M/S units, at least one
evaluated unit that takes
  clean   the slope nodes with no chunk near the tolerance (bound <= 0.5 x tol in every chunk the kernel does not skip),
  sent    the nodes with a chunk sent back to the sorted sweep by a bound of at least 4 x tol (rounding cannot move it across),
  slope   the whole-unit sorted sweep because its slope range is too wide,
  few     ... because it has fewer than 32 maskers,
  many    ... because it has more than the block length's ceiling,
  none    no masker at all.
The flat comb reaches the capacity of the masker scans at every block length, both branches of the M/S switch occur inside
frames, and the short shape has units with 0, 1 and 13 maskers.

Run with -s to see the counts, the masker counts and the bound ratios per shape (DESIGN.md section 4 quotes them).
"""
import pytest

import smr_content as C
import smr_paths_restatement as R

LONG, SHORT = (1024, 1024), (128, 128)
TRANSITION = [(1024, 128), (128, 1024)]
GENERIC = [(512, 512), (512, 256)]                    # a handle with n_mdct_lines = 512, n_short = 256
CLASSES = ("clean", "sent", "slope", "few", "many", "none")

_cache = {}


def accounts(a, b, n_mdct_lines=1024):
    """(ms_switch [B][nBands], accounts [B][4]) of the corpus at shape (a, b); computed once"""
    key = (a, b, n_mdct_lines)
    if key not in _cache:
        c = C.corpus(a, b)
        _cache[key] = R.joint_accounts(c["left"], c["right"], a, b, n_mdct_lines)
    return _cache[key]


def _evaluated(a, b, label=None, n_mdct_lines=1024, first=0):
    """(signal, account) of every evaluated unit, of one pair of the corpus (from its frame `first` on) or of all"""
    _, acc = accounts(a, b, n_mdct_lines)
    rows = range(len(acc)) if label is None else range(*C.corpus(a, b)["rows"][label].indices(len(acc)))[first:]
    return [(s, acc[f][s]) for f in rows for s in range(4) if acc[f][s]["evaluated"]]


def test_the_ceilings_are_the_headers():
    assert {dim: R.node_max_maskers(dim) for dim in R.CEILING} == R.CEILING
    assert [R.max_peaks(n) for n in (2048, 1152, 256)] == [461, 237, 13]
    assert set(R.CEILING) == {1024, 576}                                  # (kNodes: the long and the transition block)


@pytest.mark.parametrize("ab", [LONG] + TRANSITION)
def test_every_class_is_reached_on_both_sides_of_the_switch(ab):
    a, b = ab
    units = _evaluated(a, b)
    for side, sigs in (("L/R", (0, 1)), ("M/S", (2, 3))):
        count = {k: 0 for k in CLASSES}
        top = {k: 0.0 for k in ("clean", "sent")}
        for s, acc in units:
            k = R.classify(acc)
            if s in sigs and k in count:
                count[k] += 1
                if k in top:
                    top[k] = max(top[k], float(acc["chunk_ratio"][acc["needed"]].max()))
        print(ab, side, count, "largest bound / tol: clean %.2f, sent %.1f" % (top["clean"], top["sent"]))
        assert all(count[k] >= 1 for k in CLASSES), (ab, side, count)
    # what each content is in the corpus for
    tops = {lab: [acc["maskers"] for _, acc in _evaluated(a, b, lab)] for lab in C.LABELS}
    print(ab, {lab: (min(v), max(v)) for lab, v in tops.items()})
    assert all(R.classify(acc) == "clean" for _, acc in _evaluated(a, b, "noise-mix", first=1))      # (frame 0 is half silent)
    for lab in ("step-apart", "step-same"):
        sent = [R.sent_chunks(acc) for _, acc in _evaluated(a, b, lab)]
        print(ab, lab, "chunks at >= 4 x tol per evaluated unit:", sent)
        assert sum(1 for v in sent if v >= 2) >= 4, (lab, sent)
    for lab in ("comb-apart", "sparse-same", "tone-rsilent"):                       # (no unit through the nodes)
        assert not any(acc["nodes"] for _, acc in _evaluated(a, b, lab, first=1)), lab
    ceiling = R.CEILING[(a + b) // 2]
    assert any(ceiling < m < 0.8 * R.max_peaks(a + b) for m in tops["comb6-apart"]), "just above the ceiling"


@pytest.mark.parametrize("ab,least", [(LONG, 455), (TRANSITION[0], 233), (SHORT, 13), (GENERIC[0], 200), (GENERIC[1], 138)])
def test_the_flat_comb_fills_the_masker_scans(ab, least):
    a, b = ab
    nm = 512 if ab in GENERIC else 1024
    most = max(acc["maskers"] for lab in ("comb-mix", "comb-apart") for _, acc in _evaluated(a, b, lab, nm))
    print(ab, "flat comb:", most, "of", R.max_peaks(a + b))
    assert least <= most <= R.max_peaks(a + b)


@pytest.mark.parametrize("ab", [LONG] + TRANSITION + [SHORT] + GENERIC)
def test_both_branches_of_the_switch_inside_frames(ab):
    a, b = ab
    sw, _ = accounts(a, b, 512 if ab in GENERIC else 1024)
    mixed = int((sw.min(axis=1) != sw.max(axis=1)).sum())
    print(ab, "frames with L/R and M/S bands:", mixed, "of", len(sw), " M/S share %.2f" % sw.mean())
    assert mixed >= 8 and (sw.min(axis=1) == 1).any() and (sw.max(axis=1) == 0).any()


def test_short_and_generic_units_take_the_sorted_sweep():
    counts = sorted(set(acc["maskers"] for _, acc in _evaluated(*SHORT)))
    print(SHORT, "masker counts of the evaluated units:", counts)
    assert {0, 1, 13} <= set(counts)
    for ab, nm in [(SHORT, 1024)] + [(g, 512) for g in GENERIC]:
        assert set(acc["why"] for _, acc in _evaluated(*ab, n_mdct_lines=nm)) == {"length", "none"}
