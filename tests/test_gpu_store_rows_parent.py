"""
The store's window calls against what the commit before their restructuring gave (tests/golden/store_rows_parent.npz,
recorded by tools/record_store_rows.py from that commit's library): every case of tests/store_rows_cases.py gives the same
bytes (sha256), shape, chunks_parsed, decode_launches, slabs and plan_bytes_uploaded, and every refused call the same status
and the same words.  The other store tests hold reverberated and transformed rows to a tolerance only; a change of the
pre-roll a slab is decoded with, or of the path a range without a convolved term takes, would pass them while moving bits and
chunks_parsed -- this test is what notices.

If a later change of a kernel legitimately moves the bits of reverberated or transformed rows, the fixture is recorded again
with the tool (see its docstring); nothing here is loosened.
"""
import os

import pytest

from chain_kit import handles_closed_after_module  # noqa: F401
import store_rows_cases as cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_rows_parent.npz")


@pytest.fixture(scope="module")
def both():
    """(recorded, got): every case is run once, here"""
    files, recorded = cases.load(FIXTURE)
    return recorded, cases.run_all(files)


def test_the_table_is_the_recorded_one(both):
    recorded, got = both
    assert sorted(recorded["success"]) == sorted(label for label, _, _, _ in cases.success_cases())
    assert sorted(recorded["success"]) == sorted(got["success"]) and sorted(recorded["refused"]) == sorted(got["refused"])
    assert len(recorded["success"]) >= 40 and len(recorded["refused"]) >= 100
    assert all(v["status"] != 0 and v["error"] for v in recorded["refused"].values())


def test_successful_calls_give_the_recorded_bytes_and_statistics(both):
    recorded, got = both
    different = {k: (v, got["success"].get(k)) for k, v in recorded["success"].items() if got["success"].get(k) != v}
    assert not different, different
    # the rows that went through the kernels whose times are reported did report them
    assert any(v.get("reverb_ms_positive") for v in recorded["success"].values())
    assert all(v["stft_ms_positive"] for k, v in recorded["success"].items() if k.startswith("stft"))


def test_refused_calls_give_the_recorded_status_and_words(both):
    recorded, got = both
    different = {k: (v, got["refused"].get(k)) for k, v in recorded["refused"].items() if got["refused"].get(k) != v}
    assert not different, different
