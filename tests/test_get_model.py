"""The get model (tests/get_model.py) against the reference: for every query
of every fixture tests/golden/get_*.npz -- tables with data segments, filled
and queried by the reference's own acquire / resize / update_stamps /
tombstone / find / value (tests/golden/make_get_golden.py) -- the model's
status, pos, chains, inc, value size, value location and value bytes equal
what KeyCtx::find + KeyCtx::value answered.  CPU only."""
import numpy as np
import pytest

import oracle_lib
import find_model as fm
import get_model as gm

ORC = oracle_lib.load_oracle()
FIX = gm.get_fixtures()
IDS = [f["name"] for f in FIX]
FIND_FIX = fm.find_fixtures()


def test_fixture_set_is_complete():
    assert {f["name"] for f in FIX} == {"999_4x4", "499_lin_e128", "999_2x2"}
    assert {(f["es"], f["buckets"], f["arity"]) for f in FIX} == {(64, 4, 4), (128, 1, 1), (64, 2, 2)}
    for f in FIX:
        assert len(f["queries"]) == 2 * f["n"] and f["nsegs"] > 0 and f["max_value"] > 0 and f["ratio"] < 1.0
        assert f["image"].shape == (int(f["geom"][3]), f["es"]) and len(f["segments"]) == f["nsegs"] * f["seg_size"]


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_model_equals_reference_find_and_value(f):
    g = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    m = gm.get_model(ORC, oracle_lib, g, f["image"], f["es"], f["segments"], f["seg"], f["queries"])
    np.testing.assert_array_equal(m["status"], gm.fixture_status(f))
    for k in ("pos", "chains", "inc"):
        np.testing.assert_array_equal(m[k], f[k])
    np.testing.assert_array_equal(m["vlen"], f["vsize"].astype(np.uint32))
    np.testing.assert_array_equal(m["vloc"], f["vloc"])
    assert m["values"] == gm.fixture_values(f)


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_fixture_covers_both_kinds_and_the_bounds_hold(f):
    """What the GPU tests rely on: both value kinds with and without a stamp,
    sizes on both sides of every stride used, no KEY_MUTATED / KEY_NO_VALUE /
    KEY_BUSY, and none of the bounded divergences in a table the reference
    wrote (the model applies them and still equals the reference above)."""
    st = gm.fixture_status(f)
    assert not np.isin(st, (fm.KEY_BUSY, gm.KEY_MUTATED, gm.KEY_NO_VALUE)).any()
    ok = np.flatnonzero(st == fm.KEY_OK)
    assert (ok < f["n"]).all() and (st[f["n"]:] != fm.KEY_OK).all()
    fl = f["image"].view(np.uint16)[f["pos"][ok].astype(np.int64), 10]
    seg = (f["vloc"][ok] & np.uint64(gm.SEGBIT)) != 0
    np.testing.assert_array_equal(seg, (fl & gm.FL_SEGMENT_VALUE) != 0)
    np.testing.assert_array_equal(~seg, (fl & gm.FL_IMMEDIATE_VALUE) != 0)
    stamped = (fl & gm.FL_STAMPS) != 0
    for kind in (seg, ~seg):
        assert (kind & stamped).any() and (kind & ~stamped).any()
    sizes = set(int(x) for x in f["vsize"][ok])
    assert {0, 1, 15, 16, 17, 63, 64, 65, 4000} <= sizes
    k1, k2 = (f["flags3"][:, j] & (gm.FL_SEGMENT_VALUE | gm.FL_IMMEDIATE_VALUE) for j in (0, 1))
    assert ((k1 == gm.FL_IMMEDIATE_VALUE) & (k2 == gm.FL_SEGMENT_VALUE)).any()
    assert ((k1 == gm.FL_SEGMENT_VALUE) & (k2 == gm.FL_IMMEDIATE_VALUE)).any()
    # every segment value has a message of its own
    live = set(int(x) & (gm.SEGBIT - 1) for x in f["vloc"][ok][seg])
    assert len(live) == int(seg.sum())


@pytest.mark.parametrize("f", FIND_FIX, ids=[f["name"] for f in FIND_FIX])
def test_find_fixtures_without_segments(f):
    """nsegs = 0: every value of the find fixtures is immediate; inserted row i
    yields the 8 bytes of u64 i."""
    g = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    m = gm.get_model(ORC, oracle_lib, g, f["image"], f["es"], None, (0, 0, 6), f["queries"])
    np.testing.assert_array_equal(m["status"], f["status"])
    np.testing.assert_array_equal(m["pos"], f["pos"])
    ok = np.flatnonzero(f["status"] == fm.KEY_OK)
    assert (m["vlen"][ok] == 8).all() and (m["vlen"][f["status"] != fm.KEY_OK] == 0).all()
    np.testing.assert_array_equal(m["vloc"][ok], f["pos"][ok] * np.uint64(f["es"]) + np.uint64(fm.VALUE_OFF))
    for i in ok:
        assert m["values"][i] == int(i).to_bytes(8, "little")


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_model_only_states(f):
    """The changed images of the GPU test: every changed key gets the status
    its state stands for, and every other query answers what the reference
    did."""
    g = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    img, segs, states = gm.mutated_images(f)
    assert len(states) == 14
    m = gm.get_model(ORC, oracle_lib, g, img, f["es"], segs, f["seg"], f["queries"])
    changed = np.zeros(len(f["queries"]), bool)
    for name, (idx, want) in states.items():
        assert not changed[idx].any(), name
        changed[idx] = True
        assert (m["status"][idx] == want).all(), (name, m["status"][idx])
        assert (m["vlen"][idx] == 0).all() and (m["vloc"][idx] == gm.NOLOC).all(), name
        if want == fm.KEY_BUSY:
            assert (m["pos"][idx] == fm.NOPOS).all(), name
        else:  # pos, inc, chains stay what find reports
            for k in ("pos", "chains", "inc"):
                np.testing.assert_array_equal(m[k][idx], f[k][idx], err_msg=name)
    rest = ~changed
    np.testing.assert_array_equal(m["status"][rest], gm.fixture_status(f)[rest])
    np.testing.assert_array_equal(m["vloc"][rest], f["vloc"][rest])
    want = gm.fixture_values(f)
    assert all(m["values"][i] == want[i] for i in np.flatnonzero(rest))
