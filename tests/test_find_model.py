"""The find model (tests/find_model.py) against the reference: for every
query of every fixture tests/golden/find_*.npz -- tables filled and queried
by the reference's own KeyCtx::acquire / tombstone / find
(tests/golden/make_find_golden.py) -- the model's status, pos, chains and inc
equal what KeyCtx::find answered.  CPU only."""
import numpy as np
import pytest

import oracle_lib
import find_model as fm

ORC = oracle_lib.load_oracle()
FIX = fm.find_fixtures()


def test_fixture_set_is_complete():
    names = {f["name"] for f in FIX}
    assert names == {"600_8x8", "5000_4x4", "4096_2x2", "600_2x5", "3000_lin", "64_lin_full", "2000_4x4_e128"}
    assert {f["es"] for f in FIX} == {64, 128}


@pytest.mark.parametrize("f", FIX, ids=[f["name"] for f in FIX])
def test_model_equals_reference_find(f):
    g = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    assert int(g.ht_size) == f["slots"] == len(f["image"])
    status, pos, chains, inc, _ = fm.find_model(ORC, oracle_lib, g, f["image"], f["es"], f["queries"])
    np.testing.assert_array_equal(status, f["status"])
    np.testing.assert_array_equal(pos, f["pos"])
    np.testing.assert_array_equal(chains, f["chains"])
    np.testing.assert_array_equal(inc, f["inc"])


@pytest.mark.parametrize("f", FIX, ids=[f["name"] for f in FIX])
def test_fixture_values_and_real_keys(f):
    """What the GPU tests rely on: a KEY_OK row's immediate value is the key
    index, and keys16 hash (fixed up) to the queries they are listed for."""
    ok = np.flatnonzero(f["status"] == fm.KEY_OK)
    assert len(ok) and (ok < f["n"]).all()
    rows = f["image"][f["pos"][ok].astype(np.int64)]
    np.testing.assert_array_equal(rows[:, fm.VALUE_OFF:fm.VALUE_OFF + 8].copy().view(np.uint64)[:, 0],
                                  ok.astype(np.uint64))
    h = oracle_lib.orc_fixed(ORC, f["keys16"], 16, f["seed"], fixup=True)
    np.testing.assert_array_equal(h, f["queries"][f["keys16_q"]])


def test_build_image_is_findable():
    """The model's own placement (used for the shapes no fixture has): every
    placed pair is found at its slot with its index as the value."""
    g = oracle_lib.orc_geom(ORC, (448 << 10) + 64 * 700, 64, 1.0, 4, 4)
    rng = np.random.default_rng(5)
    h = rng.integers(2, 2**63, size=(600, 2), dtype=np.uint64)
    img, placed = fm.build_image(ORC, oracle_lib, g, 64, h)
    status, pos, _, _, _ = fm.find_model(ORC, oracle_lib, g, img, 64, h)
    assert placed.sum() > 500
    assert (status[placed] == fm.KEY_OK).all() and (status[~placed] == fm.KEY_NOT_FOUND).all()
    vals = img[pos[placed].astype(np.int64)][:, 32:40].copy().view(np.uint64)[:, 0]
    np.testing.assert_array_equal(vals, np.flatnonzero(placed).astype(np.uint64))
