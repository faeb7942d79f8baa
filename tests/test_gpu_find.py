"""GPU parity of the batched find (kvh_ht_find, kvh_meow128_fixed_find)
against the reference's own KeyCtx::find on tables the reference filled
(tests/golden/find_*.npz, tests/golden/make_find_golden.py) and, for the
snapshot states the reference would spin on, against the model that
tests/test_find_model.py pins to those fixtures.  Exact: status, inc, chains,
pos (u64 and KVH_POS32), the gathered rows.

Run on an MI355X:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle_lib  # noqa: E402
import find_model as fm  # noqa: E402

ORC = oracle_lib.load_oracle()
FIX = fm.find_fixtures()
IDS = [f["name"] for f in FIX]
STATIC = (0xA8E0BCC94D1855F5, 0xAD3BEC1E8DE4A1A3)


@pytest.fixture(scope="module")
def kvh():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    import raikv_amd
    raikv_amd.set_poison_outputs(True)  # outputs start as 0xA5 bytes: a row no lane wrote shows
    return raikv_amd


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    if a.dtype == np.int32:
        return a.view(np.uint32)
    return a.view(np.uint64) if a.dtype == np.int64 else a


def geom_of(kvh, f):
    g = kvh.HtGeom()
    g.ht_mod_mask, g.ht_mod_fraction, g.ht_mod_shift, g.ht_size = (int(x) for x in f["geom"])
    g.cuckoo_buckets, g.cuckoo_arity = f["buckets"], f["arity"]
    return g


def want_of(f):
    """(res u32, pos u64) the reference answered for every query of the fixture."""
    return fm.pack_res(f["status"], f["chains"], f["inc"]), f["pos"]


def want_rows(image, status, pos):
    rows = np.zeros((len(status), image.shape[1]), np.uint8)
    ok = status == fm.KEY_OK
    rows[ok] = image[pos[ok].astype(np.int64)]
    return rows


def check_find(got, res, pos, rows=None, pos32=False):
    gpos, gres, grows = got
    np.testing.assert_array_equal(host(gres), res)
    np.testing.assert_array_equal(host(gpos), pos.astype(np.uint32) if pos32 else pos)
    if rows is not None:
        np.testing.assert_array_equal(host(grows), rows)
    else:
        assert grows is None


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_find_golden(kvh, f):
    g = geom_of(kvh, f)
    ent = torch.from_numpy(f["image"]).cuda()
    h = dev_u64(f["queries"])
    res, pos = want_of(f)
    rows = want_rows(f["image"], f["status"], f["pos"])
    check_find(kvh.ht_find(ent, g, h, entry_size=f["es"]), res, pos)
    check_find(kvh.ht_find(ent, g, h, entry_size=f["es"], pos32=True), res, pos, pos32=True)
    got = kvh.ht_find(ent, g, h, entry_size=f["es"], gather=True)
    check_find(got, res, pos, rows)
    # a KEY_OK row carries the 8-byte immediate value: the key's index
    ok = np.flatnonzero(f["status"] == fm.KEY_OK)
    vals = host(got[2])[ok][:, fm.VALUE_OFF:fm.VALUE_OFF + 8].copy().view(np.uint64)[:, 0]
    np.testing.assert_array_equal(vals, ok.astype(np.uint64))
    check_find(kvh.ht_find(ent, g, h, entry_size=f["es"], pos32=True, gather=True), res, pos, rows, pos32=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ent.cpu().numpy(), f["image"])  # the table is never written


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_find_prefixes(kvh, f, n):
    """wave and block edges: the first n queries (repeated if the fixture has fewer)"""
    g = geom_of(kvh, f)
    ent = torch.from_numpy(f["image"]).cuda()
    sel = np.arange(n) % len(f["queries"])
    res, pos = want_of(f)
    h = dev_u64(f["queries"][sel]) if n else torch.empty((0, 2), dtype=torch.int64, device="cuda")
    got = kvh.ht_find(ent, g, h, entry_size=f["es"], gather=True)
    assert tuple(got[0].shape) == (n,) and tuple(got[1].shape) == (n,) and tuple(got[2].shape) == (n, f["es"])
    check_find(got, res[sel], pos[sel], want_rows(f["image"], f["status"][sel], f["pos"][sel]))


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_fused_golden_keys16(kvh, f):
    g = geom_of(kvh, f)
    ent = torch.from_numpy(f["image"]).cuda()
    keys = torch.from_numpy(f["keys16"]).cuda()
    sel = f["keys16_q"]
    res, pos = want_of(f)
    rows = want_rows(f["image"], f["status"][sel], f["pos"][sel])
    for pos32 in (False, True):
        hh, *got = kvh.meow128_fixed_find(keys, 16, f["seed"], ent, g, entry_size=f["es"], pos32=pos32, gather=True)
        np.testing.assert_array_equal(host(hh), f["queries"][sel])
        check_find(got, res[sel], pos[sel], rows, pos32=pos32)
    hh, *got = kvh.meow128_fixed_find(keys, 16, f["seed"], ent, g, entry_size=f["es"], keep_hashes=False)
    assert hh is None
    check_find(got, res[sel], pos[sel])


@pytest.mark.parametrize("L,buckets,arity,es", [(32, 4, 4, 64), (24, 4, 4, 64), (16, 2, 3, 64), (32, 1, 1, 128),
                                                (24, 8, 2, 128)])
def test_fused_equals_hash_then_find(kvh, L, buckets, arity, es):
    """The fused kernel (L 16/32 with 1/2/4/8 positions) and the two-launch
    path (the rest) on a model-built image: equal to meow128_fixed(fixup) +
    ht_find, and to the model."""
    rng = np.random.default_rng(L * 1000 + buckets * 10 + arity)
    slots, n_in, n_out = 700, 560, 300
    kb = rng.integers(0, 256, (n_in + n_out) * L, dtype=np.uint8)
    hk = oracle_lib.orc_fixed(ORC, kb, L, STATIC, fixup=True)
    og = oracle_lib.orc_geom(ORC, (448 << 10) + es * slots, es, 1.0, buckets, arity)
    image, placed = fm.build_image(ORC, oracle_lib, og, es, hk[:n_in])
    status, pos, chains, inc, _ = fm.find_model(ORC, oracle_lib, og, image, es, hk)
    assert (status[:n_in][placed] == fm.KEY_OK).all() and (status[n_in:] != fm.KEY_OK).all()
    g = kvh.HtGeom.from_map((448 << 10) + es * slots, es, 1.0, buckets, arity)
    assert int(g.ht_size) == slots
    ent = torch.from_numpy(image).cuda()
    keys = torch.from_numpy(kb).cuda()
    hh, *got = kvh.meow128_fixed_find(keys, L, STATIC, ent, g, entry_size=es, gather=True)
    h2 = kvh.meow128_fixed(keys, L, STATIC, fixup=True)
    assert torch.equal(hh, h2)
    np.testing.assert_array_equal(host(hh), hk)
    two = kvh.ht_find(ent, g, h2, entry_size=es, gather=True)
    for a, b in zip(got, two):
        assert torch.equal(a, b)
    check_find(got, fm.pack_res(status, chains, inc), pos, want_rows(image, status, pos))


@pytest.mark.parametrize("name", ["5000_4x4", "3000_lin", "2000_4x4_e128", "600_8x8"])
def test_snapshot_states_the_reference_would_spin_on(kvh, name):
    """Zombie hashes and broken seals in a copy of a fixture image: KEY_BUSY
    where the walk meets one (the stated divergence; expected values from the
    model), and every query whose walk touches none of the changed slots still
    answers what the reference did."""
    f = next(x for x in FIX if x["name"] == name)
    es = f["es"]
    og = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    image = f["image"].copy()
    rng = np.random.default_rng(11)
    occ = np.flatnonzero(image.view(np.uint64)[:, 0] != 0)
    pick = rng.choice(occ, 24, replace=False)
    zombies, unsealed = pick[:12], pick[12:]
    image.view(np.uint64)[zombies, 0] |= np.uint64(1 << 63)
    image.view(np.uint32)[unsealed, es // 4 - 2] &= np.uint32(~(1 << 15) & 0xFFFFFFFF)
    status, pos, chains, inc, probed = fm.find_model(ORC, oracle_lib, og, image, es, f["queries"])
    assert (status == fm.KEY_BUSY).sum() >= 12 and (pos[status == fm.KEY_BUSY] == fm.NOPOS).all()
    changed = set(int(x) for x in pick)
    clean = np.array([not (changed & set(p)) for p in probed])
    assert clean.sum() > len(clean) // 2
    for k in ("status", "pos", "chains", "inc"):
        np.testing.assert_array_equal({"status": status, "pos": pos, "chains": chains, "inc": inc}[k][clean],
                                      f[k][clean])
    g = geom_of(kvh, f)
    got = kvh.ht_find(torch.from_numpy(image).cuda(), g, dev_u64(f["queries"]), entry_size=es, gather=True)
    check_find(got, fm.pack_res(status, chains, inc), pos, want_rows(image, status, pos))


def test_non_default_stream_and_no_gather(kvh):
    f = next(x for x in FIX if x["name"] == "5000_4x4")
    g = geom_of(kvh, f)
    ent = torch.from_numpy(f["image"]).cuda()
    h = dev_u64(f["queries"])
    res, pos = want_of(f)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = kvh.ht_find(ent, g, h, entry_size=64, gather=True, stream=s)
    s.synchronize()
    check_find(got, res, pos, want_rows(f["image"], f["status"], f["pos"]))
    got = kvh.ht_find(ent, g, h, entry_size=64, gather=False, stream=s)
    s.synchronize()
    check_find(got, res, pos)
    keys = torch.from_numpy(f["keys16"]).cuda()
    torch.cuda.synchronize()
    hh, *got = kvh.meow128_fixed_find(keys, 16, f["seed"], ent, g, stream=s)
    s.synchronize()
    sel = f["keys16_q"]
    np.testing.assert_array_equal(host(hh), f["queries"][sel])
    check_find(got, res[sel], pos[sel])
