"""GPU parity of the batched get (kvh_ht_get) against the reference's own
KeyCtx::find + KeyCtx::value on tables with data segments that the reference
filled (tests/golden/get_*.npz, tests/golden/make_get_golden.py) and, for the
states the reference would report or spin on and for the bounded
divergences, against the model that tests/test_get_model.py pins to those
fixtures.  Exact: res (status, inc, chains), pos (u64 and KVH_POS32), val_len,
val_loc, the value rows.

Run on an MI355X:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle_lib  # noqa: E402
import find_model as fm  # noqa: E402
import get_model as gm  # noqa: E402

ORC = oracle_lib.load_oracle()
FIX = gm.get_fixtures()
IDS = [f["name"] for f in FIX]
STRIDES = (16, 64, 4096)


@pytest.fixture(scope="module")
def kvh():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu tests must run on an MI355X")
    import raikv_amd
    raikv_amd.set_poison_outputs(True)  # outputs start as 0xA5 bytes: a byte no lane wrote shows
    return raikv_amd


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    if a.dtype == np.int32:
        return a.view(np.uint32)
    return a.view(np.uint64) if a.dtype == np.int64 else a


def geoms_of(kvh, f):
    g = kvh.HtGeom()
    g.ht_mod_mask, g.ht_mod_fraction, g.ht_mod_shift, g.ht_size = (int(x) for x in f["geom"])
    g.cuckoo_buckets, g.cuckoo_arity = f["buckets"], f["arity"]
    return g, kvh.SegGeom(f["seg_size"], f["nsegs"], f["shift"])


_WANT = {}


def want_of(f):
    """What the reference answered for every query of the fixture (computed once, never changed)."""
    if f["name"] not in _WANT:
        values = gm.fixture_values(f)
        w = dict(res=fm.pack_res(gm.fixture_status(f), f["chains"], f["inc"]), pos=f["pos"],
                 vlen=f["vsize"].astype(np.uint32), vloc=f["vloc"], rows={s: gm.rows_of(values, s) for s in STRIDES})
        for a in (w["res"], w["vlen"], *w["rows"].values()):
            a.setflags(write=False)
        _WANT[f["name"]] = w
    return _WANT[f["name"]]


def check_get(got, w, sel=slice(None), stride=None, pos32=False, loc=True):
    gpos, gres, gvlen, gvloc, grows = got
    np.testing.assert_array_equal(host(gres), w["res"][sel])
    np.testing.assert_array_equal(host(gpos), w["pos"][sel].astype(np.uint32) if pos32 else w["pos"][sel])
    np.testing.assert_array_equal(host(gvlen), w["vlen"][sel])
    if loc:
        np.testing.assert_array_equal(host(gvloc), w["vloc"][sel])
    else:
        assert gvloc is None
    if stride is not None:
        np.testing.assert_array_equal(host(grows), w["rows"][stride][sel])
    else:
        assert grows is None


def images(f):
    return torch.from_numpy(f["image"]).cuda(), torch.from_numpy(f["segments"]).cuda()


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_get_golden(kvh, f, stride):
    g, sg = geoms_of(kvh, f)
    ent, segs = images(f)
    h = dev_u64(f["queries"])
    w = want_of(f)
    check_get(kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], stride=stride), w, stride=stride)
    check_get(kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], stride=stride, pos32=True), w, stride=stride,
              pos32=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ent.cpu().numpy(), f["image"])  # neither image is ever written
    np.testing.assert_array_equal(segs.cpu().numpy(), f["segments"])


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_get_without_rows_and_without_loc(kvh, f):
    g, sg = geoms_of(kvh, f)
    ent, segs = images(f)
    h = dev_u64(f["queries"])
    w = want_of(f)
    check_get(kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], copy=False), w)
    check_get(kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], stride=64, want_loc=False), w, stride=64, loc=False)
    check_get(kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], copy=False, want_loc=False, pos32=True), w,
              pos32=True, loc=False)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_get_slices(kvh, f, n):
    """wave edges: n queries across the end of the inserted ones, at every stride"""
    g, sg = geoms_of(kvh, f)
    ent, segs = images(f)
    sel = slice(f["n"] - 30, f["n"] - 30 + n)  # inserted keys, then absent ones
    h = dev_u64(f["queries"][sel])
    for stride in STRIDES:
        got = kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], stride=stride)
        assert tuple(got[4].shape) == (n, stride) and tuple(got[2].shape) == (n,)
        check_get(got, want_of(f), sel=sel, stride=stride)


def test_get_empty_batch(kvh):
    f = FIX[0]
    g, sg = geoms_of(kvh, f)
    ent, segs = images(f)
    got = kvh.ht_get(ent, g, segs, sg, torch.empty((0, 2), dtype=torch.int64, device="cuda"), entry_size=f["es"])
    assert [tuple(t.shape) for t in got] == [(0,), (0,), (0,), (0,), (0, 64)]


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_get_agrees_with_find(kvh, f):
    """pos, inc and chains of ht_get equal ht_find's on the same inputs; the
    status differs only where value() changed a KEY_OK."""
    g, sg = geoms_of(kvh, f)
    img, sgs, _ = gm.mutated_images(f)
    for image, segments in ((f["image"], f["segments"]), (img, sgs)):
        ent, segs = torch.from_numpy(image).cuda(), torch.from_numpy(segments).cuda()
        h = dev_u64(f["queries"])
        fpos, fres, _ = kvh.ht_find(ent, g, h, entry_size=f["es"])
        gpos, gres, _, _, _ = kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], copy=False)
        assert torch.equal(fpos, gpos)
        fr, gr = host(fres), host(gres)
        np.testing.assert_array_equal(fr >> 8, gr >> 8)
        diff = (fr & 0xFF) != (gr & 0xFF)
        assert ((fr & 0xFF)[diff] == fm.KEY_OK).all() and np.isin((gr & 0xFF)[diff],
                                                                   (gm.KEY_MUTATED, gm.KEY_NO_VALUE)).all()


@pytest.mark.parametrize("f", FIX, ids=IDS)
def test_model_only_states(kvh, f):
    """Copies of the fixture images with single fields changed, a few keys per
    state (get_model.mutated_images; tests/test_get_model.py checks that each
    state gives its status in the model and leaves every other query as the
    reference answered it): the kernel equals the model on every query."""
    g, sg = geoms_of(kvh, f)
    og = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    img, sgs, states = gm.mutated_images(f)
    m = gm.get_model(ORC, oracle_lib, og, img, f["es"], sgs, f["seg"], f["queries"])
    w = dict(res=fm.pack_res(m["status"], m["chains"], m["inc"]), pos=m["pos"], vlen=m["vlen"], vloc=m["vloc"],
             rows={64: gm.rows_of(m["values"], 64)})
    ent, segs = torch.from_numpy(img).cuda(), torch.from_numpy(sgs).cuda()
    got = kvh.ht_get(ent, g, segs, sg, dev_u64(f["queries"]), entry_size=f["es"], stride=64)
    st = host(got[1]) & 0xFF
    for name, (idx, want) in states.items():
        assert (st[idx] == want).all(), (name, st[idx])
    check_get(got, w, stride=64)
    untouched = np.ones(len(st), bool)
    for idx, _ in states.values():
        untouched[idx] = False
    np.testing.assert_array_equal(host(got[4])[untouched], want_of(f)["rows"][64][untouched])


@pytest.mark.parametrize("name", ["5000_4x4", "3000_lin", "2000_4x4_e128"])
def test_get_without_segments(kvh, name):
    """nsegs = 0 with a NULL segment image, on the find fixtures: every value
    is the immediate u64 key index; an entry that claims a segment value is
    KEY_MUTATED as seg_data reports it."""
    f = next(x for x in fm.find_fixtures() if x["name"] == name)
    es = f["es"]
    g = kvh.HtGeom()
    g.ht_mod_mask, g.ht_mod_fraction, g.ht_mod_shift, g.ht_size = (int(x) for x in f["geom"])
    g.cuckoo_buckets, g.cuckoo_arity = f["buckets"], f["arity"]
    og = fm.geom_from_fields(oracle_lib, f["geom"], f["buckets"], f["arity"])
    image = f["image"].copy()
    ok = np.flatnonzero(f["status"] == fm.KEY_OK)
    claim = f["pos"][ok[:5]].astype(np.int64)
    image.view(np.uint16)[claim, 10] ^= np.uint16(gm.FL_SEGMENT_VALUE | gm.FL_IMMEDIATE_VALUE)
    m = gm.get_model(ORC, oracle_lib, og, image, es, None, (0, 0, 6), f["queries"])
    assert (m["status"][ok[:5]] == gm.KEY_MUTATED).all() and (m["status"][ok[5:]] == fm.KEY_OK).all()
    w = dict(res=fm.pack_res(m["status"], m["chains"], m["inc"]), pos=m["pos"], vlen=m["vlen"], vloc=m["vloc"],
             rows={16: gm.rows_of(m["values"], 16)})
    got = kvh.ht_get(torch.from_numpy(image).cuda(), g, None, kvh.SegGeom(0, 0, 6), dev_u64(f["queries"]),
                     entry_size=es, stride=16)
    check_get(got, w, stride=16)
    vals = host(got[4])[ok[5:], :8].copy().view(np.uint64)[:, 0]
    np.testing.assert_array_equal(vals, ok[5:].astype(np.uint64))


def test_non_default_stream(kvh):
    f = FIX[0]
    g, sg = geoms_of(kvh, f)
    ent, segs = images(f)
    h = dev_u64(f["queries"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = kvh.ht_get(ent, g, segs, sg, h, entry_size=f["es"], stride=64, stream=s)
    s.synchronize()
    check_get(got, want_of(f), stride=64)
