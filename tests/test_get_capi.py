"""CPU: the batched get's public surface -- libkvh.so exports kvh_ht_get and
kvh_seg_geom_init, the header and the binding declare them as documented, the
argument checks that need no GPU answer KVH_EINVAL, and kvh_seg_geom_init
equals HashTab::initialize's segment geometry as the fixtures recorded it."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import get_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raikv_amd", "libkvh.so")
KVH_EINVAL = -22
FIX = gm.get_fixtures()
HDR = 448 << 10


def test_library_exports_the_get_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"kvh_ht_get", "kvh_seg_geom_init", "kvh_ht_find"} <= syms


def test_header_declares_get_with_its_reference_calls():
    hdr = open(os.path.join(ROOT, "include", "kvh.h")).read()
    assert "int kvh_ht_get(const void *entries, uint32_t hash_entry_size, const kvh_ht_geom_t *geom," in hdr
    assert "int kvh_seg_geom_init(uint64_t map_size, uint32_t hash_entry_size," in hdr
    assert "#define KVH_KEY_MUTATED    6" in hdr and "#define KVH_KEY_NO_VALUE   8" in hdr
    assert "typedef struct {\n  uint64_t seg_size;" in hdr and "} kvh_seg_geom_t;" in hdr
    sec = hdr[hdr.index("Batched get on a table image"):hdr.index("Batch order by table position")]
    for cite in ("key_ctx.cpp:959-1001", "hash_entry.h:333-340", "msg_ctx.h:113-132", "shm_ht.h:468-474",
                 "ht_init.cpp:118-192"):
        assert cite in sec


def test_binding_signature_and_struct():
    import raikv_amd as kvh
    p = inspect.signature(kvh.ht_get).parameters
    assert list(p) == ["entries", "geom", "segments", "sgeom", "hashes", "entry_size", "stride", "pos32", "want_loc",
                       "copy", "stream"]
    assert [p[k].default for k in ("entry_size", "stride", "pos32", "want_loc", "copy", "stream")] == [
        64, 64, False, True, True, None]
    assert (kvh.KVH_KEY_MUTATED, kvh.KVH_KEY_NO_VALUE) == (6, 8)
    assert [(n, t) for n, t in kvh.SegGeom._fields_] == [("seg_size", C.c_uint64), ("nsegs", C.c_uint32),
                                                         ("seg_align_shift", C.c_uint32)]
    assert C.sizeof(kvh.SegGeom) == 16
    assert len(kvh.lib.kvh_ht_get.argtypes) == 15 and len(kvh.lib.kvh_seg_geom_init.argtypes) == 6


def _args(kvh):
    g = kvh.HtGeom.from_map(HDR + 64 * 600, 64, 1.0, 4, 4)
    s = kvh.SegGeom(16384, 16, 6)
    buf = (C.c_uint64 * 16)()  # 16-byte aligned dummies: every check here comes before a device is needed
    p = C.cast(buf, C.c_void_p)
    assert p.value % 16 == 0
    return g, s, p


def test_argument_checks_without_gpu():
    import raikv_amd as kvh
    g, s, p = _args(kvh)
    get = kvh.lib.kvh_ht_get

    def call(ent=p, es=64, geom=g, segs=p, sg=s, h=p, n=1, pos=p, res=p, loc=p, vlen=p, rows=p, stride=16, flags=0):
        return get(ent, es, C.byref(geom) if geom is not None else None, segs,
                   C.byref(sg) if sg is not None else None, h, n, pos, res, loc, vlen, rows, stride, flags, None)

    for es in (0, 32, 48, 96 + 4, 33):  # a multiple of 32, at least 64
        assert call(es=es) == KVH_EINVAL and kvh.lib.kvh_last_error() == KVH_EINVAL
    for stride in (0, 24, 8, 100):  # with values_out: a non-zero multiple of 16
        assert call(stride=stride) == KVH_EINVAL
    off = C.c_void_p(p.value + 8)
    for kw in ("ent", "segs", "h", "rows"):  # 16-byte aligned
        assert call(**{kw: off}) == KVH_EINVAL, kw
    for kw, d in (("pos", 4), ("res", 2), ("vlen", 2), ("loc", 4)):
        assert call(**{kw: C.c_void_p(p.value + d)}) == KVH_EINVAL, kw
    assert call(sg=None) == KVH_EINVAL
    assert call(segs=None) == KVH_EINVAL  # nsegs > 0
    assert call(geom=None) == KVH_EINVAL
    for kw in ("ent", "h", "pos", "res", "vlen"):
        assert call(**{kw: None}) == KVH_EINVAL, kw
    # a segment geometry whose messages would not be 16-byte aligned, or whose shift cannot be a shift
    for bad in (kvh.SegGeom(16384, 16, 3), kvh.SegGeom(16384 + 32, 16, 6), kvh.SegGeom(0, 16, 6),
                kvh.SegGeom(16384, 0, 32)):
        assert call(sg=bad) == KVH_EINVAL
    # the geometry checks of kvh_ht_find
    bad = kvh.HtGeom.from_map(HDR + 64 * 600, 64, 1.0, 4, 4)
    bad.ht_size = 10
    assert call(geom=bad) == KVH_EINVAL
    big = kvh.HtGeom.from_map(1 << 41, 64, 1.0, 4, 4)
    assert call(geom=big, flags=kvh.KVH_POS32) == KVH_EINVAL


def test_empty_batch_needs_no_gpu_and_no_buffers():
    import raikv_amd as kvh
    g, s, _ = _args(kvh)
    none = kvh.SegGeom(0, 0, 6)
    for sg in (s, none):
        assert kvh.lib.kvh_ht_get(None, 64, C.byref(g), None, C.byref(sg), None, 0, None, None, None, None, None, 0,
                                  0, None) == 0


@pytest.mark.parametrize("f", FIX, ids=[f["name"] for f in FIX])
def test_seg_geom_init_equals_the_recorded_header(f):
    import raikv_amd as kvh
    s = kvh.SegGeom.from_map(f["map_size"], f["es"], np.float32(f["ratio"]), f["max_value"])
    assert (int(s.nsegs), int(s.seg_size), s.seg_start, int(s.seg_align_shift)) == (
        f["nsegs"], f["seg_size"], f["seg_start"], f["shift"])
    assert s.nbytes == len(f["segments"])
    g = kvh.HtGeom.from_map(f["map_size"], f["es"], np.float32(f["ratio"]), f["buckets"], f["arity"])
    assert [int(g.ht_mod_mask), int(g.ht_mod_fraction), int(g.ht_mod_shift), int(g.ht_size)] == [
        int(x) for x in f["geom"]]


def test_seg_geom_init_known_point_and_no_segments():
    import raikv_amd as kvh
    ratio = np.float32(64000.0 / 326144.0)
    s = kvh.SegGeom.from_map(458752 + 64000 + 262144, 64, ratio, 4096)
    g = kvh.HtGeom.from_map(458752 + 64000 + 262144, 64, ratio, 4, 4)
    assert (int(g.ht_size), int(s.nsegs), int(s.seg_size), s.seg_start, int(s.seg_align_shift)) == (
        999, 16, 16384, 522688, 6)
    z = kvh.SegGeom.from_map(HDR + 64 * 600, 64, 1.0, 0)
    assert (int(z.nsegs), int(z.seg_size), z.seg_start, z.nbytes) == (0, 0, 0, 0)
    assert kvh.lib.kvh_seg_geom_init(HDR, 64, 1.0, 4096, C.byref(z), None) == KVH_EINVAL
    assert kvh.lib.kvh_seg_geom_init(HDR + 64 * 600, 64, 1.0, 4096, None, None) == KVH_EINVAL
