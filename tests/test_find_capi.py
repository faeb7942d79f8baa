"""CPU: the batched find's public surface -- libkvh.so exports kvh_ht_find
and kvh_meow128_fixed_find, the binding exposes ht_find and
meow128_fixed_find with the documented signatures, and the argument checks
that need no GPU answer KVH_EINVAL."""
import ctypes as C
import inspect
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raikv_amd", "libkvh.so")
KVH_EINVAL = -22


def test_library_exports_both_find_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"kvh_ht_find", "kvh_meow128_fixed_find"} <= syms


def test_header_declares_both_with_their_reference_calls():
    hdr = open(os.path.join(ROOT, "include", "kvh.h")).read()
    assert "int kvh_ht_find(const void *entries, uint32_t hash_entry_size," in hdr
    assert "int kvh_meow128_fixed_find(const void *keys, uint32_t key_len, size_t n," in hdr
    sec = hdr[hdr.index("Batched find on a table image"):hdr.index("Batch order by table position")]
    for cite in ("ht_search.h:308-367", "key_ctx.h:245-246", "ht_cuckoo.h:135-141", "ht_linear.cpp:33-41"):
        assert cite in sec


def test_binding_signatures():
    import raikv_amd as kvh
    p = inspect.signature(kvh.ht_find).parameters
    assert list(p) == ["entries", "geom", "hashes", "entry_size", "pos32", "gather", "stream"]
    assert (p["entry_size"].default, p["pos32"].default, p["gather"].default, p["stream"].default) == (
        64, False, False, None)
    q = inspect.signature(kvh.meow128_fixed_find).parameters
    assert list(q)[:5] == ["keys", "key_len", "seed", "entries", "geom"]
    assert {"entry_size", "pos32", "gather", "stream"} <= set(q)
    assert (kvh.KVH_KEY_OK, kvh.KVH_KEY_NOT_FOUND, kvh.KVH_KEY_BUSY, kvh.KVH_KEY_HT_FULL) == (0, 2, 3, 5)
    assert kvh.lib.kvh_ht_find.argtypes is not None and kvh.lib.kvh_meow128_fixed_find.argtypes is not None


def test_entry_size_and_geometry_checks_without_gpu():
    import raikv_amd as kvh
    g = kvh.HtGeom.from_map((448 << 10) + 64 * 600, 64, 1.0, 4, 4)
    # non-NULL dummies: the size and geometry checks come before any pointer is looked at or a device is needed
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    for es in (0, 16, 48, 33, 100):
        assert kvh.lib.kvh_ht_find(p, es, C.byref(g), p, 1, p, p, None, 0, None) == KVH_EINVAL
        assert kvh.lib.kvh_last_error() == KVH_EINVAL
        assert kvh.lib.kvh_meow128_fixed_find(p, 16, 1, 1, 2, p, es, C.byref(g), p, p, p, None, 0,
                                              None) == KVH_EINVAL
    for es in (64, 128):
        assert kvh.lib.kvh_ht_find(p, es, None, p, 1, p, p, None, 0, None) == KVH_EINVAL
        assert kvh.lib.kvh_meow128_fixed_find(p, 16, 1, 1, 2, p, es, None, p, p, p, None, 0, None) == KVH_EINVAL
    # a geometry kvh_ht_positions refuses is refused here too (ht_mod leaving ht[])
    bad = kvh.HtGeom.from_map((448 << 10) + 64 * 600, 64, 1.0, 4, 4)
    bad.ht_size = 10
    assert kvh.lib.kvh_ht_positions(p, 1, C.byref(bad), p, 0, None) == KVH_EINVAL
    assert kvh.lib.kvh_ht_find(p, 64, C.byref(bad), p, 1, p, p, None, 0, None) == KVH_EINVAL
    # u32 positions cannot address more than 2^32 slots
    big = kvh.HtGeom.from_map(1 << 41, 64, 1.0, 4, 4)
    assert kvh.lib.kvh_ht_find(p, 64, C.byref(big), p, 1, p, p, None, kvh.KVH_POS32, None) == KVH_EINVAL


def test_empty_batch_needs_no_gpu_and_no_buffers():
    import raikv_amd as kvh
    g = kvh.HtGeom.from_map((448 << 10) + 64 * 600, 64, 1.0, 4, 4)
    assert kvh.lib.kvh_ht_find(None, 64, C.byref(g), None, 0, None, None, None, 0, None) == 0
    assert kvh.lib.kvh_meow128_fixed_find(None, 16, 0, 1, 2, None, 64, C.byref(g), None, None, None, None, 0,
                                          None) == 0
