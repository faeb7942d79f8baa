"""CPU: the C-ABI library loads and exports every symbol include/kvh.h declares
(no compute calls: there is no GPU here)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "kvh.h")
LIB = os.path.join(ROOT, "raikv_amd", "libkvh.so")


def declared():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kvh_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_hot_path():
    names = declared()
    for must in ("kvh_meow128_fixed", "kvh_meow128_var", "kvh_meow128_multiseed", "kvh_meow128_batch",
                 "kvh_hash_meow128", "kvh_hash_meow128_4_same_length_4_seed", "kvh_meow128_init"):
        assert must in names


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build libkvh.so first (make / __graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    missing = [n for n in declared() if n not in exported]
    assert not missing, missing


def test_binding_loads_without_gpu():
    import raikv_amd
    assert raikv_amd.lib.kvh_version().startswith(b"raikv_amd")
    assert raikv_amd.lib.kvh_strerror(-22) == b"invalid argument"
    # argument validation happens before any device call
    assert raikv_amd.lib.kvh_meow128_fixed(None, 16, 10, 0, 0, None, 0, None) == -22
    assert raikv_amd.lib.kvh_meow128_fixed(None, 16, 0, 0, 0, None, 0, None) == 0  # n == 0 is a no-op
    assert raikv_amd.lib.kvh_set_tuning(0, 3) == -22


def test_batched_sort_scratch_and_validation_without_gpu():
    """kvh_ht_sort_batched's scratch size and argument checks are host-only:
    batch 1..65536, one slice per batch (a nonzero size for n = 0), and the
    bad calls fail before any device work."""
    import ctypes as C
    import raikv_amd
    lib = raikv_amd.lib
    assert lib.kvh_ht_sort_batched_scratch_bytes(1000, 0) == 0
    assert lib.kvh_ht_sort_batched_scratch_bytes(1000, 65537) == 0
    one = lib.kvh_ht_sort_batched_scratch_bytes(16384, 16384)
    assert one > 0 and one % 256 == 0
    assert lib.kvh_ht_sort_batched_scratch_bytes(0, 16384) == one
    assert lib.kvh_ht_sort_batched_scratch_bytes(16385, 16384) == 2 * one
    assert lib.kvh_ht_sort_batched_scratch_bytes(1024 * 16384, 16384) == 1024 * one
    g = raikv_amd.HtGeom.from_map(64 << 20, 64, 1.0, 4, 4)
    # geometry missing, unknown flags, NULL buffers with n > 0, batch out of range
    assert lib.kvh_ht_sort_batched(None, None, 0, 16384, None, None, None, None, 0, None, 0, None) == -22
    assert lib.kvh_ht_sort_batched(None, None, 0, 16384, C.byref(g), None, None, None, 0x4, None, 0, None) == -22
    assert lib.kvh_ht_sort_batched(None, None, 10, 16384, C.byref(g), None, None, None, 0, None, 0, None) == -22
    assert lib.kvh_ht_sort_batched(None, None, 0, 0, C.byref(g), None, None, None, 0, None, 0, None) == -22
    assert lib.kvh_ht_sort_batched(None, None, 0, 16384, C.byref(g), None, None, None, 0x8, None, 0, None) == 0


def test_product_library_exports_only_the_header():
    """libkvh.so exports exactly what include/kvh.h declares; the research
    kernels and ablation builds (outputs that are not hashes) are not
    reachable: their knobs are rejected."""
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert exported == set(declared()), sorted(exported ^ set(declared()))
    import raikv_amd
    lib = raikv_amd.lib
    for knob, val in ((5, 1), (5, 2), (5, 3), (6, 2), (9, 1), (10, 1), (11, 200), (12, 4), (13, 2), (7, 2),
                      (7, 3), (7, 6), (7, 9), (7, 12), (7, 40), (7, 41), (7, 42), (7, 43), (18, 3), (18, 4), (22, 2),
                      (26, -1), (26, 1 << 16)):
        assert lib.kvh_set_tuning(knob, val) == -22, (knob, val)
    # the variants that lost their A/B compile only into the experiments build
    # (VERDICT r4 item 7): tables per LDS and keys per lane other than the
    # per-length defaults, knob 7 = 7, 13, 24, 25, 44, 45, 47-50, knob 14 =
    # 1-5, knob 23 = 1, 2, knob 24 = 3-5
    for knob, vals in ((0, (2, 4)), (3, (1, 2, 3, 4, 8)), (7, (7, 13, 24, 25, 44, 45, 47, 48, 49, 50)),
                       (14, (1, 2, 3, 4, 5)), (23, (1, 2)), (24, (3, 4, 5))):
        for val in vals:
            assert lib.kvh_set_tuning(knob, val) == -22, (knob, val)
    # product knobs still switch (and return the previous value)
    for knob, val, dflt in ((7, 23, 46), (7, 0, 46), (14, 0, 6), (23, 0, 3), (24, 1, 0), (24, 2, 0), (26, 6, 0)):
        prev = lib.kvh_set_tuning(knob, val)
        assert prev == dflt and lib.kvh_set_tuning(knob, prev) == val, (knob, val)


def test_cpp_host_mirror_compiles(tmp_path):
    # the C++ KeyFragment/HashSeed mirror is header-only over the C-ABI
    src = '#include "raikv_amd/key_hash.hpp"\nint main(){ kvh::KeyBuf kb("hello"); return kb.keylen == 6 ? 0 : 1; }\n'
    exe = str(tmp_path / "kvh_mirror_check")
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-", "-o", exe,
                        "-L", os.path.join(ROOT, "raikv_amd"), "-lkvh", "-Wl,-rpath," + os.path.join(ROOT, "raikv_amd")],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_kv_compat_library_exports_the_meow_family():
    """libkvh_kv.so (link compatibility with include/raikv/key_hash.h:8-20 and :59-130)
    exports exactly the kv_* names include/kvh_kv.h declares, and links
    libkvh.so (it hashes on the GPU through the C-ABI)."""
    lib = os.path.join(ROOT, "raikv_amd", "libkvh_kv.so")
    assert os.path.exists(lib), "build it with make"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kvh_kv.h")).read(), flags=re.S)
    want = set(re.findall(r"\b(kv_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    got = set(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert got == want and len(want) == 22, sorted(got ^ want)
    deps = subprocess.run(["ldd", lib], capture_output=True, text=True).stdout
    assert "libkvh.so" in deps


def test_kv_compat_c_program_needs_only_libkvh_kv():
    """The C test program of the CRC32C family (tests/cpp/kv_compat_crc.c)
    names only libkvh_kv.so among the engine's libraries: a raikv build that
    drops src/key_hash.c links exactly that."""
    exe = os.path.join(ROOT, "tests", "cpp", "kv_compat_crc")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tests/cpp/kv_compat_crc"], check=True)
    dyn = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    needed = [l.split("[")[1].rstrip("]") for l in dyn.splitlines() if "(NEEDED)" in l]
    assert "libkvh_kv.so" in needed and "libkvh.so" not in needed and not any("amdhip" in x for x in needed), needed

