#!/usr/bin/env python3
"""Generate tests/golden/find_*.npz from the REFERENCE itself.

Run where the reference tree exists, after `make` has built
oracle/_ref/libkvref.so and oracle/_ref/libkvref_ht.so (the unmodified
reference sources, oracle/Makefile):

    python tests/golden/make_find_golden.py

It compiles tests/golden/find_driver.cpp (our text) against the reference's
headers and libkvref_ht.so into a temporary directory, fills one table per
entry of TABLES through the reference's write path (acquire / resize /
release, every 10th key then tombstoned) and records what the reference's
KeyCtx::find answers for the n inserted keys followed by n absent ones,
together with the whole ht[] image.  Only the .npz files are kept: data the
reference's programs wrote, no binary and no reference text.

Fields of find_<name>.npz:
  params   [slots, entry_size, buckets, arity, n_inserted]        u64
  geom     [ht_mod_mask, ht_mod_fraction, ht_mod_shift, ht_size]  u64
  image    ht[0 .. ht_size), ht_size x entry_size bytes           u8
  queries  (2n, 2) fixed-up (h1, h2): rows [0, n) were inserted in this
           order (the immediate value of row i is the u64 i), rows [n, 2n)
           never were                                             u64
  status, pos, chains, inc   KeyCtx::find per query (pos ~0: left unset)
  keys16, seed, keys16_q     16-byte keys whose fixed-up kv_hash_meow128
           under `seed` is queries[keys16_q[j]]
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from raikv_amd.workload import STATIC_SEED  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/Makefile
REFLIB = os.path.join(ROOT, "oracle", "_ref")
U64, P, SZ = C.c_uint64, C.c_void_p, C.c_size_t
KEY_OK, KEY_NOT_FOUND, KEY_BUSY, KEY_HT_FULL = 0, 2, 3, 5
NOPOS = np.uint64(2**64 - 1)
LIMIT = 512 << 10

# (name, slots, entry_size, buckets, arity, load, highest inc that must hold a KEY_OK)
TABLES = [
    ("600_8x8", 600, 64, 8, 8, 0.9, 4),
    ("5000_4x4", 5000, 64, 4, 4, 0.92, 3),
    ("4096_2x2", 4096, 64, 2, 2, 0.8, 1),
    ("600_2x5", 600, 64, 2, 5, 0.85, 4),
    ("3000_lin", 3000, 64, 1, 1, 0.8, 0),
    ("64_lin_full", 64, 64, 1, 1, 1.0, 0),
    ("2000_4x4_e128", 2000, 128, 4, 4, 0.92, 3),
]


def ptr(a):
    return a.ctypes.data_as(P)


def fixup(h):
    h = h.copy()
    h[:, 0] &= np.uint64((1 << 63) - 1)
    h[h[:, 0] <= 1, 0] = 2
    return h


def build_driver(tmp):
    so = os.path.join(tmp, "libfind_driver.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-mavx", "-maes", f"-I{REF}/include", "-include", "stdint.h",
                    "-include", "string.h", "-o", so, os.path.join(HERE, "find_driver.cpp"), f"-L{REFLIB}",
                    "-lkvref_ht", f"-Wl,-rpath,{REFLIB}", "-lpthread", "-lrt"], check=True)
    lib = C.CDLL(so)
    lib.ref_find_table.restype = C.c_long
    lib.ref_find_table.argtypes = [U64, C.c_uint32, C.c_uint16, C.c_uint8, P, SZ, C.c_uint32, P, SZ, P, P, P, P, P,
                                   SZ, P]
    return lib


def main():
    ref = C.CDLL(os.path.join(REFLIB, "libkvref.so"))
    ref.ref_batch_fixed.argtypes = [P, SZ, SZ, U64, U64, P]
    with tempfile.TemporaryDirectory() as tmp:
        drv = build_driver(tmp)
        for ti, (name, slots, es, buckets, arity, load, top_inc) in enumerate(TABLES):
            # a cuckoo table near its limit may refuse an insert (the path search gives up): draw the
            # inputs again from the next seed rather than lower the load
            for attempt in range(16):
                rng = np.random.default_rng(20261019 + ti + 100 * attempt)
                n = int(round(load * slots))
                n16 = min(n // 2, 256)  # real keys: n16 inserted + n16 absent
                kb = rng.integers(0, 256, size=2 * n16 * 16, dtype=np.uint8)
                hk = np.zeros((2 * n16, 2), dtype=np.uint64)
                ref.ref_batch_fixed(ptr(kb), 16, 2 * n16, U64(STATIC_SEED[0]), U64(STATIC_SEED[1]), ptr(hk))
                hk = fixup(hk)
                rnd = fixup(rng.integers(0, 2**64, size=(2 * (n - n16), 2), dtype=np.uint64))
                q = np.ascontiguousarray(np.concatenate([hk[:n16], rnd[:n - n16], hk[n16:], rnd[n - n16:]]))
                assert len(q) == 2 * n and len(np.unique(q[:, 0])) == 2 * n
                keys16_q = np.concatenate([np.arange(n16), n + np.arange(n16)]).astype(np.uint64)
                status = np.zeros(2 * n, np.int32)
                pos = np.zeros(2 * n, np.uint64)
                chains = np.zeros(2 * n, np.uint64)
                inc = np.zeros(2 * n, np.uint8)
                image = np.zeros(slots * es, np.uint8)
                geom = np.zeros(4, np.uint64)
                rc = drv.ref_find_table(slots, es, buckets, arity, ptr(q), n, 10, ptr(q), 2 * n, ptr(status), ptr(pos),
                                        ptr(chains), ptr(inc), ptr(image), image.size, ptr(geom))
                if not (-1000000 < rc <= -100):
                    break
            assert rc == slots, (name, rc)  # every insert KEY_IS_NEW, every tombstone KEY_OK
            img = image.reshape(slots, es)
            H = img.view(np.uint64)[:, 0]
            seal = (img.view(np.uint32)[:, es // 4 - 2] >> np.uint32(15)) & np.uint32(1)
            occ = H != 0
            # the conditions the tests rely on
            assert int(occ.sum()) == n, (name, int(occ.sum()), n)
            assert not (H & np.uint64(1 << 63)).any(), name
            assert seal[occ].all(), name
            ins, absent = slice(0, n), slice(n, 2 * n)
            tomb = np.zeros(2 * n, bool)
            tomb[0:n:10] = True
            assert (status[ins][~tomb[ins]] == KEY_OK).all(), name
            assert (status[ins][tomb[ins]] == KEY_NOT_FOUND).all() and (pos[ins][tomb[ins]] != NOPOS).all(), name
            ok = status == KEY_OK
            cuckoo = buckets > 1
            for k in range(top_inc + 1):
                assert (ok & (inc == k)).any(), (name, "no KEY_OK at inc", k)
            nf_abs = status[absent] == KEY_NOT_FOUND
            empty = nf_abs & (pos[absent] != NOPOS)
            exhausted = nf_abs & (pos[absent] == NOPOS)
            if load < 1.0:
                assert empty.any(), (name, "no empty-slot miss")
                assert (H[pos[absent][empty]] == 0).all(), name
            if cuckoo:
                assert exhausted.any(), (name, "no exhausted miss")
                assert (chains[absent][exhausted] == buckets * arity).all(), name
            else:
                assert not exhausted.any(), name
            if load >= 1.0:
                assert (status[absent] == KEY_HT_FULL).all() and (chains[absent] == slots).all(), name
            assert not (status == KEY_BUSY).any(), name
            out = os.path.join(HERE, f"find_{name}.npz")
            np.savez_compressed(out, params=np.array([slots, es, buckets, arity, n], dtype=np.uint64), geom=geom,
                                image=img, queries=q, status=status, pos=pos, chains=chains, inc=inc,
                                keys16=kb, seed=np.array(STATIC_SEED, dtype=np.uint64), keys16_q=keys16_q)
            assert os.path.getsize(out) < LIMIT, (name, os.path.getsize(out))
            print(f"find_{name}: ht_size {int(geom[3])} inserted {n} ok-by-inc",
                  [int((ok & (inc == k)).sum()) for k in range(max(arity, 1))], "empty", int(empty.sum()),
                  "exhausted", int(exhausted.sum()), "ht_full", int((status == KEY_HT_FULL).sum()),
                  "max chains", int(chains.max()), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
