#!/usr/bin/env python3
"""Generate tests/golden/get_*.npz from the REFERENCE itself.

Run where the reference tree exists, after `make` has built
oracle/_ref/libkvref_ht.so (the unmodified reference sources, oracle/Makefile):

    python tests/golden/make_get_golden.py

It compiles tests/golden/get_driver.cpp (our text) against the reference's
headers and libkvref_ht.so into a temporary directory, fills one table WITH
DATA SEGMENTS per entry of TABLES through the reference's write path and
records what the reference's KeyCtx::find + KeyCtx::value answer for the n
inserted keys followed by n absent ones, together with the ht[] image and the
segment area.  Only the .npz files are kept: data the reference's programs
wrote, no binary and no reference text.

Write steps (key i has the 8-byte key u64 i; SIZES straddles the immediate
capacity of both entry sizes, with and without a stamp):
  insert     every key, size1[i] bytes, byte j = (u8)(i * 131 + j)
  resize     every 3rd key to size2[i] != size1[i], byte j = (u8)(i * 131 + j + 1):
             leaves released messages behind and switches entries between
             immediate and segment in both directions
  stamp      every 4th key: update_stamps(0, t) moves the ValuePtr and pushes
             the largest immediate values out into a segment
  tombstone  every 10th key
The segment a context allocates from is drawn from /dev/urandom, so a
regenerated fixture differs in placement; the committed record is the fixture.

Fields of get_<name>.npz:
  params   [map_size, entry_size, buckets, arity, n_inserted, max_value_size]  u64
  ratio    hash_value_ratio                                          f32
  geom     [ht_mod_mask, ht_mod_fraction, ht_mod_shift, ht_size]     u64
  seg      [nsegs, seg_size, seg_start, seg_align_shift]             u64
  image    ht[0 .. ht_size), ht_size x entry_size bytes              u8
  segments map bytes [seg_start, seg_start + nsegs x seg_size)       u8
  queries  (2n, 2) fixed-up (h1, h2): rows [0, n) inserted in this order,
           rows [n, 2n) never were                                   u64
  status, pos, chains, inc   KeyCtx::find per query (pos ~0: left unset)
  vstatus, vsize             KeyCtx::value after a KEY_OK find (-1, 0: not called)
  vloc     where value()'s pointer points: bit 63 set = offset into
           `segments`, clear = offset into `image`; ~0 without a value  u64
  blob, blob_offs            the value bytes of query i: blob[offs[i] : offs[i + 1]]
  size1, size2, flags3       the sizes written; the entry's flags after
                             insert / resize / stamp
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")  # as oracle/Makefile
REFLIB = os.path.join(ROOT, "oracle", "_ref")
P, SZ = C.c_void_p, C.c_size_t
KEY_OK, KEY_NOT_FOUND, KEY_BUSY, KEY_MUTATED, KEY_NO_VALUE = 0, 2, 3, 6, 8
FL_SEGMENT_VALUE, FL_IMMEDIATE_VALUE, FL_STAMPS = 0x40, 0x100, 0x3000
NOPOS = np.uint64(2**64 - 1)
SEGBIT = np.uint64(1 << 63)
LIMIT = 512 << 10
HDR = 458752  # KV_HT_HDR_SIZE + KV_HT_CTX_SIZE + KV_HT_STATS_SIZE

SIZES = [0, 1, 7, 8, 15, 16, 17, 24, 25, 32, 33, 63, 64, 65, 80, 81, 88, 89, 100, 255, 256, 1000, 4000]
MAP = HDR + 64000 + 262144
RATIO = np.float32(64000.0 / 326144.0)
# (name, map_size, entry_size, buckets, arity, keys, max_value_size)
TABLES = [
    ("999_4x4", MAP, 64, 4, 4, 180, 4096),
    ("499_lin_e128", MAP, 128, 1, 1, 180, 4096),
    ("999_2x2", MAP, 64, 2, 2, 180, 4096),
]
RESIZE_EVERY, STAMP_EVERY, TOMB_EVERY = 3, 4, 10


class GetTable(C.Structure):
    _fields_ = [("map_size", C.c_uint64), ("max_value_size", C.c_uint32), ("entry_size", C.c_uint32),
                ("ratio", C.c_float), ("buckets", C.c_uint16), ("arity", C.c_uint8), ("resize_every", C.c_uint32),
                ("stamp_every", C.c_uint32), ("tomb_every", C.c_uint32)]


def ptr(a):
    return a.ctypes.data_as(P)


def fixup(h):
    h = h.copy()
    h[:, 0] &= np.uint64((1 << 63) - 1)
    h[h[:, 0] <= 1, 0] = 2
    return h


def build_driver(tmp):
    so = os.path.join(tmp, "libget_driver.so")
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-mavx", "-maes", f"-I{REF}/include", "-include", "stdint.h",
                    "-include", "string.h", "-o", so, os.path.join(HERE, "get_driver.cpp"), f"-L{REFLIB}",
                    "-lkvref_ht", f"-Wl,-rpath,{REFLIB}", "-lpthread", "-lrt"], check=True)
    lib = C.CDLL(so)
    lib.ref_get_table.restype = C.c_long
    lib.ref_get_table.argtypes = [P, P, SZ, P, P, P, SZ, P, P, P, P, P, P, P, P, SZ, P, P, P, SZ, P, SZ, P]
    return lib


def pattern(i, size, pas):
    return ((i * 131 + np.arange(size) + pas) & 0xFF).astype(np.uint8)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        drv = build_driver(tmp)
        for ti, (name, map_size, es, buckets, arity, n, maxv) in enumerate(TABLES):
            rng = np.random.default_rng(20261019 + ti)
            q = np.ascontiguousarray(fixup(rng.integers(0, 2**64, size=(2 * n, 2), dtype=np.uint64)))
            assert len(np.unique(q[:, 0])) == 2 * n
            # every size occurs in both passes; a resized key never keeps its size
            size1 = np.array([SIZES[(i + ti) % len(SIZES)] for i in range(n)], np.uint32)
            size2 = np.array([SIZES[(i // RESIZE_EVERY * 7 + 11 + ti) % len(SIZES)] for i in range(n)], np.uint32)
            same = size2 == size1
            size2[same] = np.array([SIZES[(SIZES.index(int(s)) + 5) % len(SIZES)] for s in size2[same]], np.uint32)
            t = GetTable(map_size, maxv, es, float(RATIO), buckets, arity, RESIZE_EVERY, STAMP_EVERY, TOMB_EVERY)
            status = np.zeros(2 * n, np.int32)
            pos = np.zeros(2 * n, np.uint64)
            chains = np.zeros(2 * n, np.uint64)
            inc = np.zeros(2 * n, np.uint8)
            vstatus = np.zeros(2 * n, np.int32)
            vsize = np.zeros(2 * n, np.uint64)
            vloc = np.zeros(2 * n, np.uint64)
            blob = np.zeros(n * max(SIZES), np.uint8)
            offs = np.zeros(2 * n + 1, np.uint64)
            flags3 = np.zeros((n, 3), np.uint16)
            image = np.zeros(map_size - HDR, np.uint8)
            segs = np.zeros(map_size - HDR, np.uint8)
            hdr = np.zeros(8, np.uint64)
            rc = drv.ref_get_table(C.byref(t), ptr(q), n, ptr(size1), ptr(size2), ptr(q), 2 * n, ptr(status), ptr(pos),
                                   ptr(chains), ptr(inc), ptr(vstatus), ptr(vsize), ptr(vloc), ptr(blob), blob.size,
                                   ptr(offs), ptr(flags3), ptr(image), image.size, ptr(segs), segs.size, ptr(hdr))
            slots, nsegs, seg_size, seg_start, shift = int(hdr[3]), int(hdr[4]), int(hdr[5]), int(hdr[6]), int(hdr[7])
            assert rc == slots and rc > 0, (name, rc)  # every write step ended KEY_OK (KEY_IS_NEW for an insert)
            assert nsegs > 0 and seg_start == HDR + slots * es and seg_start + nsegs * seg_size <= map_size, name
            img = image[:slots * es].reshape(slots, es)
            sg = segs[:nsegs * seg_size]
            blob = blob[:int(offs[-1])]
            # ---- the conditions the tests rely on
            ins = np.arange(n)
            tomb = ins % TOMB_EVERY == 0
            resized = ins % RESIZE_EVERY == 0
            assert (status[:n][~tomb] == KEY_OK).all() and (vstatus[:n][~tomb] == KEY_OK).all(), name
            assert (status[:n][tomb] == KEY_NOT_FOUND).all() and (pos[:n][tomb] != NOPOS).all(), name
            assert (status[n:] != KEY_OK).all() and (vstatus[n:] == -1).all(), name
            for bad in (KEY_MUTATED, KEY_NO_VALUE, KEY_BUSY):
                assert not (status == bad).any() and not (vstatus == bad).any(), (name, bad)
            final = np.where(resized, size2, size1)
            assert (vsize[:n][~tomb] == final[~tomb]).all(), name
            for i in np.flatnonzero(~tomb):  # every find + value returned the written bytes, and points at them
                want = pattern(int(i), int(final[i]), 1 if resized[i] else 0)
                got = blob[int(offs[i]):int(offs[i + 1])]
                assert np.array_equal(got, want), (name, i)
                loc = int(vloc[i])
                src = sg if loc >> 63 else image
                o = loc & ((1 << 63) - 1)
                assert np.array_equal(src[o:o + len(want)], want), (name, i, "location")
            fl = img.view(np.uint16)[pos[:n][~tomb].astype(np.int64), 10]
            imm, seg, st = (fl & FL_IMMEDIATE_VALUE) != 0, (fl & FL_SEGMENT_VALUE) != 0, (fl & FL_STAMPS) != 0
            assert (imm ^ seg).all(), name
            for kind, kn in ((imm, "immediate"), (seg, "segment")):
                assert (kind & st).any() and (kind & ~st).any(), (name, kn, "with and without stamps")
            k1, k2, k3 = (flags3[:, j] & (FL_IMMEDIATE_VALUE | FL_SEGMENT_VALUE) for j in range(3))
            assert ((k1 == FL_IMMEDIATE_VALUE) & (k2 == FL_SEGMENT_VALUE)).any(), (name, "no immediate -> segment")
            assert ((k1 == FL_SEGMENT_VALUE) & (k2 == FL_IMMEDIATE_VALUE)).any(), (name, "no segment -> immediate")
            pushed = int(((k2 == FL_IMMEDIATE_VALUE) & (k3 == FL_SEGMENT_VALUE)).sum())
            assert pushed > 0, (name, "no value pushed out by a stamp")
            assert ((vloc[:n][~tomb] & SEGBIT) != 0).any() and ((vloc[:n][~tomb] & SEGBIT) == 0).any(), name
            out = os.path.join(HERE, f"get_{name}.npz")
            np.savez_compressed(out, params=np.array([map_size, es, buckets, arity, n, maxv], dtype=np.uint64),
                                ratio=np.array([RATIO], np.float32), geom=hdr[:4].copy(),
                                seg=np.array([nsegs, seg_size, seg_start, shift], np.uint64), image=img, segments=sg,
                                queries=q, status=status, pos=pos, chains=chains, inc=inc, vstatus=vstatus, vsize=vsize,
                                vloc=vloc, blob=blob, blob_offs=offs, size1=size1, size2=size2, flags3=flags3)
            assert os.path.getsize(out) < LIMIT, (name, os.path.getsize(out))
            print(f"get_{name}: ht_size {slots} nsegs {nsegs} x {seg_size} shift {shift} inserted {n}",
                  "immediate", int(imm.sum()), "segment", int(seg.sum()), "stamped", int(st.sum()),
                  "pushed out by a stamp", pushed, "max chains", int(chains.max()), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
