"""Model of the batched find over a raikv hash-table image (kvh_ht_find):
KeyCtx::find<Position> (include/raikv/ht_search.h:308-367) restated for one
key on a table image that cannot change, in numpy / Python.  The probe
positions come from the clean-room position oracle (oracle/cuckoo_oracle.c
through oracle_lib.orc_positions).  tests/test_find_model.py pins this model
to the reference's own find on every fixture of tests/golden/find_*.npz; the
GPU tests then use it for the states the reference cannot answer.

Walk (h1, h2 fixed up as KeyFragment::hash leaves them):
  pos = ht_mod(h1); chains = inc = boff = 0
  h = entry[pos].hash
    h == h1, sealed, hash2 == h2  -> KEY_NOT_FOUND if FL_DROPPED else KEY_OK, at pos
    h == h1, seal clear           -> KEY_BUSY     (the reference spins)
    h == h1, sealed, hash2 != h2  -> go on
    h == 0                        -> KEY_NOT_FOUND at pos
    h & ZOMBIE64                  -> KEY_BUSY     (the reference spins)
    else                          -> go on
  go on: ++chains, ++pos (wraps at ht_size);
    linear (cuckoo_buckets <= 1): chains == ht_size -> KEY_HT_FULL
    cuckoo: ++boff == buckets -> ++inc == arity -> KEY_NOT_FOUND
                                 else pos = CuckooAltHash::pos[inc], boff = 0
`inc` is KeyCtx::inc, the number of the last window searched: it stays at
arity - 1 when the windows run out (CuckooPosition::next_hash,
src/ht_cuckoo.cpp:488-507, sets kctx.inc only when it moves on).
pos is ~0 when the walk ended without a slot.
"""
import numpy as np

KEY_OK, KEY_NOT_FOUND, KEY_BUSY, KEY_HT_FULL = 0, 2, 3, 5
FL_IMMEDIATE_VALUE, FL_DROPPED = 0x100, 0x800
ZOMBIE64 = 1 << 63
NOPOS = 2**64 - 1
VALUE_OFF = 32  # immediate value of an entry whose key fragment has keylen 8 (hdr_size 24 + 8)


def geom_from_fields(oracle_lib, geom4, buckets, arity):
    """OrcGeom from a fixture's (ht_mod_mask, ht_mod_fraction, ht_mod_shift, ht_size)."""
    g = oracle_lib.OrcGeom()
    g.ht_mod_mask, g.ht_mod_fraction, g.ht_mod_shift, g.ht_size = (int(x) for x in geom4)
    g.cuckoo_buckets, g.cuckoo_arity = int(buckets), int(arity)
    return g


def image_fields(image, es):
    """(hash, hash2, flags, sealed) columns of an image of ht_size rows of es bytes."""
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1, es)
    w = img.view(np.uint64)
    flags = img.view(np.uint16)[:, 10]
    sealed = (img.view(np.uint32)[:, es // 4 - 2] >> np.uint32(15)) & np.uint32(1)
    return w[:, 0], w[:, 1], flags, sealed.astype(bool)


def find_model(orc, oracle_lib, g, image, es, hashes):
    """-> (status i32 [n], pos u64 [n], chains u64 [n], inc u8 [n], probed: list of slot lists)."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, 2)
    n = len(h)
    H, H2, FL, SEAL = image_fields(image, es)
    size = int(g.ht_size)
    assert len(H) == size
    B = int(g.cuckoo_buckets)
    linear = B <= 1
    A = max(int(g.cuckoo_arity), 1)
    P = oracle_lib.orc_positions(orc, g, h) if n else np.zeros((0, 1), np.uint64)
    status = np.zeros(n, np.int32)
    pos_o = np.full(n, NOPOS, np.uint64)
    chains_o = np.zeros(n, np.uint64)
    inc_o = np.zeros(n, np.uint8)
    probed = []
    for i in range(n):
        h1, h2 = int(h[i, 0]), int(h[i, 1])
        pos, chains, inc, boff = int(P[i, 0]), 0, 0, 0
        seen = []
        while True:
            seen.append(pos)
            e = int(H[pos])
            st = None
            if e == h1:
                if not SEAL[pos]:
                    st, pos = KEY_BUSY, NOPOS
                elif int(H2[pos]) == h2:
                    st = KEY_NOT_FOUND if int(FL[pos]) & FL_DROPPED else KEY_OK
            elif e == 0:
                st = KEY_NOT_FOUND
            elif e & ZOMBIE64:
                st, pos = KEY_BUSY, NOPOS
            if st is None:
                chains += 1
                pos = pos + 1 if pos + 1 < size else 0
                if linear:
                    if chains == size:
                        st, pos = KEY_HT_FULL, NOPOS
                else:
                    boff += 1
                    if boff == B:
                        if inc + 1 == A:
                            st, pos = KEY_NOT_FOUND, NOPOS
                        else:
                            inc += 1
                            pos, boff = int(P[i, inc]), 0
            if st is not None:
                status[i], pos_o[i], chains_o[i], inc_o[i] = st, pos, chains, inc
                break
        probed.append(seen)
    return status, pos_o, chains_o, inc_o, probed


def pack_res(status, chains, inc):
    """res[i] of kvh_ht_find: status | inc << 8 | min(chains, 0xFFFF) << 16."""
    c = np.minimum(np.asarray(chains, np.uint64), np.uint64(0xFFFF)).astype(np.uint32)
    return np.asarray(status).astype(np.uint32) | (np.asarray(inc).astype(np.uint32) << np.uint32(8)) | (
        c << np.uint32(16))


def make_entry(es, h1, h2, inc, value):
    """A sealed entry with an 8-byte immediate value (keylen-8 layout)."""
    e = np.zeros(es, np.uint8)
    e.view(np.uint64)[0] = h1
    e.view(np.uint64)[1] = h2
    e.view(np.uint16)[10] = FL_IMMEDIATE_VALUE | (inc & 7)
    e.view(np.uint16)[11] = 8  # keylen
    e.view(np.uint64)[VALUE_OFF // 8] = value
    e.view(np.uint32)[es // 4 - 2] = 8 | (1 << 15)  # ValueCtr: size 8, seal
    return e


def build_image(orc, oracle_lib, g, es, hashes):
    """Place every pair in the first free slot of its windows (the walk's
    order), value = its index.  -> (image u8 [ht_size, es], placed bool [n])."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, 2)
    size, B = int(g.ht_size), int(g.cuckoo_buckets)
    linear = B <= 1
    img = np.zeros((size, es), np.uint8)
    used = np.zeros(size, bool)
    P = oracle_lib.orc_positions(orc, g, h)
    placed = np.zeros(len(h), bool)
    for i in range(len(h)):
        if linear:
            cand = (((int(P[i, 0]) + k) % size, 0) for k in range(size))
        else:
            cand = (((int(p) + k) % size, a) for a, p in enumerate(P[i]) for k in range(B))
        for s, a in cand:
            if not used[s]:
                used[s] = True
                img[s] = make_entry(es, int(h[i, 0]), int(h[i, 1]), a, i)
                placed[i] = True
                break
    return img, placed


def find_fixtures():
    """tests/golden/find_*.npz (tests/golden/make_find_golden.py) as dicts."""
    import glob
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = []
    for f in sorted(glob.glob(os.path.join(here, "find_*.npz"))):
        d = np.load(f)
        slots, es, b, a, n = (int(x) for x in d["params"])
        out.append(dict(name=os.path.basename(f)[5:-4], slots=slots, es=es, buckets=b, arity=a, n=n, geom=d["geom"],
                        image=d["image"], queries=d["queries"], status=d["status"], pos=d["pos"], chains=d["chains"],
                        inc=d["inc"], keys16=d["keys16"], seed=tuple(int(x) for x in d["seed"]),
                        keys16_q=d["keys16_q"].astype(np.int64)))
    return out
