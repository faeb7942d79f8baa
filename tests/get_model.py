"""Model of the batched get over raikv table images (kvh_ht_get):
KeyCtx::find followed by KeyCtx::value (src/key_ctx.cpp:959-1001) restated for
one key on images that cannot change, in numpy / Python, on top of
find_model.find_model.  tests/test_get_model.py pins this model to the
reference's own find + value on every fixture of tests/golden/get_*.npz; the
GPU tests then use it for the states the reference cannot answer.

After a find that ends KEY_OK at entry e (es bytes), with fl = u16 at +20:
  fl & (FL_SEGMENT_VALUE | FL_IMMEDIATE_VALUE)
    neither / both -> KEY_NO_VALUE
    immediate      -> size = low 15 bits of the u32 at es - 8; data at 24 when
                      FL_PART_KEY else 24 + align8(keylen u16 at +22)
                      [bounded: offset + size > es - 8 -> KEY_MUTATED]
    segment        -> ValuePtr (u16 segment, u16 serialhi, u32 seriallo, u32
                      size, u32 offset) at es - 24, - 8 with a stamp, - 8 with
                      FL_SEQNO; size, offset << seg_align_shift
                      segment >= nsegs or offset >= seg_size -> KEY_MUTATED
                      [bounded: size < 48 or offset + size > seg_size -> KEY_MUTATED]
                      message m at segment * seg_size + offset; check_seal:
                        m.size (u32 +0) == size, m.hash (+8) == h1, m.hash2
                        (+16) == h2, m.flags (u16 +30) & FL_BUSY == 0, trailer
                        ValueCtr at size - 8: seriallo, serialhi equal, seal
                        set; m.seriallo (u32 +24) == seriallo
                      else KEY_MUTATED
                      size = m.msg_size (u32 +4), data at align8(34 + keylen
                      u16 at +32)
                      [bounded: data offset + msg_size + 8 > m.size -> KEY_MUTATED]
A find status other than KEY_OK is the status; there is no value.
val_loc: bit 63 set = offset into the segment image, clear = into the entry
image; ~0 without a value.
"""
import glob
import os

import numpy as np

import find_model as fm

KEY_OK, KEY_MUTATED, KEY_NO_VALUE = 0, 6, 8
FL_SEQNO, FL_SEGMENT_VALUE, FL_IMMEDIATE_VALUE, FL_PART_KEY = 0x10, 0x40, 0x100, 0x400
FL_STAMPS, FL_BUSY = 0x3000, 0x8000
SEGBIT = 1 << 63
NOLOC = 2**64 - 1
MSG_HEAD = 48


def align8(x):
    return (x + 7) & ~7


def u16(b, o):
    return int(b[o]) | int(b[o + 1]) << 8


def u32(b, o):
    return int.from_bytes(bytes(b[o:o + 4]), "little")


def u64(b, o):
    return int.from_bytes(bytes(b[o:o + 8]), "little")


def value_ptr_offset(fl, es):
    """HashEntry::value_ptr (hash_entry.h:333-340)"""
    return es - 24 - (8 if fl & FL_STAMPS else 0) - (8 if fl & FL_SEQNO else 0)


def value_model(e, es, slot, segs, nsegs, seg_size, shift, h1, h2):
    """KeyCtx::value for the sealed entry bytes e matched to (h1, h2).
    -> (status, size, loc)"""
    fl, keylen = u16(e, 20), u16(e, 22)
    kind = fl & (FL_SEGMENT_VALUE | FL_IMMEDIATE_VALUE)
    if kind == FL_IMMEDIATE_VALUE:
        size = u32(e, es - 8) & 0x7FFF
        off = 24 if fl & FL_PART_KEY else 24 + align8(keylen)
        if off + size > es - 8:
            return KEY_MUTATED, 0, NOLOC
        return KEY_OK, size, slot * es + off
    if kind != FL_SEGMENT_VALUE:
        return KEY_NO_VALUE, 0, NOLOC
    vp = value_ptr_offset(fl, es)
    segment, serialhi, seriallo = u16(e, vp), u16(e, vp + 2), u32(e, vp + 4)
    gsize, goff = u32(e, vp + 8) << shift, u32(e, vp + 12) << shift
    if segment >= nsegs or goff >= seg_size:
        return KEY_MUTATED, 0, NOLOC
    if gsize < MSG_HEAD or goff + gsize > seg_size:
        return KEY_MUTATED, 0, NOLOC
    mo = segment * seg_size + goff
    m = segs[mo:mo + gsize]
    if u32(m, 0) != gsize or u64(m, 8) != h1 or u64(m, 16) != h2 or u16(m, 30) & FL_BUSY:
        return KEY_MUTATED, 0, NOLOC
    t0, t1 = u32(m, gsize - 8), u32(m, gsize - 4)
    if t1 != seriallo or (t0 >> 16) != serialhi or not (t0 & 0x8000) or u32(m, 24) != seriallo:
        return KEY_MUTATED, 0, NOLOC
    msg_size, doff = u32(m, 4), align8(34 + u16(m, 32))
    if doff + msg_size + 8 > gsize:
        return KEY_MUTATED, 0, NOLOC
    return KEY_OK, msg_size, SEGBIT | (mo + doff)


def get_model(orc, oracle_lib, g, image, es, segments, seg, hashes):
    """seg = (nsegs, seg_size, seg_align_shift).  -> dict: status i32 (the
    combined one), pos u64, chains u64, inc u8, vlen u32, vloc u64, values
    (list of bytes), probed (find_model's)."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, 2)
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1, es)
    segs = np.zeros(0, np.uint8) if segments is None else np.ascontiguousarray(segments, dtype=np.uint8).reshape(-1)
    nsegs, seg_size, shift = (int(x) for x in seg)
    assert len(segs) == nsegs * seg_size
    status, pos, chains, inc, probed = fm.find_model(orc, oracle_lib, g, img, es, h)
    status = status.copy()
    n = len(h)
    vlen = np.zeros(n, np.uint32)
    vloc = np.full(n, NOLOC, np.uint64)
    values = [b""] * n
    flat = img.reshape(-1)
    for i in np.flatnonzero(status == fm.KEY_OK):
        slot = int(pos[i])
        st, size, loc = value_model(img[slot], es, slot, segs, nsegs, seg_size, shift, int(h[i, 0]), int(h[i, 1]))
        status[i] = st
        if st == KEY_OK:
            vlen[i], vloc[i] = size, loc
            src, o = (segs, loc & (SEGBIT - 1)) if loc & SEGBIT else (flat, loc)
            values[i] = bytes(src[o:o + size])
            assert len(values[i]) == size
    return dict(status=status, pos=pos, chains=chains, inc=inc, vlen=vlen, vloc=vloc, values=values, probed=probed)


def rows_of(values, stride):
    """values_out of kvh_ht_get: row i = the first min(len, stride) bytes, then zeros."""
    rows = np.zeros((len(values), stride), np.uint8)
    for i, v in enumerate(values):
        k = min(len(v), stride)
        rows[i, :k] = np.frombuffer(v[:k], np.uint8)
    return rows


def fixture_values(f):
    """the value bytes the reference returned per query of a get fixture"""
    o = f["blob_offs"].astype(np.int64)
    b = f["blob"]
    return [bytes(b[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def fixture_status(f):
    """the combined status: find's, or value()'s after a KEY_OK find"""
    return np.where(f["status"] == fm.KEY_OK, f["vstatus"], f["status"]).astype(np.int32)


def get_fixtures():
    """tests/golden/get_*.npz (tests/golden/make_get_golden.py) as dicts."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = []
    for p in sorted(glob.glob(os.path.join(here, "get_*.npz"))):
        d = np.load(p)
        map_size, es, b, a, n, maxv = (int(x) for x in d["params"])
        nsegs, seg_size, seg_start, shift = (int(x) for x in d["seg"])
        f = dict(name=os.path.basename(p)[4:-4], map_size=map_size, es=es, buckets=b, arity=a, n=n, max_value=maxv,
                 ratio=float(d["ratio"][0]), nsegs=nsegs, seg_size=seg_size, seg_start=seg_start, shift=shift)
        for k in ("geom", "image", "segments", "queries", "status", "pos", "chains", "inc", "vstatus", "vsize", "vloc",
                  "blob", "blob_offs", "size1", "size2", "flags3"):
            f[k] = d[k]
        f["seg"] = (nsegs, seg_size, shift)
        out.append(f)
    return out


# ------------------------------------------------------------ model-only states
def _put(buf, o, val, nbytes):
    buf[o:o + nbytes] = np.frombuffer(int(val).to_bytes(nbytes, "little"), np.uint8)


def mutated_images(f, per_state=4, seed=7):
    """Copies of a get fixture's images with single fields changed, a few
    keys per state: the states the reference would report KEY_MUTATED /
    KEY_NO_VALUE for or spin on, and the bounded divergences.
    -> (image, segments, {state: (query indices, expected status)})"""
    es, (nsegs, seg_size, shift) = f["es"], f["seg"]
    img = f["image"].copy()
    segs = f["segments"].copy()
    flat = img.reshape(-1)
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(fixture_status(f) == KEY_OK)
    in_seg = (f["vloc"][ok] & np.uint64(SEGBIT)) != 0
    S = list(rng.permutation(ok[in_seg]))
    I = list(rng.permutation(ok[~in_seg]))
    states = {}

    def take(pool, name, status):
        idx = np.array([pool.pop() for _ in range(per_state)], np.int64)
        states[name] = (idx, status)
        return idx

    def entry_off(i):
        return int(f["pos"][i]) * es

    def msg_of(i):
        """(entry offset of the ValuePtr, message offset in segs, message size)"""
        e = entry_off(i)
        vp = e + value_ptr_offset(u16(flat, e + 20), es)
        gsize, goff = u32(flat, vp + 8) << shift, u32(flat, vp + 12) << shift
        return vp, u16(flat, vp) * seg_size + goff, gsize

    for i in take(S, "msg_busy", KEY_MUTATED):
        _, m, _ = msg_of(i)
        _put(segs, m + 30, u16(segs, m + 30) | FL_BUSY, 2)
    for i in take(S, "trailer_serial", KEY_MUTATED):
        _, m, sz = msg_of(i)
        _put(segs, m + sz - 4, u32(segs, m + sz - 4) ^ 1, 4)
    for i in take(S, "msg_seriallo", KEY_MUTATED):
        _, m, _ = msg_of(i)
        _put(segs, m + 24, u32(segs, m + 24) ^ 1, 4)
    for i in take(S, "trailer_seal", KEY_MUTATED):
        _, m, sz = msg_of(i)
        _put(segs, m + sz - 8, u32(segs, m + sz - 8) & ~0x8000, 4)
    for i in take(S, "msg_size_field", KEY_MUTATED):
        _, m, sz = msg_of(i)
        _put(segs, m, sz + (1 << shift), 4)
    for i in take(S, "msg_hash2", KEY_MUTATED):
        _, m, _ = msg_of(i)
        _put(segs, m + 16, u64(segs, m + 16) ^ 1, 8)
    for i in take(S, "segment_past_nsegs", KEY_MUTATED):
        vp, _, _ = msg_of(i)
        _put(flat, vp, nsegs, 2)
    for i in take(S, "offset_past_seg_size", KEY_MUTATED):
        vp, _, _ = msg_of(i)
        _put(flat, vp + 12, seg_size >> shift, 4)
    for i in take(S, "message_past_last_segment", KEY_MUTATED):
        vp, _, _ = msg_of(i)
        _put(flat, vp, nsegs - 1, 2)
        _put(flat, vp + 8, 2, 4)                                # two alignment units ...
        _put(flat, vp + 12, (seg_size >> shift) - 1, 4)         # ... from the last one of the last segment
    for i in take(S, "msg_size_past_message", KEY_MUTATED):
        _, m, sz = msg_of(i)
        _put(segs, m + 4, sz, 4)
    for i in take(I, "both_value_bits", KEY_NO_VALUE):
        e = entry_off(i)
        _put(flat, e + 20, u16(flat, e + 20) | FL_SEGMENT_VALUE | FL_IMMEDIATE_VALUE, 2)
    for i in take(I, "no_value_bits", KEY_NO_VALUE):
        e = entry_off(i)
        _put(flat, e + 20, u16(flat, e + 20) & ~(FL_SEGMENT_VALUE | FL_IMMEDIATE_VALUE), 2)
    for i in take(I, "immediate_past_entry", KEY_MUTATED):
        e = entry_off(i)
        _put(flat, e + es - 8, (u32(flat, e + es - 8) & ~0x7FFF) | es, 4)
    for i in take(I, "entry_seal_clear", fm.KEY_BUSY):
        e = entry_off(i)
        _put(flat, e + es - 8, u32(flat, e + es - 8) & ~0x8000, 4)
    return img, segs, states
