#!/usr/bin/env python3
"""Time the batched get (kvh_ht_get) on table images at scale, beside
kvh_ht_find + gather on the same image and queries in the same run -- the
floor: get does that work plus the dependent reads of the value.  Needs an
MI355X.

    python tools/get_time.py [--log2-slots 24] [--n 100000000] [--loads 0.5,0.9] [--out FILE]

The ht[] image and the queries are tools/find_time.py's (the model's
placement rule, half of the queries present).  Two value mixes per load:

  imm8     every value the 8-byte immediate the image was built with, no
           segments (nsegs = 0), stride 16
  seg      half of the placed keys get a segment value of 64..256 bytes,
           stride 256.  The segment image is written from the model's layout
           (tests/get_model.py): per value one message of align64(48 + len + 16)
           bytes -- MsgHdr with an 8-byte key, the data, a stamp slot, the
           trailer ValueCtr -- packed in key order into 64 MiB segments; the
           entry's FL_IMMEDIATE_VALUE becomes FL_SEGMENT_VALUE and its
           ValuePtr (at es - 24) points at the message.  Data bytes are a
           pattern that goes on past the value's end, so a copy that does
           not mask its last word shows in the spot check.

20k results of each mix are spot-checked against tests/get_model.py.  Times
are HIP events around the call on the current stream (median of --iters
after --warmup).  touched bytes are counted as for find: 64 B per entry head
the walk compared, plus the 64-byte lines the value phase reads -- the entry
again for an immediate value (as find's gather counts its row), and for a
segment value the lines of the message header + data and the trailer's line.
Rows written are not counted (n x stride bytes, in order).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import raikv_amd as kvh  # noqa: E402
from find_time import DEV, HDR, SEED, build_image, timed  # noqa: E402

SEG_SIZE = 64 << 20
SHIFT = 6
MAX_ALLOC = 320  # align64(48 + 256 + 16)


def add_segment_values(image, es, slots, gen):
    """Move the values of half of the entries at `slots` into a new segment
    image.  -> (segments uint8 [nsegs * SEG_SIZE], SegGeom, count)"""
    pick = slots[torch.rand((slots.numel(),), device=DEV, generator=gen) < 0.5]
    k = pick.numel()
    vlen = torch.randint(64, 257, (k,), device=DEV, generator=gen)
    alloc = (48 + vlen + 16 + 63) & ~63
    per = SEG_SIZE // MAX_ALLOC  # messages per segment: a message never straddles two
    seg = torch.arange(k, device=DEV) // per
    nsegs = int(seg.max()) + 1 if k else 1
    assert nsegs <= 65536
    start = torch.cumsum(alloc, 0) - alloc
    off = start - start[seg * per]
    assert int((off + alloc).max()) <= SEG_SIZE
    mw = (seg * SEG_SIZE + off) // 8  # message offsets in u64 words
    words = nsegs * (SEG_SIZE // 8)
    sw = torch.arange(words, device=DEV, dtype=torch.int64) * -7046029254386353131 + 0x0123456789ABCDEF  # pattern
    w = image.view(torch.int64).view(-1, es // 8)
    h1, h2, idx = w[pick, 0], w[pick, 1], w[pick, 4]
    serlo, serhi = (idx & 0x3FFFFFFF) + 1, 1
    fl = ((w[pick, 2] >> 32) & 0xFFFF & ~0x100) | 0x40
    sw[mw + 0] = alloc | (vlen << 32)                      # size, msg_size
    sw[mw + 1] = h1
    sw[mw + 2] = h2
    sw[mw + 3] = serlo | (fl << 48)                        # seriallo, db 0, type 0, flags
    sw[mw + 4] = 8 | ((idx & 0xFFFFFFFFFFFF) << 16)        # keylen 8, key bytes 0-5
    sw[mw + 5] = (idx >> 48) & 0xFFFF                      # key bytes 6-7, pad: the data starts at +48
    sw[mw + alloc // 8 - 1] = 0x8000 | (serhi << 16) | (serlo << 32)  # trailer ValueCtr: seal, serial
    w[pick, 2] = (w[pick, 2] & ~(0xFFFF << 32)) | (fl << 32)
    w[pick, es // 8 - 3] = seg | (serhi << 16) | (serlo << 32)      # ValuePtr: segment, serialhi, seriallo
    w[pick, es // 8 - 2] = (alloc >> SHIFT) | ((off >> SHIFT) << 32)  # size, offset in alignment units
    return sw.view(torch.uint8), kvh.SegGeom(SEG_SIZE, nsegs, SHIFT), k


def spot_check(g, sg, es, image, segs, hashes, got, stride, count, gen):
    import oracle_lib
    import find_model as fm
    import get_model as gm
    orc = oracle_lib.load_oracle()
    og = oracle_lib.OrcGeom()
    for k in ("ht_size", "ht_mod_mask", "ht_mod_fraction", "ht_mod_shift", "cuckoo_buckets", "cuckoo_arity"):
        setattr(og, k, getattr(g, k))
    pos, res, vlen, vloc, rows = got
    idx = torch.randint(0, hashes.shape[0], (count,), device=DEV, generator=gen)
    hq = hashes[idx].cpu().numpy().view(np.uint64)
    m = gm.get_model(orc, oracle_lib, og, image.cpu().numpy(), es, None if segs is None else segs.cpu().numpy(),
                     (int(sg.nsegs), int(sg.seg_size), int(sg.seg_align_shift)), hq)
    np.testing.assert_array_equal(res[idx].cpu().numpy().view(np.uint32),
                                  fm.pack_res(m["status"], m["chains"], m["inc"]))
    np.testing.assert_array_equal(pos[idx].cpu().numpy().view(np.uint64), m["pos"])
    np.testing.assert_array_equal(vlen[idx].cpu().numpy().view(np.uint32), m["vlen"])
    np.testing.assert_array_equal(vloc[idx].cpu().numpy().view(np.uint64), m["vloc"])
    np.testing.assert_array_equal(rows[idx].cpu().numpy(), gm.rows_of(m["values"], stride))
    return int((m["status"] == 0).sum()), int((((m["vloc"] >> np.uint64(63)) == 1) & (m["status"] == 0)).sum())


def measure(name, g, sg, es, image, segs, hq, stride, a, gen):
    n = hq.shape[0]
    got = kvh.ht_get(image, g, segs, sg, hq, entry_size=es, stride=stride)
    pos, res, vlen, vloc, _ = got
    fpos, fres, _ = kvh.ht_find(image, g, hq, entry_size=es)
    assert torch.equal(pos, fpos) and torch.equal(res >> 8, fres >> 8)
    st = res & 0xFF
    assert torch.equal(st, fres & 0xFF), "an image written from the model's layout has no KEY_MUTATED / KEY_NO_VALUE"
    ok = st == kvh.KVH_KEY_OK
    found = int(ok.sum())
    in_seg = ok & (vloc < 0)  # bit 63
    n_seg = int(in_seg.sum())
    n_ok, n_ok_seg = spot_check(g, sg, es, image, segs, hq, got, stride, a.check, gen)
    chains = (res >> 16) & 0xFFFF
    probes = int((chains + (pos != -1).to(torch.int32)).sum())
    ln = vlen[in_seg].to(torch.int64)
    data_lines = (48 + ln + 63) // 64
    all_lines = (48 + ln + 16 + 63) // 64  # the message; its last line holds the trailer
    seg_lines = int((data_lines + (all_lines > data_lines).to(torch.int64)).sum())
    value_bytes = int(vlen[ok].to(torch.int64).sum())
    del got, pos, res, vlen, vloc, fpos, fres, st, ok, in_seg, chains, ln, data_lines, all_lines
    torch.cuda.empty_cache()
    t_get = timed(lambda: kvh.ht_get(image, g, segs, sg, hq, entry_size=es, stride=stride), a.warmup, a.iters)
    t_nocopy = timed(lambda: kvh.ht_get(image, g, segs, sg, hq, entry_size=es, copy=False), a.warmup, a.iters)
    t_floor = timed(lambda: kvh.ht_find(image, g, hq, entry_size=es, gather=True), a.warmup, a.iters)
    touched = 64 * (probes + (found - n_seg) + seg_lines)
    touched_floor = 64 * (probes + found)
    r = {"mix": name, "stride": stride, "n": n, "found": found, "in_segments": n_seg, "value_bytes": value_bytes,
         "nsegs": int(sg.nsegs), "segment_bytes": sg.nbytes, "spot_checked": a.check, "spot_ok": n_ok,
         "spot_ok_in_segments": n_ok_seg, "probes": probes, "touched_bytes": touched,
         "touched_bytes_floor": touched_floor, "calls": {}}
    for k, (med, lo, hi) in (("ht_get", t_get), ("ht_get_no_copy", t_nocopy), ("ht_find_gather", t_floor)):
        r["calls"][k] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                         "keys_per_s": round(n / med * 1e3)}
    r["get_over_find_gather"] = round(t_get[0] / t_floor[0], 2)
    r["touched_GBps_get"] = round(touched / t_get[0] / 1e6, 1)
    r["touched_GBps_find_gather"] = round(touched_floor / t_floor[0] / 1e6, 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-slots", type=int, default=24)
    ap.add_argument("--es", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=4)
    ap.add_argument("--arity", type=int, default=4)
    ap.add_argument("--loads", default="0.5,0.9")
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--check", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("get_time.py measures on the GPU: none visible")
    size, es, n = 1 << a.log2_slots, a.es, a.n
    g = kvh.HtGeom.from_map(HDR + es * size, es, 1.0, a.buckets, a.arity)
    assert int(g.ht_size) == size
    gen = torch.Generator(device=DEV)
    gen.manual_seed(20261019)
    results = []
    for load in (float(x) for x in a.loads.split(",")):
        image, keys, placed, slots = build_image(g, es, a.buckets, int(load * size), gen)
        pick = placed[torch.randint(0, placed.numel(), (n,), device=DEV, generator=gen)]
        qk = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=DEV, generator=gen)
        present = torch.rand((n,), device=DEV, generator=gen) < 0.5
        qk[present] = keys[pick[present]]
        del pick, present
        hq = kvh.meow128_fixed(qk.view(-1), 16, SEED, fixup=True)
        del qk
        for mix in ("imm8", "seg"):
            if mix == "imm8":
                segs, sg, stride = None, kvh.SegGeom(0, 0, SHIFT), 16
            else:
                segs, sg, _ = add_segment_values(image, es, slots, gen)
                stride = 256
            r = {"slots": size, "entry_size": es, "buckets": a.buckets, "arity": a.arity, "load": load,
                 "placed": int(placed.numel())}
            r.update(measure(mix, g, sg, es, image, segs, hq, stride, a, gen))
            print(json.dumps(r), flush=True)
            results.append(r)
        del image, keys, placed, slots, hq, segs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
