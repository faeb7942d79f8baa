#!/usr/bin/env python3
"""Time the batched find (kvh_ht_find, with and without the entry gather, and
the fused kvh_meow128_fixed_find) on a table image at scale, beside the two
positions calls at the same n -- the floor: find does that work plus the
reads.  Needs an MI355X.

    python tools/find_time.py [--log2-slots 24] [--n 100000000] [--loads 0.5,0.9] [--out FILE]

The image is built on the device with the model's placement rule restated in
parallel rounds: every key proposes the next slot of its windows (ring order
inside a window, then the next alternate), the lowest key index wins a free
slot, the others move on -- so every slot a placed key passed over is
occupied, which is what find needs.  The inserted pairs are the fixed-up
Meow128 hashes of random 16-byte keys, so one data set serves the hash-pair
and the fused call.  Queries: half drawn from the placed keys, half fresh
keys, mixed.  20k results are spot-checked against tests/find_model.py.

Times are HIP events around the call on the current stream (median of
--iters after --warmup).  touched bytes = 64 B x (probes + gathered rows)
with probes = entry heads the walk compared; window bytes counts what the
kernel loads (whole windows of cuckoo_buckets heads).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raikv_amd as kvh  # noqa: E402

SEED = kvh.STATIC_SEED
DEV = "cuda"
HDR = 448 << 10  # KV_HT_HDR_SIZE + KV_HT_CTX_SIZE + KV_HT_STATS_SIZE


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return statistics.median(ms), min(ms), max(ms)


def build_image(g, es, buckets, m, gen):
    """-> (image uint8 [size, es], keys uint8 [m, 16] of the PLACED pairs, their slots)"""
    size = int(g.ht_size)
    keys = torch.randint(0, 256, (m, 16), dtype=torch.uint8, device=DEV, generator=gen)
    h = kvh.meow128_fixed(keys.view(-1), 16, SEED, fixup=True)
    P = kvh.ht_positions(h, g)
    A = P.shape[1]
    owner = torch.full((size,), -1, dtype=torch.int64, device=DEV)
    slot_of = torch.full((m,), -1, dtype=torch.int64, device=DEV)
    inc_of = torch.zeros((m,), dtype=torch.int64, device=DEV)
    active = torch.arange(m, device=DEV)
    probe = torch.zeros((m,), dtype=torch.int64, device=DEV)
    big = torch.iinfo(torch.int64).max
    for _ in range(A * buckets):
        if active.numel() == 0:
            break
        pr = probe[active]
        inc = pr // buckets
        slot = (P[active, inc] + pr % buckets) % size
        free = owner[slot] < 0
        ci, cs = active[free], slot[free]
        win = torch.full((size,), big, dtype=torch.int64, device=DEV)
        win.scatter_reduce_(0, cs, ci, "amin")
        won = win[cs] == ci
        owner[cs[won]] = ci[won]
        slot_of[ci[won]] = cs[won]
        inc_of[ci[won]] = inc[free][won]
        probe[active] += 1
        active = active[(slot_of[active] < 0) & (probe[active] < A * buckets)]
    placed = torch.nonzero(slot_of >= 0).view(-1)
    w = torch.zeros((size, es // 8), dtype=torch.int64, device=DEV)
    s = slot_of[placed]
    w[s, 0] = h[placed, 0]
    w[s, 1] = h[placed, 1]
    w[s, 2] = ((0x100 | inc_of[placed]) << 32) | (8 << 48)  # flags FL_IMMEDIATE_VALUE | inc, keylen 8
    w[s, 4] = placed                                          # the immediate value: the key's index in `keys`
    w[s, es // 8 - 1] = 8 | (1 << 15)                         # ValueCtr: size 8, seal
    return w.view(torch.uint8).view(size, es), keys, placed, s


def spot_check(g, es, image, hashes, pos, res, rows, count, gen):
    import oracle_lib
    import find_model as fm
    orc = oracle_lib.load_oracle()
    og = oracle_lib.OrcGeom()
    for k in ("ht_size", "ht_mod_mask", "ht_mod_fraction", "ht_mod_shift", "cuckoo_buckets", "cuckoo_arity"):
        setattr(og, k, getattr(g, k))
    idx = torch.randint(0, hashes.shape[0], (count,), device=DEV, generator=gen)
    img = image.cpu().numpy()
    hq = hashes[idx].cpu().numpy().view(np.uint64)
    st, p, ch, inc, _ = fm.find_model(orc, oracle_lib, og, img, es, hq)
    np.testing.assert_array_equal(res[idx].cpu().numpy().view(np.uint32), fm.pack_res(st, ch, inc))
    np.testing.assert_array_equal(pos[idx].cpu().numpy().view(np.uint64), p)
    want = np.zeros((count, es), np.uint8)
    ok = st == fm.KEY_OK
    want[ok] = img[p[ok].astype(np.int64)]
    np.testing.assert_array_equal(rows[idx].cpu().numpy(), want)
    return int(ok.sum())


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
        sys.exit("find_time.py measures on the GPU: none visible")
    size, es, n = 1 << a.log2_slots, a.es, a.n
    g = kvh.HtGeom.from_map(HDR + es * size, es, 1.0, a.buckets, a.arity)
    assert int(g.ht_size) == size
    gen = torch.Generator(device=DEV)
    gen.manual_seed(20261019)
    results = []
    for load in (float(x) for x in a.loads.split(",")):
        image, keys, placed, _ = build_image(g, es, a.buckets, int(load * size), gen)
        # queries: half present (drawn from the placed keys), half fresh keys, mixed
        pick = placed[torch.randint(0, placed.numel(), (n,), device=DEV, generator=gen)]
        qk = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=DEV, generator=gen)
        present = torch.rand((n,), device=DEV, generator=gen) < 0.5
        qk[present] = keys[pick[present]]
        del pick
        qk = qk.view(-1)
        hq = kvh.meow128_fixed(qk, 16, SEED, fixup=True)
        pos, res, rows = kvh.ht_find(image, g, hq, entry_size=es, gather=True)
        hh, pos2, res2, _ = kvh.meow128_fixed_find(qk, 16, SEED, image, g, entry_size=es)
        assert torch.equal(hh, hq) and torch.equal(pos, pos2) and torch.equal(res, res2)
        st = res & 0xFF
        found = int((st == kvh.KVH_KEY_OK).sum())
        assert found == int(present.sum()), (found, int(present.sum()))  # a fresh key colliding: 2^-64
        n_ok = spot_check(g, es, image, hq, pos, res, rows, a.check, gen)
        chains = (res >> 16) & 0xFFFF
        probes = int((chains + (pos != -1).to(torch.int32)).sum())
        windows = int((((res >> 8) & 0xFF) + 1).sum())
        del pos2, res2, hh, rows, st, chains
        t = {
            "ht_positions": timed(lambda: kvh.ht_positions(hq, g), a.warmup, a.iters),
            "meow128_fixed_positions": timed(lambda: kvh.meow128_fixed_positions(qk, 16, SEED, g), a.warmup, a.iters),
            "ht_find": timed(lambda: kvh.ht_find(image, g, hq, entry_size=es), a.warmup, a.iters),
            "ht_find_gather": timed(lambda: kvh.ht_find(image, g, hq, entry_size=es, gather=True), a.warmup, a.iters),
            "meow128_fixed_find": timed(lambda: kvh.meow128_fixed_find(qk, 16, SEED, image, g, entry_size=es),
                                        a.warmup, a.iters),
        }
        r = {"slots": size, "entry_size": es, "buckets": a.buckets, "arity": a.arity, "load": load,
             "placed": int(placed.numel()), "n": n, "found": found, "spot_checked": a.check, "spot_ok_rows": n_ok,
             "probes": probes, "touched_bytes": 64 * probes, "touched_bytes_gather": 64 * (probes + found),
             "window_bytes": windows * a.buckets * es if a.buckets > 1 else None, "calls": {}}
        for k, (med, lo, hi) in t.items():
            r["calls"][k] = {"ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                             "keys_per_s": round(n / med * 1e3)}
        r["find_over_positions"] = round(t["ht_find"][0] / t["ht_positions"][0], 2)
        r["fused_find_over_fused_positions"] = round(t["meow128_fixed_find"][0] / t["meow128_fixed_positions"][0], 2)
        r["touched_GBps_find"] = round(64 * probes / t["ht_find"][0] / 1e6, 1)
        r["touched_GBps_find_gather"] = round(64 * (probes + found) / t["ht_find_gather"][0] / 1e6, 1)
        print(json.dumps(r), flush=True)
        results.append(r)
        del image, keys, placed, qk, hq, pos, res
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
