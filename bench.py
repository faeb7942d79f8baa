#!/usr/bin/env python3
"""bench.py -- device-resident 128-bit Meow key-hash throughput on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c1|c2|c3|c4|c4g|c64|...]
                    [--dump-outputs DIR] [--full]

A plain run sets up the keys, settles and warms up, times the K steps, writes
the last step's outputs if --dump-outputs is given, and prints the JSON line
(value, ms_per_step, and the roofline figures the timed steps' own HIP events
give).  Everything that takes runs of its own -- the parity of the timed
output against the reference, the poisoned relaunch, the 1-GPU c4g scaling
anchor, the copy-peak probe, the PCIe-inclusive host pipeline and the CPU
baseline -- runs only with --full.

A "step" is one pass of the hot path (one kvh_meow128_* launch) over one
batch of synthetic keys already resident in HBM.  Default workload at every
N is BASELINE.json configs[1] (C1: 100M fixed 16-byte keys) per GPU: at N>1
each rank hashes its own 100M-key shard of an N x 100M batch ("scaling":
"weak"), so the driver's per-N values compare one workload.  Keys are
independent: there is no data-path collective; a CPU gloo group only carries
the barrier and the max-over-ranks time.  BASELINE configs[4] as stated (c4g:
ONE global batch of 1B 32-byte keys, rank r hashing index range
shard_range(1B, r, N), "scaling": "strong") runs with --config c4g and reads
against its 1-GPU anchor, which the default N=1 line carries under --full.

The JSON line carries
  roofline     : algorithmic bytes/launch / avg kernel time (HIP events on
                 the launch stream) against 8 TB/s HBM; `traffic` from the
                 committed rocprofv3 PMC summary for this workload, if any;
  cpu_baseline : (--full) the reference CPU path (oracle/_ref: the unmodified
                 src/key_hash.c kv_hash_meow128) on this box's host cores,
                 rank 0 at N=1 only, bounded sample; falls back to the
                 clean-room oracle port if the reference build is absent.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "128-bit key hashes/sec device-resident, 16–64B keys; GB/s vs HBM peak"
METRIC_F1 = "keys/sec -> hash + cuckoo table positions, device-resident (SURVEY.md §8 f1)"
METRIC_F4 = "CRC32C (kv_crc_c) keys/sec, device-resident (SURVEY.md §8 f4)"
METRIC_F3 = "tokens/sec: text -> tokenize -> NUL-terminated key hashes, device-resident (SURVEY.md §8 f3)"
METRIC_F2 = "keys/sec ordered by hash-table slot with adjacent duplicates marked, device-resident (SURVEY.md §8 f2)"
HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md chip table)
# LDS table-lookup ceiling: ds_read_b32 serves 32 lanes per LDS cycle per CU
# (MI355X_MICROARCH.md §LDS, 128 B/clk), 256 CUs, 2.4 GHz peak engine clock
LDS_PEAK_LOOKUPS = 32 * 256 * 2.4e9
# T-table lookups per unit of work (16 per AES round; folded rounds)
# (C3's unit is one hash: 7 rounds of 16 lookups per seed, four seeds per key)
LOOKUPS_PER_UNIT = {"c1": 5 * 16, "c4": 7 * 16, "c4g": 7 * 16, "c64": 13 * 16, "c3": 7 * 16, "f1": 5 * 16,
                    "f4": 16}
# the float4 copy rate MI355X_MICROARCH.md records for this part (the guide's
# achievable streaming figure, beside the box's own copy probe)
GUIDE_COPY_GBS = 6290.0

CONFIGS = {
    "c1": dict(workload="C1: 100M fixed 16-byte keys resident in HBM, one lane per key, bit-exact vs reference",
               n=100_000_000, key_len=16, arity=1, var=False),
    "c2": dict(workload="C2: 100M variable-length keys 8-256B (zipf theta .99 lengths), packed buffer + u64 offsets",
               n=100_000_000, key_len=0, arity=1, var=True),
    "c3": dict(workload="C3: cuckoo arity=4 multi-seed, 4 hashes per key over 50M 32B keys",
               n=50_000_000, key_len=32, arity=4, var=False),
    "c4": dict(workload="C4: 32-byte keys, 125M per GPU (1B over 8 GPUs), sharded by index range",
               n=125_000_000, key_len=32, arity=1, var=False),
    # BASELINE configs[4] as stated: one global 1B x 32 B batch, index-range shards (strong scaling)
    "c4g": dict(workload="C4: 1B 32-byte keys, one global batch sharded by index range across the GPUs "
                         "(per-GPU and aggregate hashes/s)",
                n=1_000_000_000, key_len=32, arity=1, var=False, global_batch=True),
    # the metric's top length: 100M x 64-byte keys (80 B/key: 64 in + 16 out)
    "c64": dict(workload="C64: 100M fixed 64-byte keys resident in HBM (the 64 B end of the metric's 16-64 B range)",
                n=100_000_000, key_len=64, arity=1, var=False),
    # SURVEY.md §8 f1 (next row): the consumer side of the hash
    "f1": dict(workload="F1: 100M fixed 16-byte keys -> Meow128 + fixup + cuckoo arity-4 table positions "
                        "(64 GiB map, 4 buckets), hashes and u64 positions stored; one fused kernel",
               n=100_000_000, key_len=16, arity=1, var=False, positions="fused"),
    "f1p": dict(workload="F1p: 100M resident fixed-up (h1,h2) -> cuckoo arity-4 table positions "
                         "(64 GiB map, 4 buckets), u64 positions",
                n=100_000_000, key_len=16, arity=1, var=False, positions="only"),
    # kv_ht_radix_sort + ctest's duplicate marking on a hashed batch
    "f2": dict(workload="F2: 100M resident fixed-up (h1,h2) pairs of 16-byte keys (1% duplicates) + u64 items -> "
                        "ordered by ht_mod(h1) (64 GiB map), adjacent duplicates marked (kvh_ht_sort, KVH_DEDUP)",
               n=100_000_000, key_len=16, arity=1, var=False, sort=True),
    # batched CRC32C (kv_crc_c) on the C1 / C2 key shapes
    "f4": dict(workload="F4: 100M fixed 16-byte keys -> kv_crc_c (CRC32C, seed 0), u32 out",
               n=100_000_000, key_len=16, arity=1, var=False, crc=True),
    "f4v": dict(workload="F4v: 100M zipf 8-256 B keys (C2 shape) -> kv_crc_c, u32 out",
                n=100_000_000, key_len=0, arity=1, var=True, crc=True),
    # ctest-style ingest of a text buffer
    "f3": dict(workload="F3: 1 GiB whitespace-separated text (≈25% separators) -> device tokenizer (ctest.c) -> "
                        "NUL-terminated key hashes with fixup (kv_hash_key_frag semantics)",
               n=1 << 30, key_len=0, arity=1, var=False, ingest=True),
}
F1_GEOM = dict(map_size=64 << 30, hash_entry_size=64, hash_value_ratio=1.0, cuckoo_buckets=4, cuckoo_arity=4)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def cpu_threads():
    """Host threads for the all-core CPU leg: the CPUs this process may run on
    (sched_getaffinity), capped by OMP_NUM_THREADS when the box sets it (the
    GPU box gives one GPU's job 16 CPUs and exports OMP_NUM_THREADS=16)."""
    try:
        aff = len(os.sched_getaffinity(0))
    except Exception:
        aff = os.cpu_count() or 1
    env = os.environ.get("OMP_NUM_THREADS", "")
    t = int(env) if env.isdigit() and int(env) > 0 else aff
    return max(1, min(t, aff)), aff


def host_model():
    try:
        return [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        return "unknown"


def c0_hash_test():
    """Config C0: the reference's own test/hash_test.cpp (compiled from its
    sources by oracle/Makefile into oracle/_ref/hash_test), `hash_test int
    meow 16`, one host thread; its 1,048,576-key line (10M timed calls, seeds
    (0,0), hash_test.cpp:730-760)."""
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "hash_test")
    if not os.path.exists(exe):
        return {"value": None, "error": "oracle/_ref/hash_test not built"}
    r = subprocess.run([exe, "int", "meow", "16"], capture_output=True, text=True, timeout=120)
    line = [l for l in r.stdout.splitlines() if l.startswith("1048576 keys")]
    if r.returncode != 0 or not line:
        return {"value": None, "error": f"rc={r.returncode}", "tail": r.stdout[-300:]}
    ns = float(line[-1].split("hash =")[1].split("ns")[0])
    return {"value": 1e9 / ns, "unit": "hash/s", "ns_per_hash": ns, "cores": 1, "kind": "reference",
            "line": line[-1].strip(), "cmd": "oracle/_ref/hash_test int meow 16 (1M IntContent keys, 10M calls)"}


def cpu_baseline(cfg, seed, seconds: float):
    """The reference CPU path (oracle/_ref/libkvref.so: the unmodified
    src/key_hash.c) on this box's host cores, on a bounded sample of the same
    workload shape: all available threads (value) and one thread; plus the C0
    hash_test line."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import load_ref, load_oracle  # test infrastructure: the checker only
    from raikv_amd.workload import C3_SEEDS, zipf_lengths, offsets_from_lengths
    import ctypes as C
    threads, aff = cpu_threads()
    rng = np.random.default_rng(42)
    arity = cfg["arity"]
    if cfg["var"]:
        n = 4_000_000
        offs = offsets_from_lengths(zipf_lengths(n, 8, 256, seed=42))
        keys = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
        shape = f"{n} zipf 8-256 B keys ({int(offs[-1]) / n:.1f} B mean) + u64 offsets"
        L = 0
    else:
        L = cfg["key_len"]
        n = 8_000_000 if arity == 1 else 2_000_000
        keys = rng.integers(0, 256, n * L, dtype=np.uint8)
        shape = f"{n} packed {L}-byte keys" + (f" x {arity} seeds" if arity > 1 else "")
    out = np.zeros(2 * n * arity, dtype=np.uint64)
    seeds4 = np.array(C3_SEEDS, dtype=np.uint64).reshape(-1)
    ref = load_ref()
    if ref is not None:
        kind = "reference"
        ref.ref_bench_var.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]
        ref.ref_bench_var.restype = C.c_double
        ref.ref_bench_4seed.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
        ref.ref_bench_4seed.restype = C.c_double
        what = ("kv_hash_meow128_4_same_length_4_seed (key in all 4 slots)" if arity == 4 else "kv_hash_meow128")

        def run(t):
            if cfg["var"]:
                return ref.ref_bench_var(keys.ctypes.data, offs.ctypes.data, n, C.c_uint64(seed[0]),
                                         C.c_uint64(seed[1]), out.ctypes.data, t)
            if arity == 4:
                return ref.ref_bench_4seed(keys.ctypes.data, L, n, seeds4.ctypes.data, out.ctypes.data, t)
            return ref.ref_bench_fixed(keys.ctypes.data, L, n, C.c_uint64(seed[0]), C.c_uint64(seed[1]),
                                       out.ctypes.data, t)
    else:  # clean-room port (single thread, scalar C)
        kind, threads, what = "port", 1, "oracle port of kv_hash_meow128"
        orc = load_oracle()

        def run(t):
            t0 = time.perf_counter()
            if cfg["var"]:
                orc.orc_batch_var(keys.ctypes.data, offs.ctypes.data, n, C.c_uint64(seed[0]), C.c_uint64(seed[1]),
                                  out.ctypes.data, 0)
            else:
                orc.orc_batch_fixed(keys.ctypes.data, L, n, C.c_uint64(seed[0]), C.c_uint64(seed[1]),
                                    out.ctypes.data, 0)
            return time.perf_counter() - t0

    def timed(t, budget):
        tt, nn = 0.0, 0
        while tt < budget:
            tt += float(run(t))
            nn += n
        return nn * arity / tt, nn, tt

    v, nn, tt = timed(threads, seconds * 0.6)
    res = {"value": v, "unit": "hash/s", "cores": threads, "kind": kind,
           "sample": f"{nn} keys ({shape}, {nn // n} passes) x {what} (src/key_hash.c), "
                     f"{threads} threads on {host_model()}, {tt:.1f} s",
           "cores_available": aff}
    if threads > 1:
        v1, nn1, tt1 = timed(1, seconds * 0.4)
        res["one_thread"] = {"value": v1, "unit": "hash/s", "cores": 1, "sample": f"{nn1} keys, {tt1:.1f} s"}
    if not cfg["var"] and arity == 1 and L == 16:
        res["c0_hash_test"] = c0_hash_test()
    return res


def cpu_baseline_positions(cfg, seed, seconds: float, geom):
    """Reference per-key path for the f1 configs: kv_hash_meow128 + fixup +
    KeyCtx::set_hash + CuckooAltHash::calc_hash (oracle/ref_cuckoo.cpp,
    compiled from the reference's ht_init/ht_cuckoo/key_ctx sources) on host
    threads; f1p times calc_hash alone on precomputed hashes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import load_ref_ht, load_oracle, orc_geom, orc_positions  # checker only
    import ctypes as C
    threads, _aff = cpu_threads()
    L, n = cfg["key_len"], 4_000_000
    rng = np.random.default_rng(42)
    keys = rng.integers(0, 256, n * L, dtype=np.uint8)
    hashes = np.zeros(2 * n, dtype=np.uint64)
    pos = np.zeros(n * geom.per_key, dtype=np.uint64)
    only = cfg["positions"] == "only"
    if only:
        hashes[:] = rng.integers(0, 2 ** 63, 2 * n, dtype=np.uint64)
    ref = load_ref_ht()
    if ref is not None:
        kind = "reference"
        run = lambda: ref.ref_cuckoo_bench(geom.ht_size, geom.ht_mod_mask, geom.ht_mod_fraction, geom.ht_mod_shift,
                                           geom.cuckoo_buckets, geom.cuckoo_arity,
                                           None if only else keys.ctypes.data, L, n, C.c_uint64(seed[0]),
                                           C.c_uint64(seed[1]), hashes.ctypes.data, pos.ctypes.data, threads)
    else:  # clean-room port, positions only, single thread
        kind, threads, only = "port", 1, True
        orc = load_oracle()
        og = orc_geom(orc, F1_GEOM["map_size"], 64, 1.0, F1_GEOM["cuckoo_buckets"], F1_GEOM["cuckoo_arity"])

        def run():
            t = time.perf_counter()
            orc_positions(orc, og, hashes.reshape(-1, 2))
            return time.perf_counter() - t
    total_t, total_n = 0.0, 0
    while total_t < seconds:
        total_t += float(run())
        total_n += n
    what = "calc_hash on resident hashes" if only else f"kv_hash_meow128({L} B) + fixup + set_hash + calc_hash"
    return {"value": total_n / total_t, "unit": "key/s", "cores": threads, "kind": kind,
            "sample": f"{total_n} keys ({n} distinct) x {what}, arity {geom.cuckoo_arity}, "
                      f"{threads} threads, {total_t:.1f} s"}


def cpu_baseline_sort(seconds: float, geom, hashes_np):
    """The reference's kv_ht_radix_sort + ctest.c:96-104's duplicate marking
    (oracle/ref_cuckoo.cpp ref_ht_sort_bench, compiled from radix_sort.cpp
    and the KV-core sources), one thread (the reference sort is serial), on
    4M-pair slices of the same hashes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import load_ref_ht  # checker only
    import ctypes as C
    ref = load_ref_ht()
    if ref is None:
        return {"value": None, "error": "oracle/_ref/libkvref_ht.so not built"}
    m = 4_000_000
    d = np.zeros(1, np.uint64)
    total_t, total_n, k = 0.0, 0, 0
    while total_t < seconds:
        sl = np.ascontiguousarray(hashes_np[(k * m) % (len(hashes_np) - m):][:m])
        t = ref.ref_ht_sort_bench(geom.ht_size, geom.ht_mod_mask, geom.ht_mod_fraction, geom.ht_mod_shift,
                                  sl.ctypes.data, m, d.ctypes.data)
        if t < 0:
            return {"value": None, "error": "ref_ht_sort_bench failed"}
        total_t += t
        total_n += m
        k += 1
    return {"value": total_n / total_t, "unit": "key/s", "cores": 1, "kind": "reference",
            "sample": f"{total_n} hash pairs in 4M-pair slices x kv_ht_radix_sort + adjacent-duplicate marking "
                      f"(64 GiB map geometry), 1 thread, {total_t:.1f} s"}


def cpu_baseline_crc(cfg, seconds: float):
    """Reference kv_crc_c_array (key_hash.c:122-142, SSE4.2 crc32, its own
    source compiled into oracle/_ref/libkvref.so) on host threads."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import load_ref  # checker only
    import ctypes as C
    import threading
    from raikv_amd.workload import zipf_lengths, offsets_from_lengths
    ref = load_ref()
    if ref is None:
        return {"value": None, "error": "oracle/_ref/libkvref.so not built"}
    ref.kv_crc_c_array.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    threads, _aff = cpu_threads()
    n = 2_000_000
    L = cfg["key_len"]
    lens = zipf_lengths(n, 8, 256, seed=3) if cfg["var"] else np.full(n, L, np.int64)
    offs = offsets_from_lengths(lens)
    keys = np.random.default_rng(1).integers(0, 256, int(offs[-1]), dtype=np.uint8)
    ptrs = (keys.ctypes.data + offs[:-1].astype(np.uint64)).astype(np.uint64)
    szs = np.asarray(lens, dtype=np.uint64)
    seeds = np.zeros(n, dtype=np.uint32)
    bounds = [n * t // threads for t in range(threads + 1)]

    def part(t):
        a, b = bounds[t], bounds[t + 1]
        ref.kv_crc_c_array(ptrs.ctypes.data + 8 * a, szs.ctypes.data + 8 * a, seeds.ctypes.data + 4 * a, b - a)

    total_t, total_n = 0.0, 0
    while total_t < seconds:
        ts = [threading.Thread(target=part, args=(t,)) for t in range(threads)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        total_t += time.perf_counter() - t0
        total_n += n
    return {"value": total_n / total_t, "unit": "key/s", "cores": threads, "kind": "reference",
            "sample": f"{total_n} keys ({n} distinct, {'zipf 8-256 B' if cfg['var'] else f'{L} B'}) x "
                      f"kv_crc_c_array, {threads} threads (ctypes releases the GIL), {total_t:.1f} s"}


def cpu_baseline_ingest(seconds: float, text):
    """ctest.c's per-token path through the reference's own functions
    (kv_make_key_frag + kv_set_key_frag_string + kv_hash_key_frag,
    oracle/ref_cuckoo.cpp ref_ctest_frags), one thread, on 4 MiB slices of
    the same text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import load_ref_ht  # checker only
    import ctypes as C
    ref = load_ref_ht()
    if ref is None:
        return {"value": None, "error": "oracle/_ref/libkvref_ht.so not built"}
    ref.ref_ctest_frags.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]
    ref.ref_ctest_frags.restype = C.c_long
    m = 4 << 20
    sl = np.ascontiguousarray(text[:m + 16].cpu().numpy())
    frag = np.zeros(2 * m + 64, np.uint8)
    ro = np.zeros(m // 2 + 1, np.uint64)
    hh = np.zeros(m + 2, np.uint64)
    sd = np.zeros(2, np.uint64)
    total_t, total_n = 0.0, 0
    while total_t < seconds:
        t0 = time.perf_counter()
        k = ref.ref_ctest_frags(sl.ctypes.data, m, 256, frag.ctypes.data, frag.size, ro.ctypes.data, hh.ctypes.data,
                                ro.size, sd.ctypes.data)
        total_t += time.perf_counter() - t0
        total_n += int(k)
    return {"value": total_n / total_t, "unit": "key/s", "cores": 1, "kind": "reference",
            "sample": f"{total_n} tokens from 4 MiB slices x ctest ingest (tokenize + kv_make_key_frag + "
                      f"kv_set_key_frag_string + kv_hash_key_frag), 1 thread, {total_t:.1f} s"}


def lds_line(config_name, units, kern_ms):
    """The Meow/CRC kernels are bound by LDS table lookups, not HBM
    (DESIGN.md §3.3): lookups per launch / kernel time vs the LDS ceiling."""
    lk = LOOKUPS_PER_UNIT.get(config_name)
    if lk is None:
        return None
    ach = units * lk / (kern_ms * 1e-3)
    return {"lookups_per_unit": lk, "achieved": ach, "peak": LDS_PEAK_LOOKUPS, "unit": "lookups/s",
            "frac": ach / LDS_PEAK_LOOKUPS,
            "note": "peak at the 2.4 GHz engine clock; under this load the chip holds 1.7-1.9 GHz"}


def load_traffic(config_name: str):
    """HBM bytes per launch from the committed rocprofv3 PMC summary, its
    source, and (gather kernels) the bracket [unique bytes, FETCH x2 + WRITE]
    the uncalibrated figure lies in."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(p):
        return None, None, None
    try:
        d = json.load(open(p))
        e = d.get(config_name)
        if e:
            return float(e["hbm_bytes_per_launch"]), e.get("source"), e.get("traffic_bounds")
    except Exception:
        pass
    return None, None, None


ANCHOR = "c4g"  # BASELINE configs[4] as stated: the workload of `--config c4g` at N > 1


def measure_anchor(kvh, seed, steps: int = 10, settle_ms: float = 300.0) -> dict:
    """The scaling anchor: the WHOLE c4g global batch
    (1B x 32-byte keys) hashed on this one GPU, timed like the main line
    (settle, then `steps` launches between synchronizes; HIP events on the
    launch stream for the kernel time).  At N = 1 it follows the C1 timed
    region, so the default line carries the 1-GPU point of the N > 1 curve;
    at N > 1 every rank measures it alone on its own GPU, one rank at a time."""
    import torch
    cfg = CONFIGS[ANCHOR]
    n, L = cfg["n"], cfg["key_len"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    keys = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda", generator=gen)
    out = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream()
    t_s = time.perf_counter()
    while (time.perf_counter() - t_s) * 1e3 < settle_ms:
        kvh.meow128_fixed(keys, L, seed, out=out)
        torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a, b in ev:
        a.record(st)
        kvh.meow128_fixed(keys, L, seed, out=out)
        b.record(st)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    km = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    del keys, out
    torch.cuda.empty_cache()
    return {"config": ANCHOR, "workload": cfg["workload"] + "; all of it on ONE GPU", "keys": n, "key_len": L,
            "steps": steps, "ms_per_step": wall / steps * 1e3, "kernel_ms": km,
            "hashes_per_s": n * steps / wall, "hashes_per_s_kernel": n / (km * 1e-3)}


def anchor_efficiency(world: int, value: float, per_gpu, anchors) -> dict:
    """Strong-scaling efficiency of an N-rank c4g line against the 1-GPU c4g
    anchor: aggregate / (N x anchor rate), the anchors being each rank's own
    GPU; per rank, its shard's kernel rate / its anchor's kernel rate."""
    ref = float(np.mean([a["hashes_per_s"] for a in anchors]))
    return {"efficiency_vs_anchor": value / (world * ref),
            "per_rank": [{"rank": p["rank"], "efficiency_vs_anchor": p["hashes_per_s"] / a["hashes_per_s_kernel"]}
                         for p, a in zip(per_gpu, anchors)],
            "anchor_hashes_per_s_mean": ref}


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_env(rank: int, world: int, port: int, base=None) -> dict:
    """The environment torch.distributed.run would give rank `rank` of a
    one-node job (one process per GPU; rendezvous on 127.0.0.1)."""
    env = dict(os.environ if base is None else base)
    env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
               GROUP_RANK="0", ROLE_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    return env


def launch_ranks(world: int, argv, exe=None, port=None, poll_s: float = 0.2) -> int:
    """`bench.py --gpus N` with no WORLD_SIZE: start N fresh rank processes
    of this script (the parent has imported neither torch nor HIP), print
    rank 0's JSON line, and return non-zero if any rank fails (the others are
    then terminated: exact PIDs this function started)."""
    import subprocess
    import threading
    port = port or free_port()
    cmd = [sys.executable, os.path.abspath(__file__)] if exe is None else list(exe)
    procs, lines = [], []
    for r in range(world):
        procs.append(subprocess.Popen(cmd + list(argv), env=rank_env(r, world, port),
                                      stdout=subprocess.PIPE if r == 0 else 2, text=True))
    reader = threading.Thread(target=lambda: lines.extend(procs[0].stdout), daemon=True)
    reader.start()
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
        failed = next((r for r, p in enumerate(procs) if p.poll() not in (None, 0)), None)
        time.sleep(poll_s)
    if failed is None:
        failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    if failed is not None:
        log(f"bench.py: rank {failed} exited with {procs[failed].returncode}; stopping the other ranks")
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    reader.join(timeout=30)
    js = [l for l in lines if l.lstrip().startswith("{")]
    if failed is None and js:
        print(js[-1].rstrip("\n"), flush=True)
        return 0
    for l in lines:
        log(l.rstrip("\n"))
    return 1


def resolve_config(name, rank: int, world: int, keys_override: int = 0):
    """The workload of this rank: c1 per GPU at every N (weak scaling: the
    driver's per-N values then compare one workload) unless named; a global
    batch (c4g, BASELINE configs[4] as stated) has rank r hash index range
    shard_range(n, r, N).  Returns (name, cfg with this rank's n, the global
    key count)."""
    if name is None:
        name = "c1"
    cfg = dict(CONFIGS[name])
    if keys_override:
        cfg["n"] = keys_override
    n_global = cfg["n"]
    if cfg.get("global_batch"):
        from raikv_amd.workload import shard_range
        lo, hi = shard_range(n_global, rank, world)
        cfg["n"] = hi - lo
        cfg["shard"] = [lo, hi]
    return name, cfg, n_global


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs = ranks; without WORLD_SIZE in the environment bench.py starts them itself")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="default: c1 per GPU at every N (weak scaling); c4g = BASELINE configs[4] as stated "
                         "(one global 1B x 32 B batch, strong scaling)")
    ap.add_argument("--keys", type=int, default=0, help="override keys per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg: parity of the timed output against the "
                         "reference and the poisoned relaunch, the 1-GPU c4g scaling anchor, the copy-peak probe, "
                         "the PCIe-inclusive host pipeline and the CPU baseline (each has its own --no-... switch); "
                         "without --full the run sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last step computed to DIR/<name>.npy (float64 words; "
                         "a fixed seeded sample of a large output, see dump_outputs)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--e2e", dest="e2e", action="store_true", default=None,
                    help="time the PCIe-inclusive host pipeline (default: on for c1/c2 at N=1)")
    ap.add_argument("--no-e2e", dest="e2e", action="store_false")
    ap.add_argument("--settle-ms", type=float, default=500.0,
                    help="untimed launches before the warmup, until the engine clock has left its post-idle "
                         "power transient (DESIGN.md §4.5); 0 disables")
    ap.add_argument("--no-copy-peak", action="store_true", help="skip the achievable-peak copy probe")
    ap.add_argument("--no-anchor", action="store_true",
                    help="skip the 1-GPU c4g scaling anchor (measured after c1 at N=1 and by every rank at N>1)")
    ap.add_argument("--parity-keys", type=int, default=20_000,
                    help="keys of the timed launch's output checked against the reference after the timed region")
    return ap.parse_args(argv)


def main():
    args = parse_args()

    # N ranks: under torch.distributed.run WORLD_SIZE is set and must agree
    # with --gpus; without it bench.py starts the N ranks itself (fresh child
    # processes, before anything here has touched torch or the GPU)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:
        if args.gpus is not None and int(env_world) != args.gpus:
            log(f"bench.py: WORLD_SIZE={env_world} but --gpus {args.gpus}: refusing to measure "
                f"{env_world} rank(s) as {args.gpus} GPU(s)")
            sys.exit(2)
    elif args.gpus is not None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    import torch

    from raikv_amd import dist as kdist
    rank, world, local = kdist.env_ranks()
    kdist.init(world)  # gloo control plane only: barrier + max time
    torch.cuda.set_device(local % max(1, torch.cuda.device_count()))  # one GPU per rank; ranks share a GPU only where fewer are visible
    import raikv_amd as kvh
    from raikv_amd.workload import STATIC_SEED, C3_SEEDS, zipf_lengths, offsets_from_lengths

    args.config, cfg, n_global = resolve_config(args.config, rank, world, args.keys)
    if args.e2e is None:
        args.e2e = args.config in ("c1", "c2")
    n, L, arity = cfg["n"], cfg["key_len"], cfg["arity"]
    seed = STATIC_SEED
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 + rank)

    # ---- synthetic keys resident in HBM (each rank its own shard)
    if cfg.get("ingest"):
        r = torch.randint(0, 8, (n,), dtype=torch.uint8, device="cuda", generator=gen)
        text = torch.where(r == 0, 32, torch.where(r == 1, 10, 97 + r)).to(torch.uint8)
        del r
        t_offs, t_lens = kvh.tokenize(text, 256)
        ntok = t_offs.numel()
        cap = ntok + 16
        t_offs = torch.empty((cap,), dtype=torch.int64, device="cuda")
        t_lens = torch.empty((cap,), dtype=torch.int32, device="cuda")
        t_cnt = torch.zeros((1,), dtype=torch.int64, device="cuda")
        t_scr = torch.empty((kvh.lib.kvh_tokenize_scratch_bytes(n) // 8 + 1,), dtype=torch.int64, device="cuda")
        t_out = torch.empty((cap, 2), dtype=torch.int64, device="cuda")
        import ctypes as _C

        def run(out):
            # one asynchronous call: tokenizer, then the span hash reading the
            # token count on the device (no host round trip in between)
            st = torch.cuda.current_stream().cuda_stream
            rc = kvh.lib.kvh_tokenize_hash(text.data_ptr(), n, 256, _C.c_uint64(seed[0]), _C.c_uint64(seed[1]),
                                           kvh.KVH_FIXUP | kvh.KVH_NULTERM, t_offs.data_ptr(), t_lens.data_ptr(),
                                           t_out.data_ptr(), cap, t_cnt.data_ptr(), t_scr.data_ptr(),
                                           t_scr.numel() * 8, st)
            assert rc == 0
        # text read twice (count + emit passes) + spans written/read + key bytes gathered + hashes
        alg_bytes = n + 12 * ntok + 16 * ntok
        cfg["tokens"] = ntok
    elif cfg.get("sort"):
        geom = kvh.HtGeom.from_map(**F1_GEOM)
        keys = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda", generator=gen)
        s_h = kvh.meow128_fixed(keys, L, seed, fixup=True)
        del keys
        nd = n // 100  # 1 % duplicates
        s_h[torch.randperm(n, device="cuda", generator=gen)[:nd]] = s_h[torch.randint(0, n, (nd,), device="cuda",
                                                                                      generator=gen)]
        s_items = torch.arange(n, dtype=torch.int64, device="cuda")
        sorter = kvh.HtSorter(geom, n)
        s_ho, s_io = torch.empty_like(s_h), torch.empty_like(s_items)
        # hashes + items in, hashes + items out
        alg_bytes = 2 * 24 * n
        run = lambda out: sorter.sort(s_h, s_items, dedup=True, out=s_ho, items_out=s_io)
    elif cfg.get("crc"):
        crc_out = torch.empty((n,), dtype=torch.int32, device="cuda")
        if cfg["var"]:
            lens = zipf_lengths(n, 8, 256, seed=3 + rank)
            offs_np = offsets_from_lengths(lens)
            keys = torch.randint(0, 256, (int(offs_np[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
            offs = torch.from_numpy(offs_np.view(np.int64)).cuda()
            alg_bytes = int(offs_np[-1]) + 8 * (n + 1) + 4 * n
            del lens
            run = lambda out: kvh.crc_c_var(keys, offs, 0, out=crc_out)
        else:
            keys = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda", generator=gen)
            alg_bytes = n * L + 4 * n
            run = lambda out: kvh.crc_c_fixed(keys, L, 0, out=crc_out)
    elif cfg["var"]:
        lens = zipf_lengths(n, 8, 256, seed=3 + rank)
        offs_np = offsets_from_lengths(lens)
        key_bytes = int(offs_np[-1])
        keys = torch.randint(0, 256, (key_bytes,), dtype=torch.uint8, device="cuda", generator=gen)
        offs = torch.from_numpy(offs_np.view(np.int64)).cuda()
        del lens
        alg_bytes = key_bytes + 8 * (n + 1) + 16 * n
        run = lambda out: kvh.meow128_var(keys, offs, seed, out=out)
    elif cfg.get("positions"):
        geom = kvh.HtGeom.from_map(**F1_GEOM)
        pk = geom.per_key
        keys = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device="cuda", generator=gen)
        hashes = torch.empty((n, 2), dtype=torch.int64, device="cuda")
        pos = torch.empty((n, pk), dtype=torch.int64, device="cuda")
        if cfg["positions"] == "fused":
            alg_bytes = n * L + 16 * n + 8 * pk * n
            run = lambda out: kvh.meow128_fixed_positions(keys, L, seed, geom, hashes=hashes, out=pos)
        else:
            kvh.meow128_fixed(keys, L, seed, out=hashes, fixup=True)
            alg_bytes = 16 * n + 8 * pk * n
            run = lambda out: kvh.ht_positions(hashes, geom, out=pos)
    else:
        key_bytes = n * L
        keys = torch.randint(0, 256, (key_bytes,), dtype=torch.uint8, device="cuda", generator=gen)
        alg_bytes = key_bytes + 16 * n * arity
        if arity == 1:
            run = lambda out: kvh.meow128_fixed(keys, L, seed, out=out)
        else:
            run = lambda out: kvh.meow128_multiseed(keys, L, list(C3_SEEDS[:arity]), out=out)
    keyed = cfg.get("positions") or cfg.get("crc") or cfg.get("ingest") or cfg.get("sort")
    out = None if keyed else \
        torch.empty((n, arity, 2) if arity > 1 else (n, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream()
    # settle: a GPU leaving idle boosts, then its power controller overshoots
    # (engine clock 2.1 -> 1.4 GHz by launch 6) and recovers over ~100 launches
    # (profiles/r02/driver_protocol/); steady-state throughput is the metric
    settle_n, t_s = 0, time.perf_counter()
    while (time.perf_counter() - t_s) * 1e3 < args.settle_ms:
        run(out)
        torch.cuda.synchronize()
        settle_n += 1
    for _ in range(args.warmup):
        run(out)
    torch.cuda.synchronize()
    kdist.barrier(world)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record(stream)
        run(out)
        b.record(stream)
    torch.cuda.synchronize()
    kdist.barrier(world)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    wall = kdist.reduce_max(wall, world)

    # parity of the bytes just timed (each rank its own shard), after the timed region
    T = {k: v for k, v in locals().items() if k in ("keys", "offs_np", "out", "hashes", "pos", "crc_out", "s_h", "s_ho",
                                                     "s_io", "sorter", "geom", "text", "t_offs", "t_lens", "t_out",
                                                     "t_cnt")}
    dumped = None
    if args.dump_outputs:  # before any later leg launches into these buffers again
        dumped = dump_outputs(args.dump_outputs, timed_outputs(cfg, T, out), f".rank{rank}" if world > 1 else "")
    try:
        par = (timed_parity(args.config, cfg, seed, T, args.parity_keys, rank)
               if args.full and args.parity_keys > 0 else None)
    except Exception as e:  # reported, never hidden: a failed check is not a pass
        par = {"checked": 0, "mismatches": None, "error": repr(e)[:300]}
    # every output word of the path, on the device: the timed output equals a
    # relaunch into poisoned buffers, in the default chunk order and in the
    # static one (a skipped chunk would keep the previous
    # launch's correct values and pass the sample above)
    if par is not None:
        try:
            par["full_compare"] = full_compare(kvh, cfg, T, run, out)
        except Exception as e:  # reported, never hidden
            par["full_compare"] = {"ok": False, "error": repr(e)[:300]}
    del T
    per_rank = kdist.gather({"rank": rank, "kernel_ms": kern_ms, "keys": n, "parity": par}, world)
    # the scaling anchor: the c4g workload on ONE GPU (N = 1: after the c1 line; N > 1: each rank in turn)
    anchors = None
    if args.full and not args.no_anchor and ((world == 1 and args.config == "c1") or
                                             (world > 1 and cfg.get("global_batch"))):
        a = None
        for r in range(world):
            kdist.barrier(world)
            if r == rank:
                try:
                    a = measure_anchor(kvh, seed)
                except Exception as e:  # reported, never hidden
                    a = {"error": repr(e)[:300]}
        kdist.barrier(world)
        anchors = kdist.gather(a, world)

    units = cfg["tokens"] if cfg.get("ingest") else n * arity
    # keys for the f1/f3/f4 configs; a global batch counts its keys once
    n_hash = (n_global * arity if cfg.get("global_batch") else units * world) * args.steps
    value = n_hash / wall
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    traffic, tsrc, tbounds = load_traffic(args.config)
    res = {
        "metric": METRIC_F1 if cfg.get("positions") else (METRIC_F4 if cfg.get("crc") else
                                                          (METRIC_F3 if cfg.get("ingest") else
                                                           (METRIC_F2 if cfg.get("sort") else METRIC))),
        "value": value,
        "unit": "key/s" if keyed else "hash/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": wall / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong" if cfg.get("global_batch") else "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (seeded uniform random key bytes generated on device; zipf lengths for C2)",
        "config": {"workload": cfg["workload"], "config": args.config,
                   "keys_per_gpu": cfg.get("tokens", n), **({"text_bytes": n} if cfg.get("ingest") else {}),
                   **({"global_keys": n_global, "shard_rank0": cfg["shard"]} if cfg.get("global_batch") else {}),
                   "key_len": L if L else "zipf 8-256", "hashes_per_key": arity,
                   "seed": ["0x%016x" % seed[0], "0x%016x" % seed[1]],
                   "parallelism": f"shard x{world} (index ranges, no collective)"},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "traffic": traffic,
                     "kernel_ms": kern_ms, "alg_bytes_per_launch": alg_bytes,
                     "traffic_source": tsrc,
                     **({"traffic_bounds": tbounds} if tbounds else {})},
        "settle": {"ms": args.settle_ms, "launches": settle_n},
        "hashes_per_s_per_gpu": n * arity / (kern_ms * 1e-3),
        "hashes_per_s_aggregate": n_hash / wall,
        "lds_roofline": lds_line(args.config, units, kern_ms),
        "full": args.full,
    }
    if dumped is not None:
        res["outputs_dumped"] = {"dir": args.dump_outputs, "format": "float64, one 32-bit word per element",
                                 "arrays": dumped}
    if par is not None:
        pr = [p["parity"] for p in per_rank]
        res["parity"] = {"checked": sum(p.get("checked") or 0 for p in pr),
                         "mismatches": (None if any(p.get("mismatches") is None for p in pr)
                                        else sum(p["mismatches"] for p in pr)),
                         "against": pr[0].get("against", pr[0].get("error")),
                         "sample": f"{args.parity_keys} random keys + first + last of each rank's timed output",
                         "full_compare": all((p.get("full_compare") or {}).get("ok") is True for p in pr),
                         "full_compare_detail": pr[0].get("full_compare"),
                         **({"errors": [p["error"] for p in pr if "error" in p]} if any("error" in p for p in pr)
                            else {})}
    if world > 1:
        res["per_gpu"] = [{"rank": p["rank"], "keys": p["keys"], "kernel_ms": p["kernel_ms"],
                           "hashes_per_s": p["keys"] * arity / (p["kernel_ms"] * 1e-3)} for p in per_rank]
    if anchors is not None:
        res["scaling_anchor"] = anchors[0] if world == 1 else {"per_rank": anchors}
        if world > 1 and all("hashes_per_s" in a for a in anchors):
            res.update(anchor_efficiency(world, value, res["per_gpu"], anchors))
    res["roofline"]["guide_copy_peak"] = GUIDE_COPY_GBS
    res["roofline"]["frac_vs_guide_copy"] = achieved / GUIDE_COPY_GBS
    if args.full and rank == 0 and world == 1 and not args.no_copy_peak:
        cp = copy_peak(alg_bytes)
        if cp.get("copy_GBps"):
            res["roofline"]["achievable_peak"] = cp["copy_GBps"]
            res["roofline"]["frac_vs_achievable"] = achieved / cp["copy_GBps"]
        res["roofline"]["achievable_source"] = cp
    if args.full and args.e2e and rank == 0 and world == 1:
        res["e2e_pcie"] = e2e(kvh, cfg, seed)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            if cfg.get("positions"):
                res["cpu_baseline"] = cpu_baseline_positions(cfg, seed, args.cpu_seconds, geom)
            elif cfg.get("crc"):
                res["cpu_baseline"] = cpu_baseline_crc(cfg, args.cpu_seconds)
            elif cfg.get("ingest"):
                res["cpu_baseline"] = cpu_baseline_ingest(args.cpu_seconds, text)
            elif cfg.get("sort"):
                res["cpu_baseline"] = cpu_baseline_sort(args.cpu_seconds, geom,
                                                        s_h[:16_000_000].cpu().numpy().view(np.uint64))
            else:
                res["cpu_baseline"] = cpu_baseline(cfg, seed, args.cpu_seconds)
        except Exception as e:  # report, never hide
            res["cpu_baseline"] = {"value": None, "error": repr(e)}
    kdist.finalize(world)
    if rank == 0:
        print(json.dumps(res), flush=True)


def timed_parity(name, cfg, seed, T, k: int, rank: int) -> dict:
    """Check this rank's output of the LAST timed launch (still in HBM) on a
    sample of k keys plus the first and the last, against the compiled
    reference (tests/bench_parity.py; the checker, called after the timed
    region).  T holds the run's device tensors by name."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench_parity as bp  # checker only
    from raikv_amd.workload import C3_SEEDS
    n, L, arity = cfg["n"], cfg["key_len"], cfg["arity"]
    t0 = time.perf_counter()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)

    def gather_bytes(buf, starts, lens):
        """the bytes of spans (starts, lens) of a device buffer, packed, + local offsets"""
        lo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if lo[-1] == 0:
            return np.zeros(0, np.uint8), lo.astype(np.uint64)
        pos = np.repeat(np.asarray(starts, np.int64) - lo[:-1], lens) + np.arange(lo[-1], dtype=np.int64)
        return buf[torch.from_numpy(pos).to(buf.device)].cpu().numpy(), lo.astype(np.uint64)

    if cfg.get("sort"):
        s_h, s_ho, s_io, geom = T["s_h"], T["s_ho"], T["s_io"], T["geom"]
        # a marked duplicate's h1 is 0 (ctest.c:96-104): its slot is compared through its item's input pair
        in_slots = ((s_h[s_io, 0] & int(geom.ht_mod_mask)) * int(geom.ht_mod_fraction)) >> int(geom.ht_mod_shift)
        descents = int((in_slots[1:] < in_slots[:-1]).sum())
        perm_ok = bool(torch.equal(torch.sort(s_io).values, torch.arange(n, device=s_io.device)))
        zeroed = int((s_ho[:, 0] == 0).sum())
        idx = torch.from_numpy(bp.sample_indices(n, k, seed=rank)).to(s_ho.device)
        items = s_io[idx]
        r = bp.ht_order(descents, perm_ok, u64(s_h[items]), u64(s_ho[idx]), int(T["sorter"].dups.item()), zeroed,
                        (geom.ht_mod_mask, geom.ht_mod_fraction, geom.ht_mod_shift), u64(in_slots[idx]))
    elif cfg.get("ingest"):
        cnt = int(T["t_cnt"].item())
        idx = bp.sample_indices(cnt, k, seed=rank)
        ti = torch.from_numpy(idx).to(T["t_offs"].device)
        o, ln = T["t_offs"][ti].cpu().numpy(), T["t_lens"][ti].cpu().numpy().astype(np.int64)
        text = T["text"]
        kb, lo = gather_bytes(text, o, ln)
        toks = [kb[lo[j]:lo[j + 1]] for j in range(len(idx))]
        tb = text.numel()
        nb = torch.from_numpy(np.stack([o - 1, o + ln]).clip(0, tb - 1)).to(text.device)
        nbv = text[nb].cpu().numpy().astype(np.int64)
        before = np.where(o > 0, nbv[0], -1)
        after = np.where(o + ln < tb, nbv[1], -1)
        r = bp.spans(toks, before, after, u64(T["t_out"][ti]), seed)
    elif cfg.get("crc"):
        idx = bp.sample_indices(n, k, seed=rank)
        ti = torch.from_numpy(idx).cuda()
        if cfg["var"]:
            offs_np = T["offs_np"]
            kb, lo = gather_bytes(T["keys"], offs_np[idx], (offs_np[idx + 1] - offs_np[idx]).astype(np.int64))
        else:
            kb = T["keys"].view(n, L)[ti].cpu().numpy().reshape(-1)
            lo = np.arange(len(idx) + 1, dtype=np.uint64) * np.uint64(L)
        r = bp.crc_var(kb, lo, T["crc_out"][ti].cpu().numpy().view(np.uint32), 0)
    elif cfg.get("positions"):
        idx = bp.sample_indices(n, k, seed=rank)
        ti = torch.from_numpy(idx).cuda()
        g = F1_GEOM
        r = bp.positions(u64(T["hashes"][ti]), u64(T["pos"][ti]),
                         (g["map_size"], g["hash_entry_size"], g["hash_value_ratio"], g["cuckoo_buckets"],
                          g["cuckoo_arity"]))
        if cfg["positions"] == "fused":
            rh = bp.meow_fixed(T["keys"].view(n, L)[ti].cpu().numpy(), L, u64(T["hashes"][ti]), [seed], fixup=True)
            r["mismatches"] += rh["mismatches"]
            r["against"] = f"hashes: {rh['against']}; positions: {r['against']}"
    elif cfg["var"]:
        idx = bp.sample_indices(n, k, seed=rank)
        offs_np = T["offs_np"]
        kb, lo = gather_bytes(T["keys"], offs_np[idx], (offs_np[idx + 1] - offs_np[idx]).astype(np.int64))
        r = bp.meow_var(kb, lo, u64(T["out"][torch.from_numpy(idx).cuda()]), seed)
    else:
        idx = bp.sample_indices(n, k, seed=rank)
        ti = torch.from_numpy(idx).cuda()
        seeds = [seed] if arity == 1 else list(C3_SEEDS[:arity])
        r = bp.meow_fixed(T["keys"].view(n, L)[ti].cpu().numpy(), L, u64(T["out"][ti]), seeds)
    r["seconds"] = round(time.perf_counter() - t0, 2)
    return r


def timed_outputs(cfg, T, out) -> dict:
    """The device tensors a caller of the timed path receives, by name (the
    ingest outputs cut to the token count the device wrote)."""
    if cfg.get("ingest"):
        k = int(T["t_cnt"].item())
        return {"token_offsets": T["t_offs"][:k], "token_lengths": T["t_lens"][:k], "hashes": T["t_out"][:k]}
    if cfg.get("sort"):
        return {"sorted_hashes": T["s_ho"], "sorted_items": T["s_io"]}
    if cfg.get("crc"):
        return {"crc": T["crc_out"]}
    if cfg.get("positions"):
        return {"positions": T["pos"], **({"hashes": T["hashes"]} if cfg["positions"] == "fused" else {})}
    return {"hashes": out}


DUMP_BYTES = 60_000_000  # all files of one --dump-outputs together (the limit is 64 MB)


def dump_outputs(dirname, outs: dict, suffix: str = "") -> dict:
    """--dump-outputs: what the last timed step left in each output, written
    as DIR/<name>.npy.  The outputs are integer words (u64 hashes, positions
    and items, u32 CRCs), so each row is stored as its little-endian 32-bit
    words in float64, which holds them exactly.  An output too large for its
    share of DUMP_BYTES is sampled at fixed seeded rows plus the first and
    the last (DIR/<name>_rows.npy holds the row numbers), and
    DIR/<name>_fold.npy carries the wrapping 64-bit sum of every (signed)
    32-bit word column of the WHOLE output, in 16-bit pieces, so two builds
    can be compared over all of it."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    written = {}
    for name, t in outs.items():
        rows = t.shape[0]
        wpr = t.element_size() * int(np.prod(t.shape[1:], dtype=np.int64)) // 4  # 32-bit words per row
        w = t.contiguous().view(torch.int32).reshape(rows, wpr)
        cap = DUMP_BYTES // len(outs) // (8 * (wpr + 1))
        if rows > cap:
            idx = np.unique(np.concatenate([[0, rows - 1],
                                            np.random.default_rng(20240531).integers(0, rows, cap - 2)]))
            sample = w[torch.from_numpy(idx).to(w.device)]
        else:
            idx, sample = np.arange(rows, dtype=np.int64), w
        fold = torch.sum(w, 0, dtype=torch.int64).cpu().numpy().view(np.uint64)
        pieces = np.stack([(fold >> np.uint64(s)) & np.uint64(0xffff) for s in (0, 16, 32, 48)], axis=1)
        np.save(os.path.join(dirname, f"{name}{suffix}.npy"), sample.cpu().numpy().view(np.uint32).astype(np.float64))
        np.save(os.path.join(dirname, f"{name}_rows{suffix}.npy"), idx.astype(np.float64))
        np.save(os.path.join(dirname, f"{name}_fold{suffix}.npy"), pieces.astype(np.float64))
        written[name] = {"rows": int(rows), "rows_written": int(len(idx)), "words32_per_row": int(w.shape[1])}
    return written


POISON = 0xA5


def full_compare(kvh, cfg, T, run, out) -> dict:
    """After the timed region: clone the output of the last timed launch,
    fill every output buffer with 0xA5 bytes, launch once more (default chunk
    order), compare the WHOLE output on the device with the clone and count
    words still holding the sentinel; then the same under the static chunk
    order (knob 24 = 1).  Every key's output must be rewritten, identically,
    by both orders (src/key_hash.c:1413-1429: every key has a hash)."""
    import torch
    outs = list(timed_outputs(cfg, T, out).values())
    timed = [t.clone() for t in outs]
    word = int.from_bytes(bytes([POISON]) * 8, "little", signed=True)
    res = {"words": int(sum(t.numel() for t in outs)), "against": "the timed output, whole, on the device"}
    for name, order in (("default_order", None), ("static_order", 1)):
        prev = kvh.lib.kvh_set_tuning(24, order) if order is not None else None
        try:
            for t in outs:
                t.view(torch.uint8).fill_(POISON)
            run(out)
            torch.cuda.synchronize()
        finally:
            if prev is not None:
                kvh.lib.kvh_set_tuning(24, prev)
        same = all(torch.equal(a, b) for a, b in zip(outs, timed))
        left = sum(int((t.view(torch.int64) == word).sum()) for t in outs
                   if t.dtype == torch.int64 and t.is_contiguous())
        res[name] = {"equal": bool(same), "sentinel_words": left}
    for t, c in zip(outs, timed):  # leave the timed output in place
        t.copy_(c)
    res["ok"] = all(res[k]["equal"] and res[k]["sentinel_words"] == 0 for k in ("default_order", "static_order"))
    return res


def copy_peak(alg_bytes):
    """The box's achievable streaming rate for this traffic (tools/copy_peak:
    16 B read + 16 B written per item, k_fixed's wave-chunked non-temporal
    access pattern, same byte count, after the same settle), run as a child
    process after the timed region."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "copy_peak")
    if not os.path.exists(exe):
        return {"error": "tools/copy_peak not built"}
    try:
        r = subprocess.run([exe, str(max(1, int(alg_bytes) // 32)), "500", "50"], capture_output=True, text=True,
                           timeout=120)
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as ex:  # reported, never hidden
        return {"error": repr(ex)[:200]}


def e2e(kvh, cfg, seed):
    """PCIe-inclusive host pipeline: pinned host keys (+ offsets) -> H2D ->
    kernel -> D2H -> pinned host hashes (kvh_meow128_fixed_host for c1,
    kvh_meow128_var_host for c2).  Measured from a C++ host on the system HIP
    runtime (tests/cpp/e2e_host, how raikv's C/C++ calls the C-ABI; the
    number DESIGN.md §4.4 quotes), in this Python process (torch's bundled
    HIP runtime), and, when this process sees more than one GPU, through
    kvh_meow128_*_host_multi over 2/4/8 of them (one host thread each)."""
    import subprocess
    import torch
    var = cfg["var"]
    L = 0 if var else (cfg["key_len"] or 16)
    n = 50_000_000
    res = {"keys": n, "key_len": "zipf 8-256" if var else L}
    exe = os.path.join(ROOT, "tests", "cpp", "e2e_host")

    def cpp(devs=None):
        try:
            cmd = [exe, str(n), str(L), "5"] + ([",".join(map(str, devs))] if devs else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            return json.loads(r.stdout.strip().splitlines()[-1])
        except Exception as ex:  # the figure is reported, not required
            return {"error": repr(ex)[:200]}
    res["cpp_host"] = cpp()
    ndev = torch.cuda.device_count()
    if ndev > 1:
        res["cpp_host_multi"] = {str(k): cpp(list(range(k))) for k in (2, 4, 8) if k <= ndev}
    rng = np.random.default_rng(7)
    if var:
        from raikv_amd.workload import zipf_lengths, offsets_from_lengths
        offs = offsets_from_lengths(zipf_lengths(n, 8, 256, seed=7))
        hf = kvh.host_empty(offs.shape, np.uint64)
        hf[:] = offs
        hk = kvh.host_empty((int(offs[-1]),), np.uint8)
        hk[:] = rng.integers(0, 256, hk.size, dtype=np.uint8)
        ho = kvh.host_empty((n, 2), np.uint64)
        call = lambda: kvh.meow128_var_host(hk, hf, seed, out=ho)
        ref = kvh.meow128_var(torch.from_numpy(hk).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(), seed)
        moved = hk.size + 8 * (n + 1) + 16 * n
    else:
        hk = kvh.host_empty((n * L,), np.uint8)
        hk[:] = rng.integers(0, 256, n * L, dtype=np.uint8)
        ho = kvh.host_empty((n, 2), np.uint64)
        call = lambda: kvh.meow128_fixed_host(hk, L, seed, out=ho)
        ref = kvh.meow128_fixed(torch.from_numpy(hk).cuda(), L, seed)
        moved = n * (L + 16)
    call()
    assert np.array_equal(ho, ref.cpu().numpy().view(np.uint64)), "host pipeline differs from the device kernel"
    del ref
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    dt = float(np.median(ts))
    res["python_torch_runtime"] = {"hash_per_s": n / dt, "GB_per_s_h2d_plus_d2h": moved / dt / 1e9}
    res["note"] = ("pinned host buffers (kvh_host_alloc), 16 MiB chunks, H2D / kernel / D2H on three streams; "
                   "median of 5 calls; outputs checked against the device kernel")
    return res


if __name__ == "__main__":
    main()
