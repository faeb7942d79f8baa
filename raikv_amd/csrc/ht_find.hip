// ht_find.hip -- batched read-only find over a device-resident copy of a
// raikv hash table's ht[] (kvh_ht_find, kvh_meow128_fixed_find): what
// KeyCtx::find (include/raikv/ht_search.h:308-367) answers for one key, for n
// keys in one launch, on an image that cannot change.
//
//   k_find<A,W>          (h1,h2) pairs resident in HBM -> slot, status,
//                        optionally the matched entry
//   k_fixed_find<L,A,W>  fused: fixed-length keys -> Meow128 -> KeyFragment
//                        fixup -> the same walk (16/32-byte keys, the shapes
//                        k_fixed_pos fuses)
//
// The walk, per key (one lane each):
//   pos = ht_mod(h1); h = entry[pos].hash
//     h == h1: seal clear -> KEY_BUSY; hash2 == h2 -> KEY_OK, or KEY_NOT_FOUND
//              when FL_DROPPED; else go on      (KeyCtx::equals compares
//              hash2 only, key_ctx.h:245-246)
//     h == 0 -> KEY_NOT_FOUND at pos; h & ZOMBIE64 -> KEY_BUSY; else go on
//   go on: ++chains, ++pos (ring); a linear table (cuckoo_buckets <= 1,
//     key_ctx.cpp:209-215) ends KEY_HT_FULL at chains == ht_size
//     (ht_linear.cpp:33-41); a cuckoo table moves to CuckooAltHash::pos[++inc]
//     after cuckoo_buckets slots and ends KEY_NOT_FOUND when inc reaches the
//     arity (ht_cuckoo.h:135-141, ht_cuckoo.cpp:488-507).
// Where the reference spins (a locked slot, a broken seal) the snapshot cannot
// change, so the key is reported KEY_BUSY and the walk stays bounded:
// arity x buckets probes, or ht_size on a linear table.
//
// Memory shape.  A probe reads the 16-byte head (hash, hash2) of an entry,
// one global_load_dwordx4 at a random 64-byte-aligned (entry-aligned)
// address: latency bound, so the kernels keep many probes in flight.  The
// heads of a whole window (up to 8 slots, contiguous but for the ring wrap)
// are loaded before the first is compared, so a window costs one memory
// latency; a linear table is walked in groups of 4 slots.  flags and the
// seal word are read only on a hash match (once per found key).  The
// alternate positions (cuckoo_positions, ht_pos.hpp) are computed only by
// lanes whose home window failed, as the reference creates CuckooAltHash on
// demand.  No LDS (but the Meow tables of the fused kernel), small workgroups,
// one-shot grid: occupancy is what hides the latency.  The entry gather is a
// second phase of the same kernel: the wave's 64 results stay in registers and
// es/16 lanes cooperate on one row (its slot read from the owner lane by a
// wave shuffle), so every store instruction writes one contiguous run of
// 16-byte pieces; rows of keys that are not KEY_OK are zero-filled there too.
// The table is only read; results go out through plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "kvh_internal.hpp"
#include "ht_pos.hpp"
#include "ht_find_dev.hpp"
#include "../../include/kvh.h"

using namespace kvh;
using namespace kvh::rt;
using namespace kvh::htf;

namespace {

constexpr int kFindBlock = 256;        // no LDS: small groups, many waves per CU
constexpr int kFusedFindBlock = 1024;  // the Meow tables are filled once per workgroup

// The wave's keys b .. b + 63 (lane l owns key b + l: ok, at) -> rows of
// `rows`: the entry of a KEY_OK key, zeros otherwise.  Called by all 64 lanes.
template <typename W>
__device__ __forceinline__ void gather_rows(const Image& im, uint8_t* __restrict__ rows, const RowPlan rp, uint64_t b,
                                            uint64_t n, uint32_t lane, bool ok, W at) {
  const bool wide = rp.R > 64;
  const uint32_t kk = wide ? 0u : lane / rp.R;
  const uint32_t p0 = wide ? lane : lane - kk * rp.R;
  const uint32_t pstep = wide ? 64u : rp.R;
  const bool act = kk < rp.rpi;
  const uint32_t at_lo = (uint32_t)at, at_hi = sizeof(W) == 8 ? (uint32_t)((uint64_t)at >> 32) : 0u;
  constexpr int U = 4;  // rows steps whose loads are issued before their stores
  for (uint32_t k0 = 0; k0 < 64; k0 += U * rp.rpi) {
    uint32_t k[U];
    uint64_t slot[U];
    bool live[U], hit[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t row = k0 + u * rp.rpi + kk;
      k[u] = std::min<uint32_t>(row, 63u);
      const uint32_t lo = (uint32_t)__shfl((int)at_lo, (int)k[u], 64);
      const uint32_t hi = sizeof(W) == 8 ? (uint32_t)__shfl((int)at_hi, (int)k[u], 64) : 0u;
      hit[u] = __shfl((int)ok, (int)k[u], 64) != 0;
      slot[u] = (uint64_t)lo | ((uint64_t)hi << 32);
      live[u] = act && row < 64 && b + row < n;
    }
    for (uint32_t p = p0; p < rp.R; p += pstep) {
      v4u v[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        v[u] = v4u{0u, 0u, 0u, 0u};
        if (live[u] && hit[u]) v[u] = *(const v4u*)(entry_at(im, slot[u]) + (uint64_t)p * 16);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; u++)
        if (live[u]) __builtin_nontemporal_store(v[u], (v4u*)(rows + (b + k[u]) * (uint64_t)im.es + (uint64_t)p * 16));
    }
  }
}

template <int A, typename W>
__global__ void __launch_bounds__(kFindBlock)
k_find(Image im, HtGeom g, const uint64_t* __restrict__ hashes, uint64_t n, void* __restrict__ pos,
       uint32_t* __restrict__ res, uint8_t* __restrict__ rows, RowPlan rp, uint32_t p32) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t step = (((uint64_t)gridDim.x * blockDim.x) >> 6) * 64;
  const uint64_t last = n - 1;
  for (uint64_t b = wave * 64; b < n; b += step) {
    const uint64_t idx = b + lane;
    const v4u h = __builtin_nontemporal_load((const v4u*)(hashes + 2 * std::min<uint64_t>(idx, last)));
    W at;
    const uint32_t r = find_one<A, W>(im, g, (uint64_t)h.x | ((uint64_t)h.y << 32),
                                      (uint64_t)h.z | ((uint64_t)h.w << 32), at);
    if (idx <= last) store_result<W>(pos, res, idx, p32 != 0, r, at);
    if (rows) gather_rows<W>(im, rows, rp, b, n, lane, idx <= last && (r & 0xFFu) == kKeyOk, at);
  }
}

// k_fixed_pos's front end (ht_pos.hip: keys -> Meow128 -> KeyFragment fixup,
// the Meow T-tables in LDS) in front of the same walk.
template <int L, int A, typename W>
__global__ void __launch_bounds__(kFusedFindBlock)
k_fixed_find(const uint8_t* __restrict__ keys, uint64_t n, uint64_t s1, uint64_t s2, Image im, HtGeom g,
             uint64_t* __restrict__ out, void* __restrict__ pos, uint32_t* __restrict__ res,
             uint8_t* __restrict__ rows, RowPlan rp, uint32_t p32) {
  constexpr int NT = 2, NC = Plan<L>::NC;
  __shared__ uint32_t lds[LdsTab<NT>::kWords];
  fill_tables<NT>(lds);
  __syncthreads();
  const LdsTab<NT> T(lds);
  const MeowConst K = uniform(make_const(s1, s2, (uint64_t)L, T));
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t step = (((uint64_t)gridDim.x * blockDim.x) >> 6) * 64;
  const uint64_t last = n - 1;
  for (uint64_t b = wave * 64; b < n; b += step) {
    const uint64_t idx = b + lane, j = std::min<uint64_t>(idx, last);
    Blk D[NC];
    load_fixed<L, true, true>(keys + j * L, D);
    const Blk h = fixup(meow_ct<L>(D, K, T));
    if (out != nullptr && idx <= last) store_h<true>(out, j, h, false);
    W at;
    const uint32_t r = find_one<A, W>(im, g, (uint64_t)h.w[0] | ((uint64_t)h.w[1] << 32),
                                      (uint64_t)h.w[2] | ((uint64_t)h.w[3] << 32), at);
    if (idx <= last) store_result<W>(pos, res, idx, p32 != 0, r, at);
    if (rows) gather_rows<W>(im, rows, rp, b, n, lane, idx <= last && (r & 0xFFu) == kKeyOk, at);
  }
}

// ------------------------------------------------------------ host side
struct FindArgs {
  Image im;
  HtGeom g;
  uint64_t n;
  void* pos;
  uint32_t* res;
  uint8_t* rows;
  RowPlan rp;
  uint32_t p32;
  hipStream_t st;
};

template <int A>
void launch_find(const FindArgs& a, const uint64_t* h) {
  // one-shot grid (the dispatcher hands blocks out in order); the loop in the kernel covers n beyond it
  const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((a.n + kFindBlock - 1) / kFindBlock, 1u << 30));
  if (narrow(a.g))
    hipLaunchKernelGGL((k_find<A, uint32_t>), dim3((uint32_t)grid), dim3(kFindBlock), 0, a.st, a.im, a.g, h, a.n, a.pos,
                       a.res, a.rows, a.rp, a.p32);
  else
    hipLaunchKernelGGL((k_find<A, uint64_t>), dim3((uint32_t)grid), dim3(kFindBlock), 0, a.st, a.im, a.g, h, a.n, a.pos,
                       a.res, a.rows, a.rp, a.p32);
}

int find_a(uint32_t arity, const FindArgs& a, const uint64_t* h) {
  switch (arity) {
    case 1: launch_find<1>(a, h); break;
    case 2: launch_find<2>(a, h); break;
    case 3: launch_find<3>(a, h); break;
    case 4: launch_find<4>(a, h); break;
    case 5: launch_find<5>(a, h); break;
    case 6: launch_find<6>(a, h); break;
    case 7: launch_find<7>(a, h); break;
    case 8: launch_find<8>(a, h); break;
    default: return set_err(KVH_EINVAL);
  }
  return launch_done();
}

template <int L, int A>
void launch_fused(const FindArgs& a, const uint8_t* k, uint64_t s1, uint64_t s2, uint64_t* out, int cus) {
  const uint64_t need = (a.n + kFusedFindBlock - 1) / kFusedFindBlock;
  const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cus * 2));
  if (narrow(a.g))
    hipLaunchKernelGGL((k_fixed_find<L, A, uint32_t>), dim3((uint32_t)grid), dim3(kFusedFindBlock), 0, a.st, k, a.n, s1,
                       s2, a.im, a.g, out, a.pos, a.res, a.rows, a.rp, a.p32);
  else
    hipLaunchKernelGGL((k_fixed_find<L, A, uint64_t>), dim3((uint32_t)grid), dim3(kFusedFindBlock), 0, a.st, k, a.n, s1,
                       s2, a.im, a.g, out, a.pos, a.res, a.rows, a.rp, a.p32);
}

template <int L>
int fused_a(uint32_t arity, const FindArgs& a, const uint8_t* k, uint64_t s1, uint64_t s2, uint64_t* out, int cus) {
  switch (arity) {
    case 1: launch_fused<L, 1>(a, k, s1, s2, out, cus); break;
    case 2: launch_fused<L, 2>(a, k, s1, s2, out, cus); break;
    case 4: launch_fused<L, 4>(a, k, s1, s2, out, cus); break;
    case 8: launch_fused<L, 8>(a, k, s1, s2, out, cus); break;
    default: return set_err(KVH_EINVAL);
  }
  return launch_done();
}

// the shapes k_fixed_pos fuses (ht_pos.hip fused_ok)
bool fused_ok(uint32_t key_len, uint32_t a, const void* keys) {
  return (key_len == 16 || key_len == 32) && (a == 1 || a == 2 || a == 4 || a == 8) && ((uintptr_t)keys & 15) == 0;
}

// argument checks shared by both entries; 0, or 1 for "n == 0: nothing to do", or a negative error
int check_find(const void* entries, uint32_t es, const kvh_ht_geom_t* geom, size_t n, const void* pos,
               const uint32_t* res, const void* entries_out, bool p32) {
  if (es < 32 || (es & 31) != 0) return KVH_EINVAL;
  if (int rc = ht_check_geom(geom, p32)) return rc;
  if (n == 0) return 1;
  if (!entries || ((uintptr_t)entries & 15) || !pos || ((uintptr_t)pos & (p32 ? 3 : 7)) || !res ||
      ((uintptr_t)res & 3) || ((uintptr_t)entries_out & 15))
    return KVH_EINVAL;
  return 0;
}

FindArgs find_args(const void* entries, uint32_t es, const kvh_ht_geom_t* geom, size_t n, void* pos, uint32_t* res,
                   void* entries_out, bool p32, void* stream) {
  FindArgs a;
  a.im.ent = (const uint8_t*)entries;
  a.im.es = es;
  a.g = ht_dev_geom(geom);
  a.n = n;
  a.pos = pos;
  a.res = res;
  a.rows = (uint8_t*)entries_out;
  a.rp = row_plan(es);
  a.p32 = p32 ? 1u : 0u;
  a.st = (hipStream_t)stream;
  return a;
}

}  // namespace

extern "C" {

int kvh_ht_find(const void* entries, uint32_t hash_entry_size, const kvh_ht_geom_t* geom, const uint64_t* hashes,
                size_t n, void* pos, uint32_t* res, void* entries_out, uint32_t flags, void* stream) {
  const bool p32 = (flags & KVH_POS32) != 0;
  int rc = check_find(entries, hash_entry_size, geom, n, pos, res, entries_out, p32);
  if (rc) return set_err(rc < 0 ? rc : 0);
  if (!hashes || ((uintptr_t)hashes & 15)) return set_err(KVH_EINVAL);
  int cus = 0;
  rc = device_cus(&cus);  // the first call on a device initialises the runtime, as the neighbours do
  if (rc) return rc;
  return find_a(ht_per_key(geom), find_args(entries, hash_entry_size, geom, n, pos, res, entries_out, p32, stream),
                hashes);
}

int kvh_meow128_fixed_find(const void* keys, uint32_t key_len, size_t n, uint64_t seed1, uint64_t seed2,
                           const void* entries, uint32_t hash_entry_size, const kvh_ht_geom_t* geom, uint64_t* hashes,
                           void* pos, uint32_t* res, void* entries_out, uint32_t flags, void* stream) {
  const bool p32 = (flags & KVH_POS32) != 0;
  int rc = check_find(entries, hash_entry_size, geom, n, pos, res, entries_out, p32);
  if (rc) return set_err(rc < 0 ? rc : 0);
  if (!keys || (hashes && ((uintptr_t)hashes & 15))) return set_err(KVH_EINVAL);
  const uint32_t a = ht_per_key(geom);
  const bool fused = fused_ok(key_len, a, keys);
  // other shapes run the hash kernel, then the find kernel on its output: that output is the caller's
  // `hashes` (nothing is allocated in the call), so they need it
  if (!fused && !hashes) return set_err(KVH_EINVAL);
  int cus = 0;
  rc = device_cus(&cus);
  if (rc) return rc;
  const FindArgs fa = find_args(entries, hash_entry_size, geom, n, pos, res, entries_out, p32, stream);
  if (fused) {
    const uint8_t* k = (const uint8_t*)keys;
    return key_len == 16 ? fused_a<16>(a, fa, k, seed1, seed2, hashes, cus)
                         : fused_a<32>(a, fa, k, seed1, seed2, hashes, cus);
  }
  rc = kvh_meow128_fixed(keys, key_len, n, seed1, seed2, hashes, KVH_FIXUP, stream);
  if (rc) return rc;
  return find_a(a, fa, hashes);
}

}  // extern "C"
