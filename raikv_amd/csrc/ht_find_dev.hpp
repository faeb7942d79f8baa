// ht_find_dev.hpp -- the device side of the batched find walk, shared by the
// find kernels (ht_find.hip) and the get kernel (ht_get.hip): one key's
// KeyCtx::find (include/raikv/ht_search.h:308-367) over a table image that
// cannot change.  The walk and its memory shape are described at the top of
// ht_find.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "kvh_internal.hpp"
#include "ht_pos.hpp"

namespace kvh {
namespace htf {

constexpr uint32_t kKeyOk = 0, kKeyNotFound = 2, kKeyBusy = 3, kKeyHtFull = 5;  // KeyStatus, key_ctx.h
constexpr uint32_t kFlDropped = 0x800;                                          // hash_entry.h:127
constexpr uint32_t kSealBit = 0x8000;  // ValueCtr::seal: bit 15 of the u32 at es - 8 (hash_entry.h:175-180)

struct Image {
  const uint8_t* ent;  // ht[0]
  uint32_t es;         // hash_entry_size
};

__device__ __forceinline__ const uint8_t* entry_at(const Image& im, uint64_t slot) {
  return im.ent + slot * (uint64_t)im.es;
}

// `cnt` (<= G) slots from s on, in ring order: all heads loaded, then compared
// in the walk's order.  True when the walk ended (st, at set); else chains and
// s moved on by cnt.
template <int G, typename W>
__device__ __forceinline__ bool probe_group(const Image& im, W size, W& s, uint32_t cnt, uint64_t h1, uint64_t h2,
                                            uint32_t& st, W& at, uint64_t& chains) {
  W sl[G];
  v4u hd[G];
  W t = s;
#pragma unroll
  for (int k = 0; k < G; k++) {
    sl[k] = t;
    t = (W)(t + 1) == size ? (W)0 : (W)(t + 1);
  }
#pragma unroll
  for (int k = 0; k < G; k++)
    if ((uint32_t)k < cnt) hd[k] = *(const v4u*)entry_at(im, sl[k]);
  __builtin_amdgcn_sched_barrier(0);  // every head of the group in flight before the first compare
#pragma unroll
  for (int k = 0; k < G; k++) {
    if ((uint32_t)k < cnt) {
      const uint64_t h = (uint64_t)hd[k].x | ((uint64_t)hd[k].y << 32);
      if (h == h1) {
        const uint8_t* e = entry_at(im, sl[k]);
        const uint32_t ctr = *(const uint32_t*)(e + im.es - 8);
        const uint32_t fl = *(const uint32_t*)(e + 20);  // flags u16 at +20 (low half)
        if (!(ctr & kSealBit)) { st = kKeyBusy; at = (W)~(W)0; return true; }
        if (((uint64_t)hd[k].z | ((uint64_t)hd[k].w << 32)) == h2) {
          st = (fl & kFlDropped) ? kKeyNotFound : kKeyOk;
          at = sl[k];
          return true;
        }
      } else if (h == 0) {
        st = kKeyNotFound; at = sl[k]; return true;
      } else if (h >> 63) {
        st = kKeyBusy; at = (W)~(W)0; return true;
      }
      ++chains;
      s = (W)(sl[k] + 1) == size ? (W)0 : (W)(sl[k] + 1);
    }
  }
  return false;
}

// one cuckoo window: `buckets` slots from s, in groups of 8
template <typename W>
__device__ __forceinline__ bool probe_window(const Image& im, W size, W s, uint32_t buckets, uint64_t h1, uint64_t h2,
                                             uint32_t& st, W& at, uint64_t& chains) {
  for (uint32_t off = 0; off < buckets; off += 8)
    if (probe_group<8, W>(im, size, s, std::min<uint32_t>(8u, buckets - off), h1, h2, st, at, chains)) return true;
  return false;
}

// -> res = status | inc << 8 | min(chains, 0xFFFF) << 16; at = the slot, or ~0
template <int A, typename W>
__device__ __forceinline__ uint32_t find_one(const Image& im, const HtGeom& g, uint64_t h1, uint64_t h2, W& at) {
  const W size = (W)g.size;
  uint32_t st = kKeyNotFound, inc = 0;
  uint64_t chains = 0;
  at = (W)~(W)0;
  W s = Slot<W>::mod(g, h1);
  if (g.buckets <= 1) {  // linear probe: ht_size slots, then full
    bool done = false;
    for (uint64_t left = g.size; left != 0 && !done;) {
      const uint32_t cnt = (uint32_t)std::min<uint64_t>(4, left);
      done = probe_group<4, W>(im, size, s, cnt, h1, h2, st, at, chains);
      left -= cnt;
    }
    if (!done) { st = kKeyHtFull; at = (W)~(W)0; }
  } else {
    bool done = probe_window<W>(im, size, s, g.buckets, h1, h2, st, at, chains);
    if constexpr (A > 1) {
      if (!done) {  // only now: the alternates (CuckooAltHash is created on demand)
        W q[A];
        cuckoo_positions<A, W>(g, h1, h2, q);
#pragma unroll
        for (int i = 1; i < A; i++) {
          if (!done) {
            if (q[i] >= size) {  // the ~0 of an unplaceable alternate (no accepted geometry has one)
              done = true;
            } else {
              inc = (uint32_t)i;
              done = probe_window<W>(im, size, q[i], g.buckets, h1, h2, st, at, chains);
            }
          }
        }
      }
    }
    if (!done) { st = kKeyNotFound; at = (W)~(W)0; }
  }
  return st | (inc << 8) | ((uint32_t)std::min<uint64_t>(chains, 0xFFFFu) << 16);
}

template <typename W>
__device__ __forceinline__ void store_result(void* __restrict__ pos, uint32_t* __restrict__ res, uint64_t idx, bool p32,
                                             uint32_t r, W at) {
  res[idx] = r;
  if (p32)
    ((uint32_t*)pos)[idx] = (uint32_t)at;
  else
    ((uint64_t*)pos)[idx] = at == (W)~(W)0 ? ~0ull : (uint64_t)at;
}

// Row layout of a wave's copy phase, wave-uniform: with R 16-byte pieces per
// row, R <= 64 puts 64 / R whole rows on the wave per step (lane -> row
// lane / R, piece lane % R); a longer row takes the whole wave, 64 pieces
// per step.
struct RowPlan {
  uint32_t R, rpi;  // pieces per row, rows per step
};

inline RowPlan row_plan(uint32_t row_bytes) {
  RowPlan rp;
  rp.R = row_bytes / 16;
  rp.rpi = rp.R <= 64 ? 64 / rp.R : 1;
  return rp;
}

inline bool narrow(const HtGeom& g) { return g.mask < (1ull << 32) && g.size < (1ull << 32); }

}  // namespace htf
}  // namespace kvh
