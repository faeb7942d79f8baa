// ht_get.hip -- batched read-only get over device-resident copies of a raikv
// hash table's ht[] and of its data segments (kvh_ht_get): KeyCtx::find
// (include/raikv/ht_search.h:308-367) followed by KeyCtx::value
// (src/key_ctx.cpp:959-1001) for n keys in one launch, on images that cannot
// change; and kvh_seg_geom_init, the segment geometry of HashTab::initialize
// (src/ht_init.cpp:118-192) on the host.
//
//   k_get<A,W>   (h1,h2) pairs resident in HBM -> slot, status, value size,
//                value location, optionally the value bytes
//
// Phase 1, one lane per key: the walk of ht_find_dev.hpp (find_one, the same
// code k_find runs).  A KEY_OK lane then reads flags | keylen (u32 at +20) and
// the ValueCtr word (es - 8) of its entry and switches as value() does on
// FL_SEGMENT_VALUE | FL_IMMEDIATE_VALUE:
//   immediate   size = ValueCtr::size, data after the key part
//               (HashEntry::hdr_size2, hash_entry.h:276-281)
//   segment     the ValuePtr before the stamps (HashEntry::value_ptr,
//               hash_entry.h:333-340) -> ValueGeom -> HashTab::seg_data
//               (shm_ht.h:468-474) -> the message's 48 leading bytes, three
//               16-byte loads issued together -> MsgHdr::check_seal
//               (msg_ctx.h:113-132) with the trailer ValueCtr at size - 8
//   neither or both  KEY_NO_VALUE
// A pointer or a header that fails seg_data or check_seal is KEY_MUTATED, as
// attach_msg(ATTACH_READ) + is_msg_valid() report it (key_ctx.cpp:481-524,
// :565-571).  The reference trusts a live table and checks no bounds; this
// kernel never reads outside the two images, so a ValuePtr whose message
// would leave its segment, a msg_size that leaves its message and an
// immediate size that leaves its entry are KEY_MUTATED too: every load below
// is issued only after the check that proves it in bounds.
// The chain entry -> ValuePtr -> message header -> trailer is three dependent
// random loads after the walk: latency bound, hidden by occupancy as in
// k_find (no LDS, small workgroups, one-shot grid).
//
// Phase 2, the same kernel: the wave's 64 (location, size) results stay in
// registers; stride / 16 lanes cooperate on one row, reading the owner
// lane's result by wave shuffles, so every store instruction writes one
// contiguous run of 16-byte pieces.  Value sources are only 8-byte aligned
// (24 + align8(keylen) in an entry, an 8-aligned header in a 64-aligned
// message), so a piece is two 8-byte loads; a word that starts at or past the
// value's size is not loaded, the bytes of the last word past the size are
// masked, and the rest of the row is zero-filled in the same pass.  An 8-byte
// word that starts inside a value ends inside its container: both the entry's
// value area (ends at es - 8) and a message's (ends at msg.size - 8, msg.size
// a multiple of the segment alignment) end 8-byte aligned.
// Both images are only read; results go out through plain vector stores.
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

constexpr int kGetBlock = 256;  // no LDS: small groups, many waves per CU

constexpr uint32_t kKeyMutated = 6, kKeyNoValue = 8;  // KeyStatus, key_ctx.h
// KeyValueFlags, hash_entry.h:115-132
constexpr uint32_t kFlSeqno = 0x10, kFlSegment = 0x40, kFlImmediate = 0x100, kFlPartKey = 0x400;
constexpr uint32_t kFlStamps = 0x1000 | 0x2000, kFlBusy = 0x8000;
constexpr uint32_t kMsgHead = 48;  // the three 16-byte loads: MsgHdr (40 bytes with a 4-byte key) and 8 more
constexpr uint64_t kLocSeg = 1ull << 63;

struct SegImage {
  const uint8_t* seg;  // map + seg_start
  uint64_t seg_size;
  uint32_t nsegs, shift;
};

__device__ __forceinline__ uint32_t align8(uint32_t x) { return (x + 7u) & ~7u; }

// KeyCtx::value for the sealed entry at `slot` that find matched to (h1, h2):
// -> KEY_OK with (loc, len), or KEY_MUTATED / KEY_NO_VALUE
__device__ __forceinline__ uint32_t value_one(const Image& im, const SegImage& sg, uint64_t h1, uint64_t h2,
                                              uint64_t slot, uint64_t& loc, uint32_t& len) {
  const uint8_t* e = entry_at(im, slot);
  const uint32_t fk = *(const uint32_t*)(e + 20);  // flags u16 at +20, keylen u16 at +22
  const uint32_t ctr = *(const uint32_t*)(e + im.es - 8);
  const uint32_t fl = fk & 0xFFFFu;
  const uint32_t kind = fl & (kFlSegment | kFlImmediate);
  if (kind == kFlImmediate) {
    const uint32_t size = ctr & 0x7FFFu;  // ValueCtr::size
    const uint32_t off = 24u + ((fl & kFlPartKey) ? 0u : align8(fk >> 16));
    if (off + size > im.es - 8u) return kKeyMutated;
    loc = slot * (uint64_t)im.es + off;
    len = size;
    return kKeyOk;
  }
  if (kind != kFlSegment) return kKeyNoValue;
  // es >= 64: the ValuePtr starts at es - 40 >= 24 at the lowest, behind the header
  const uint32_t vpo = im.es - 24u - ((fl & kFlStamps) ? 8u : 0u) - ((fl & kFlSeqno) ? 8u : 0u);
  const v2u p0 = *(const v2u*)(e + vpo), p1 = *(const v2u*)(e + vpo + 8);
  const uint32_t segment = p0.x & 0xFFFFu, serialhi = p0.x >> 16, seriallo = p0.y;
  const uint64_t gsize = (uint64_t)p1.x << sg.shift, goff = (uint64_t)p1.y << sg.shift;
  if (segment >= sg.nsegs || goff >= sg.seg_size) return kKeyMutated;            // seg_data
  if (gsize < kMsgHead || gsize > sg.seg_size - goff) return kKeyMutated;        // the message stays in its segment
  const uint64_t moff = (uint64_t)segment * sg.seg_size + goff;
  const uint8_t* m = sg.seg + moff;
  const v4u a = *(const v4u*)m, b = *(const v4u*)(m + 16), c = *(const v4u*)(m + 32);
  __builtin_amdgcn_sched_barrier(0);  // the three header loads in flight together
  // a = size, msg_size, hash; b = hash2, seriallo, db | type << 8 | flags << 16; c.x = keylen | key bytes
  const bool hdr_sealed = (uint64_t)a.x == gsize && ((uint64_t)a.z | ((uint64_t)a.w << 32)) == h1 &&
                          ((uint64_t)b.x | ((uint64_t)b.y << 32)) == h2 && ((b.w >> 16) & kFlBusy) == 0;
  if (!hdr_sealed) return kKeyMutated;
  const v2u t = *(const v2u*)(m + gsize - 8);  // trailer ValueCtr: in the message, msg.size == gsize
  if (t.y != seriallo || (t.x >> 16) != serialhi || !(t.x & kSealBit) || b.z != seriallo) return kKeyMutated;
  const uint32_t doff = align8(34u + (c.x & 0xFFFFu));  // MsgHdr::hdr_size
  if ((uint64_t)doff + a.y + 8u > gsize) return kKeyMutated;
  loc = kLocSeg | (moff + doff);
  len = a.y;  // msg_size
  return kKeyOk;
}

__device__ __forceinline__ v2u keep_bytes(v2u w, uint32_t nbytes) {  // nbytes >= 1
  if (nbytes >= 8) return w;
  const uint64_t m = (1ull << (8 * nbytes)) - 1;
  return v2u{w.x & (uint32_t)m, w.y & (uint32_t)(m >> 32)};
}

// The wave's keys b .. b + 63 (lane l owns key b + l: loc, len; len 0 for a
// key that is not KEY_OK) -> rows of `rows`: the first min(len, stride) value
// bytes, then zeros.  Called by all 64 lanes.
__device__ __forceinline__ void gather_values(const Image& im, const SegImage& sg, uint8_t* __restrict__ rows,
                                              const RowPlan rp, uint32_t stride, uint64_t b, uint64_t n, uint32_t lane,
                                              uint64_t loc, uint32_t len) {
  const bool wide = rp.R > 64;
  const uint32_t kk = wide ? 0u : lane / rp.R;
  const uint32_t p0 = wide ? lane : lane - kk * rp.R;
  const uint32_t pstep = wide ? 64u : rp.R;
  const bool act = kk < rp.rpi;
  const uint32_t loc_lo = (uint32_t)loc, loc_hi = (uint32_t)(loc >> 32);
  constexpr int U = 4;  // rows steps whose loads are issued before their stores
  for (uint32_t k0 = 0; k0 < 64; k0 += U * rp.rpi) {
    uint32_t k[U], cap[U];
    const uint8_t* src[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t row = k0 + u * rp.rpi + kk;
      k[u] = std::min<uint32_t>(row, 63u);
      const uint32_t lo = (uint32_t)__shfl((int)loc_lo, (int)k[u], 64);
      const uint32_t hi = (uint32_t)__shfl((int)loc_hi, (int)k[u], 64);
      const uint32_t ln = (uint32_t)__shfl((int)len, (int)k[u], 64);
      live[u] = act && row < 64 && b + row < n;
      cap[u] = live[u] ? std::min<uint32_t>(ln, stride) : 0u;  // 0: src is never dereferenced
      const uint64_t off = (uint64_t)lo | ((uint64_t)(hi & 0x7FFFFFFFu) << 32);
      src[u] = ((hi >> 31) ? sg.seg : im.ent) + off;
    }
    for (uint32_t p = p0; p < rp.R; p += pstep) {
      const uint32_t o = p * 16;
      v2u w0[U], w1[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        w0[u] = v2u{0u, 0u};
        w1[u] = v2u{0u, 0u};
        if (o < cap[u]) w0[u] = *(const v2u*)(src[u] + o);
        if (o + 8 < cap[u]) w1[u] = *(const v2u*)(src[u] + o + 8);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (live[u]) {
          if (o < cap[u]) w0[u] = keep_bytes(w0[u], cap[u] - o);
          if (o + 8 < cap[u]) w1[u] = keep_bytes(w1[u], cap[u] - o - 8);
          __builtin_nontemporal_store(v4u{w0[u].x, w0[u].y, w1[u].x, w1[u].y},
                                      (v4u*)(rows + (b + k[u]) * (uint64_t)stride + o));
        }
      }
    }
  }
}

template <int A, typename W>
__global__ void __launch_bounds__(kGetBlock)
k_get(Image im, SegImage sg, HtGeom g, const uint64_t* __restrict__ hashes, uint64_t n, void* __restrict__ pos,
      uint32_t* __restrict__ res, uint64_t* __restrict__ val_loc, uint32_t* __restrict__ val_len,
      uint8_t* __restrict__ rows, RowPlan rp, uint32_t stride, uint32_t p32) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t step = (((uint64_t)gridDim.x * blockDim.x) >> 6) * 64;
  const uint64_t last = n - 1;
  for (uint64_t b = wave * 64; b < n; b += step) {
    const uint64_t idx = b + lane;
    const v4u h = __builtin_nontemporal_load((const v4u*)(hashes + 2 * std::min<uint64_t>(idx, last)));
    const uint64_t h1 = (uint64_t)h.x | ((uint64_t)h.y << 32), h2 = (uint64_t)h.z | ((uint64_t)h.w << 32);
    W at;
    uint32_t r = find_one<A, W>(im, g, h1, h2, at);
    uint64_t loc = ~0ull;
    uint32_t len = 0;
    if ((r & 0xFFu) == kKeyOk) {
      const uint32_t vs = value_one(im, sg, h1, h2, (uint64_t)at, loc, len);
      if (vs != kKeyOk) {
        r = (r & ~0xFFu) | vs;
        loc = ~0ull;
        len = 0;
      }
    }
    if (idx <= last) {
      store_result<W>(pos, res, idx, p32 != 0, r, at);
      val_len[idx] = len;
      if (val_loc) val_loc[idx] = loc;
    }
    if (rows) gather_values(im, sg, rows, rp, stride, b, n, lane, loc, len);
  }
}

// ------------------------------------------------------------ host side
struct GetArgs {
  Image im;
  SegImage sg;
  HtGeom g;
  const uint64_t* h;
  uint64_t n;
  void* pos;
  uint32_t* res;
  uint64_t* loc;
  uint32_t* len;
  uint8_t* rows;
  RowPlan rp;
  uint32_t stride, p32;
  hipStream_t st;
};

template <int A>
void launch_get(const GetArgs& a) {
  // one-shot grid (the dispatcher hands blocks out in order); the loop in the kernel covers n beyond it
  const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((a.n + kGetBlock - 1) / kGetBlock, 1u << 30));
  if (narrow(a.g))
    hipLaunchKernelGGL((k_get<A, uint32_t>), dim3((uint32_t)grid), dim3(kGetBlock), 0, a.st, a.im, a.sg, a.g, a.h, a.n,
                       a.pos, a.res, a.loc, a.len, a.rows, a.rp, a.stride, a.p32);
  else
    hipLaunchKernelGGL((k_get<A, uint64_t>), dim3((uint32_t)grid), dim3(kGetBlock), 0, a.st, a.im, a.sg, a.g, a.h, a.n,
                       a.pos, a.res, a.loc, a.len, a.rows, a.rp, a.stride, a.p32);
}

int get_a(uint32_t arity, const GetArgs& a) {
  switch (arity) {
    case 1: launch_get<1>(a); break;
    case 2: launch_get<2>(a); break;
    case 3: launch_get<3>(a); break;
    case 4: launch_get<4>(a); break;
    case 5: launch_get<5>(a); break;
    case 6: launch_get<6>(a); break;
    case 7: launch_get<7>(a); break;
    case 8: launch_get<8>(a); break;
    default: return set_err(KVH_EINVAL);
  }
  return launch_done();
}

// the segment image: nsegs x seg_size bytes, messages aligned to 1 << shift (16 at the least, for the
// 16-byte header loads), offsets below bit 63 (the image bit of val_loc)
bool seg_geom_ok(const kvh_seg_geom_t* s) {
  if (!s || s->seg_align_shift > 31) return false;
  if (s->nsegs == 0) return true;
  if (s->seg_align_shift < 4 || s->seg_size == 0 || (s->seg_size & ((1ull << s->seg_align_shift) - 1)) != 0)
    return false;
  return s->nsegs <= 0x10000u && s->seg_size <= (1ull << 46);  // ValuePtr::segment is a u16
}

}  // namespace

extern "C" {

int kvh_seg_geom_init(uint64_t map_size, uint32_t hash_entry_size, float hash_value_ratio, uint32_t max_value_size,
                      kvh_seg_geom_t* out, uint64_t* seg_start) {
  // HashTab::initialize, src/ht_init.cpp:118-192 (header regions: include/raikv/shm_ht.h:59-69)
  const uint64_t hdr = (192ull + 128ull + 128ull) * 1024ull;
  const uint64_t kMaxSegs = 2032;  // HashHdr::SHM_MAX_SEG_COUNT (shm_ht.h:368-369): the Segment slots of the 192K header
  const uint64_t kMsgHdrSize = 40;  // sizeof( MsgHdr ), msg_ctx.h:53-62
  if (!out || map_size <= hdr || hash_entry_size == 0 || !(hash_value_ratio > 0.0f)) return set_err(KVH_EINVAL);
  const uint64_t area = map_size - hdr;
  const uint64_t entries = (uint64_t)((double)hash_value_ratio * (double)area) / (uint64_t)hash_entry_size;
  if (entries == 0 || entries > area / hash_entry_size) return set_err(KVH_EINVAL);
  const uint64_t tab = entries * (uint64_t)hash_entry_size;
  const uint64_t data = area - tab;
  uint32_t shift = 6;
  uint64_t nsegs = 0, seg_size = 0, start = 0;
  if (max_value_size != 0) {
    uint64_t max_sz = (uint64_t)max_value_size + 63 + kMsgHdrSize + 16;
    max_sz = (max_sz + 63) & ~63ull;
    while ((max_sz >> shift) > (1ull << 32)) shift++;
    nsegs = kMaxSegs;
    while (nsegs > 0 && data / nsegs < max_sz) nsegs--;
    while (nsegs > 16 && data / nsegs < max_sz * 16) nsegs--;
    if (nsegs == 0) return set_err(KVH_EINVAL);  // the reference asserts: no room for one value
    const uint64_t seg_off = hdr + tab;
    while ((seg_off >> shift) > (1ull << 32)) shift++;
    seg_size = (data / nsegs) & ~((1ull << shift) - 1);
    while ((seg_size >> shift) > (1ull << 32)) shift++;
    seg_size = (data / nsegs) & ~((1ull << shift) - 1);
    // as stored: u32 values in units of the alignment (FileHdr::seg_start, seg_size; shm_ht.h:174-179)
    start = (uint64_t)(uint32_t)(seg_off >> shift) << shift;
    seg_size = (uint64_t)(uint32_t)(seg_size >> shift) << shift;
  }
  out->seg_size = seg_size;
  out->nsegs = (uint32_t)nsegs;
  out->seg_align_shift = shift;
  if (seg_start) *seg_start = start;
  return set_err(0);
}

int kvh_ht_get(const void* entries, uint32_t hash_entry_size, const kvh_ht_geom_t* geom, const void* segments,
               const kvh_seg_geom_t* sgeom, const uint64_t* hashes, size_t n, void* pos, uint32_t* res,
               uint64_t* val_loc, uint32_t* val_len, void* values_out, uint32_t val_stride, uint32_t flags,
               void* stream) {
  const bool p32 = (flags & KVH_POS32) != 0;
  // 64 at the least: the ValuePtr (es - 40 at the lowest) never overlaps the 24-byte header
  if (hash_entry_size < 64 || (hash_entry_size & 31) != 0) return set_err(KVH_EINVAL);
  if (int rc = ht_check_geom(geom, p32)) return set_err(rc);
  if (!seg_geom_ok(sgeom)) return set_err(KVH_EINVAL);
  if (values_out && (val_stride == 0 || (val_stride & 15) != 0)) return set_err(KVH_EINVAL);
  if (n == 0) return set_err(0);
  if (!entries || ((uintptr_t)entries & 15) || !hashes || ((uintptr_t)hashes & 15) || !pos ||
      ((uintptr_t)pos & (p32 ? 3 : 7)) || !res || ((uintptr_t)res & 3) || !val_len || ((uintptr_t)val_len & 3) ||
      ((uintptr_t)val_loc & 7) || ((uintptr_t)values_out & 15) || ((uintptr_t)segments & 15) ||
      (sgeom->nsegs > 0 && !segments))
    return set_err(KVH_EINVAL);
  int cus = 0;
  int rc = device_cus(&cus);  // the first call on a device initialises the runtime, as the neighbours do
  if (rc) return rc;
  GetArgs a;
  a.im.ent = (const uint8_t*)entries;
  a.im.es = hash_entry_size;
  a.sg.seg = (const uint8_t*)segments;
  a.sg.seg_size = sgeom->seg_size;
  a.sg.nsegs = sgeom->nsegs;
  a.sg.shift = sgeom->seg_align_shift;
  a.g = ht_dev_geom(geom);
  a.h = hashes;
  a.n = n;
  a.pos = pos;
  a.res = res;
  a.loc = val_loc;
  a.len = val_len;
  a.rows = (uint8_t*)values_out;
  a.stride = values_out ? val_stride : 16u;
  a.rp = row_plan(a.stride);
  a.p32 = p32 ? 1u : 0u;
  a.st = (hipStream_t)stream;
  return get_a(ht_per_key(geom), a);
}

}  // extern "C"
