/*
 * tests/golden/find_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Driver for tests/golden/make_find_golden.py, which compiles it against the
 * reference's headers and oracle/_ref/libkvref_ht.so (the unmodified KV-core
 * sources, oracle/Makefile) into a temporary directory.  It fills a malloc()
 * HashTab (HashTab::alloc_map, src/ht_init.cpp:252-261) through the
 * reference's own write path and then asks the reference's read path
 * (KeyCtx::find, include/raikv/ht_search.h:308-367) for every query:
 *
 *   insert     set_hash, acquire, resize(&p, 8) + memcpy of the key index (an
 *              immediate value), release
 *   tombstone  every tomb_every-th inserted key: acquire, tombstone, release
 *   find       status, kctx.pos (~0 when find left it unset), kctx.chains,
 *              kctx.inc
 *
 * and copies out ht[0 .. ht_size).  No reference source is copied here.
 */
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <raikv/shm_ht.h>
#include <raikv/key_ctx.h>
#include <raikv/key_buf.h>
#include <raikv/work.h>

using namespace rai::kv;

/* Returns ht_size, or a negative number: -1 no map, -2 no context, -(100 + i)
 * insert i did not end KEY_IS_NEW + KEY_OK, -(1000000 + i) tombstone i failed.
 * geom_out = {ht_mod_mask, ht_mod_fraction, ht_mod_shift, ht_size}.
 * image = ht_size * entry_size bytes (image_cap >= that). */
extern "C" long ref_find_table(uint64_t slots, uint32_t entry_size, uint16_t buckets, uint8_t arity,
                               const uint64_t *ins, size_t n_ins, uint32_t tomb_every,
                               const uint64_t *q, size_t nq, int32_t *status, uint64_t *pos,
                               uint64_t *chains, uint8_t *inc, uint8_t *image, size_t image_cap,
                               uint64_t *geom_out) {
  HashTabGeom g;
  memset(&g, 0, sizeof(g));
  g.map_size = (uint64_t)(KV_HT_HDR_SIZE + KV_HT_CTX_SIZE + KV_HT_STATS_SIZE) + (uint64_t)entry_size * slots;
  g.max_value_size = 0;
  g.hash_entry_size = entry_size;
  g.hash_value_ratio = 1.0f;
  g.cuckoo_buckets = buckets;
  g.cuckoo_arity = arity;
  HashTab *ht = HashTab::alloc_map(g);
  if (ht == NULL) return -1;
  const uint32_t ctx_id = ht->attach_ctx(1);
  if (ctx_id == KV_NO_CTX_ID) { ::free(ht); return -2; }
  const uint32_t dbx_id = ht->attach_db(ctx_id, 0);
  if (dbx_id == KV_NO_DBSTAT_ID) { ::free(ht); return -2; }
  long rc = (long)ht->hdr.ht_size;
  {
    KeyBuf kb;
    KeyCtx kctx(*ht, dbx_id, &kb);
    WorkAlloc8k wrk;
    for (size_t i = 0; i < n_ins && rc >= 0; i++) {
      const uint64_t idx = i;
      kb.set(idx);
      kctx.set_hash(ins[2 * i], ins[2 * i + 1]);
      if (kctx.acquire(&wrk) != KEY_IS_NEW) { rc = -(long)(100 + i); break; }
      void *p = NULL;
      if (kctx.resize(&p, 8) != KEY_OK) { kctx.release(); rc = -(long)(100 + i); break; }
      memcpy(p, &idx, 8);
      kctx.release();
    }
    for (size_t i = 0; tomb_every != 0 && i < n_ins && rc >= 0; i += tomb_every) {
      const uint64_t idx = i;
      kb.set(idx);
      kctx.set_hash(ins[2 * i], ins[2 * i + 1]);
      if (kctx.acquire(&wrk) != KEY_OK) { rc = -(long)(1000000 + i); break; }
      const KeyStatus t = kctx.tombstone();
      kctx.release();
      if (t != KEY_OK) rc = -(long)(1000000 + i);
    }
    for (size_t i = 0; i < nq && rc >= 0; i++) {
      kctx.set_hash(q[2 * i], q[2 * i + 1]);
      kctx.pos = ~(uint64_t)0;
      kctx.inc = 0;
      status[i] = (int32_t)kctx.find(&wrk);
      pos[i] = kctx.pos;
      chains[i] = kctx.chains;
      inc[i] = kctx.inc;
    }
  }
  geom_out[0] = ht->hdr.ht_mod_mask;
  geom_out[1] = ht->hdr.ht_mod_fraction;
  geom_out[2] = ht->hdr.ht_mod_shift;
  geom_out[3] = ht->hdr.ht_size;
  const size_t bytes = (size_t)ht->hdr.ht_size * entry_size;
  if (rc >= 0 && bytes <= image_cap)
    memcpy(image, ht->get_entry(0, entry_size), bytes);
  else if (rc >= 0)
    rc = -3;
  ::free(ht);
  return rc;
}
