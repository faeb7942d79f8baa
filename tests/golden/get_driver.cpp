/*
 * tests/golden/get_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Driver for tests/golden/make_get_golden.py, which compiles it against the
 * reference's headers and oracle/_ref/libkvref_ht.so (the unmodified KV-core
 * sources, oracle/Makefile) into a temporary directory.  It fills a malloc()
 * HashTab that has data segments (HashTab::alloc_map with max_value_size > 0
 * and hash_value_ratio < 1) through the reference's own write path and then
 * asks the reference's read path for every query:
 *
 *   insert     kb.set(idx), set_hash, acquire, resize(&p, size1[i]), fill
 *              byte j = (u8)(idx * 131 + j), release
 *   resize     every resize_every-th key: acquire, resize(&p, size2[i]), fill
 *              byte j = (u8)(idx * 131 + j + 1), release
 *   stamp      every stamp_every-th key: acquire, update_stamps(0, t), release
 *   tombstone  every tomb_every-th key: acquire, tombstone, release
 *   get        find: status, kctx.pos (~0 when find left it unset),
 *              kctx.chains, kctx.inc; after KEY_OK, value(&ptr, size): status,
 *              size, the bytes, and where ptr points -- kctx.entry and
 *              kctx.msg are copies in work memory, so the offset of ptr within
 *              them plus kctx.pos (entry) or kctx.geom (message)
 *
 * and copies out ht[0 .. ht_size) and the segments.  The entry's flags are
 * recorded after each write step.  No reference source is copied here.
 */
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <raikv/shm_ht.h>
#include <raikv/key_ctx.h>
#include <raikv/key_buf.h>
#include <raikv/msg_ctx.h>
#include <raikv/work.h>

using namespace rai::kv;

struct GetTable {
  uint64_t map_size;
  uint32_t max_value_size, entry_size;
  float    ratio;
  uint16_t buckets;
  uint8_t  arity;
  uint32_t resize_every, stamp_every, tomb_every;
};

static void fill( uint8_t *p, uint64_t idx, uint32_t sz, uint32_t pass ) {
  for ( uint32_t j = 0; j < sz; j++ )
    p[ j ] = (uint8_t) ( idx * 131 + j + pass );
}

/* Returns ht_size, or a negative number: -1 no map, -2 no context, -3 an output
 * is too small, -(100 + 10 * i + step) write step 0 .. 3 of key i failed.
 * hdr_out = {ht_mod_mask, ht_mod_fraction, ht_mod_shift, ht_size, nsegs,
 * seg_size, seg_start, seg_align_shift}.  flags_out = 3 u16 per key: the
 * entry's flags after insert, after the second resize, after the stamp.
 * vloc: bit 63 set = offset in the segment area, clear = offset in ht[]. */
extern "C" long ref_get_table( const GetTable *t, const uint64_t *ins, size_t n_ins, const uint32_t *size1,
                               const uint32_t *size2, const uint64_t *q, size_t nq, int32_t *status,
                               uint64_t *pos, uint64_t *chains, uint8_t *inc, int32_t *vstatus,
                               uint64_t *vsize, uint64_t *vloc, uint8_t *blob, size_t blob_cap,
                               uint64_t *blob_offs, uint16_t *flags_out, uint8_t *image, size_t image_cap,
                               uint8_t *segs, size_t segs_cap, uint64_t *hdr_out ) {
  HashTabGeom g;
  memset( &g, 0, sizeof( g ) );
  g.map_size         = t->map_size;
  g.max_value_size   = t->max_value_size;
  g.hash_entry_size  = t->entry_size;
  g.hash_value_ratio = t->ratio;
  g.cuckoo_buckets   = t->buckets;
  g.cuckoo_arity     = t->arity;
  HashTab *ht = HashTab::alloc_map( g );
  if ( ht == NULL ) return -1;
  const uint32_t ctx_id = ht->attach_ctx( 1 );
  if ( ctx_id == KV_NO_CTX_ID ) { ::free( ht ); return -2; }
  const uint32_t dbx_id = ht->attach_db( ctx_id, 0 );
  if ( dbx_id == KV_NO_DBSTAT_ID ) { ::free( ht ); return -2; }
  const uint32_t es = t->entry_size;
  const uint64_t seg_size = ht->hdr.seg_size(), stamp = 1700000000ULL * 1000000000ULL;
  long rc = (long) ht->hdr.ht_size;
  {
    KeyBuf kb;
    KeyCtx kctx( *ht, dbx_id, &kb );
    WorkAlloc8k wrk;
    for ( size_t i = 0; i < n_ins && rc >= 0; i++ ) {
      const uint64_t idx = i;
      kb.set( idx );
      kctx.set_hash( ins[ 2 * i ], ins[ 2 * i + 1 ] );
      if ( kctx.acquire( &wrk ) != KEY_IS_NEW ) { rc = -(long) ( 100 + 10 * i ); break; }
      void *p = NULL;
      if ( kctx.resize( &p, size1[ i ] ) != KEY_OK ) rc = -(long) ( 100 + 10 * i );
      else fill( (uint8_t *) p, idx, size1[ i ], 0 );
      flags_out[ 3 * i ] = flags_out[ 3 * i + 1 ] = flags_out[ 3 * i + 2 ] = kctx.entry->flags;
      kctx.release();
    }
    for ( size_t i = 0; t->resize_every != 0 && i < n_ins && rc >= 0; i += t->resize_every ) {
      const uint64_t idx = i;
      kb.set( idx );
      kctx.set_hash( ins[ 2 * i ], ins[ 2 * i + 1 ] );
      if ( kctx.acquire( &wrk ) != KEY_OK ) { rc = -(long) ( 101 + 10 * i ); break; }
      void *p = NULL;
      if ( kctx.resize( &p, size2[ i ] ) != KEY_OK ) rc = -(long) ( 101 + 10 * i );
      else fill( (uint8_t *) p, idx, size2[ i ], 1 );
      flags_out[ 3 * i + 1 ] = flags_out[ 3 * i + 2 ] = kctx.entry->flags;
      kctx.release();
    }
    for ( size_t i = 0; t->stamp_every != 0 && i < n_ins && rc >= 0; i += t->stamp_every ) {
      const uint64_t idx = i;
      kb.set( idx );
      kctx.set_hash( ins[ 2 * i ], ins[ 2 * i + 1 ] );
      if ( kctx.acquire( &wrk ) != KEY_OK ) { rc = -(long) ( 102 + 10 * i ); break; }
      if ( kctx.update_stamps( 0, stamp ) != KEY_OK ) rc = -(long) ( 102 + 10 * i );
      flags_out[ 3 * i + 2 ] = kctx.entry->flags;
      kctx.release();
    }
    for ( size_t i = 0; t->tomb_every != 0 && i < n_ins && rc >= 0; i += t->tomb_every ) {
      const uint64_t idx = i;
      kb.set( idx );
      kctx.set_hash( ins[ 2 * i ], ins[ 2 * i + 1 ] );
      if ( kctx.acquire( &wrk ) != KEY_OK ) { rc = -(long) ( 103 + 10 * i ); break; }
      const KeyStatus ts = kctx.tombstone();
      kctx.release();
      if ( ts != KEY_OK ) rc = -(long) ( 103 + 10 * i );
    }
    uint64_t used = 0;
    for ( size_t i = 0; i < nq && rc >= 0; i++ ) {
      kctx.set_hash( q[ 2 * i ], q[ 2 * i + 1 ] );
      kctx.pos = ~(uint64_t) 0;
      kctx.inc = 0;
      status[ i ] = (int32_t) kctx.find( &wrk );
      pos[ i ]    = kctx.pos;
      chains[ i ] = kctx.chains;
      inc[ i ]    = kctx.inc;
      vstatus[ i ] = -1;
      vsize[ i ]   = 0;
      vloc[ i ]    = ~(uint64_t) 0;
      blob_offs[ i ] = used;
      if ( status[ i ] == (int32_t) KEY_OK ) {
        uint8_t *ptr = NULL;
        uint64_t sz  = 0;
        vstatus[ i ] = (int32_t) kctx.value( &ptr, sz );
        if ( vstatus[ i ] == (int32_t) KEY_OK ) {
          vsize[ i ] = sz;
          if ( kctx.msg != NULL )
            vloc[ i ] = ( (uint64_t) 1 << 63 ) | ( (uint64_t) kctx.geom.segment * seg_size + kctx.geom.offset +
                                                   (uint64_t) ( ptr - (uint8_t *) (void *) kctx.msg ) );
          else
            vloc[ i ] = kctx.pos * (uint64_t) es + (uint64_t) ( ptr - (uint8_t *) (void *) kctx.entry );
          if ( used + sz > blob_cap ) { rc = -3; break; }
          memcpy( &blob[ used ], ptr, sz );
          used += sz;
        }
      }
    }
    blob_offs[ nq ] = used;
  }
  hdr_out[ 0 ] = ht->hdr.ht_mod_mask;
  hdr_out[ 1 ] = ht->hdr.ht_mod_fraction;
  hdr_out[ 2 ] = ht->hdr.ht_mod_shift;
  hdr_out[ 3 ] = ht->hdr.ht_size;
  hdr_out[ 4 ] = ht->hdr.nsegs;
  hdr_out[ 5 ] = seg_size;
  hdr_out[ 6 ] = ht->hdr.seg_start();
  hdr_out[ 7 ] = ht->hdr.seg_align_shift;
  const size_t bytes = (size_t) ht->hdr.ht_size * es, sbytes = (size_t) ht->hdr.nsegs * seg_size;
  if ( rc >= 0 && bytes <= image_cap && sbytes <= segs_cap ) {
    memcpy( image, ht->get_entry( 0, es ), bytes );
    memcpy( segs, &( (uint8_t *) (void *) ht )[ ht->hdr.seg_start() ], sbytes );
  }
  else if ( rc >= 0 )
    rc = -3;
  ::free( ht );
  return rc;
}
