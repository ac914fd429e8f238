// host_restore.h — bsg_engine_restore: streams from a pool of blobs (included by host_engine.h).
#pragma once

namespace {

// The call owns every buffer here (and hashes the pool through the engine's second engine), so
// the last run's records, dedup result and tree stay as they are.
struct RestoreWork {
  DevBuf in, seg, runs, descs;
  RefTable tab;
  PinBuf h_in, h_hdr;
  Marks marks;              // profile
  float ms[3] = {0, 0, 0};  // profile: index + resolve + tiling, verify, scatter

  int readback(hipStream_t s, RestoreHdr* h) {
    return read_header(h_hdr, in.p, s, h, [](const RestoreHdr& r) { return r.dd.error; },
                       "restore");
  }

  // The host checks what it can from its own arrays (pointers, alignment, the output ranges,
  // the blobs' bounds); the records, in their hundreds of thousands, are resolved and checked
  // on the device. Nothing is written to d_out before the header has come back clean.
  // The records come from the host (recs, uploaded with the rest) or, with d_recs, are read where
  // they lie on the device (bsg_engine_restore_walk). With `ps` the table and the index are a
  // bsg_pool's, read where they lie (bsg_pool_restore_walk).
  int run(const RunView& v, const uint8_t* d_pool, uint64_t pool_bytes,
          const bsg_pool_blob* blobs, uint64_t nblobs, const bsg_chunk* recs, uint64_t nrecs,
          const ChunkRec* d_recs, uint8_t* d_out, uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len,
          uint32_t ns, int flags, bsg_restore_info* info, const PoolSrc* ps = nullptr) {
    const hipStream_t stream = v.stream;
    auto mark = [&](size_t i) { v.profile ? marks.record(i, stream) : void(); };
    auto elapsed = [&](size_t i, size_t j) { return v.profile ? marks.ms(i, j) : 0.f; };
    const bool verify = (flags & BSG_RESTORE_VERIFY) != 0;
    if (flags & ~BSG_RESTORE_VERIFY) return BSG_EINVAL;
    if ((!d_pool && pool_bytes) || (!blobs && !ps && nblobs) || (!recs && !d_recs && nrecs) || (!d_out && out_cap) ||
        (ns && (!out_off || !out_len)))
      return BSG_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return BSG_EINVAL;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_pool), p1 = p0 + pool_bytes;
    const uintptr_t ob = reinterpret_cast<uintptr_t>(d_out);
    if (p1 < p0 || ob + out_cap < ob) return BSG_EINVAL;

    // the input block: header | blobs | records | out_off | out_len | tile prefix
    auto pad16 = [](uint64_t v) { return (v + 15) & ~15ull; };
    const uint64_t o_blobs = sizeof(RestoreHdr);
    const uint64_t o_recs = o_blobs + (ps ? 0 : pad16(sizeof(PoolBlob) * nblobs));
    const uint64_t o_off = o_recs + (d_recs ? 0 : pad16(sizeof(ChunkRec) * nrecs));
    const uint64_t o_len = o_off + pad16(8ull * ns);
    const uint64_t o_tpre = o_len + pad16(8ull * ns);
    const uint64_t in_bytes = o_tpre + pad16(8ull * (ns + 1ull));
    MCHECK(h_in.ensure(in_bytes));
    MCHECK(h_hdr.ensure(sizeof(RestoreHdr)));
    uint8_t* hin = h_in.as<uint8_t>();
    uint64_t* tpre = reinterpret_cast<uint64_t*>(hin + o_tpre);

    uint64_t total = 0, tiles = 0;
    std::vector<std::pair<uint64_t, uint64_t>> spans;  // the non-empty output ranges
    for (uint32_t s = 0; s < ns; ++s) {
      if (out_off[s] % 16 != 0 || out_off[s] > out_cap || out_len[s] > out_cap - out_off[s])
        return BSG_EINVAL;
      tpre[s] = tiles;
      if (!out_len[s]) continue;
      const uintptr_t o0 = ob + out_off[s], o1 = o0 + out_len[s];
      if (pool_bytes && o0 < p1 && p0 < o1) return BSG_EINVAL;  // the output inside the pool
      spans.emplace_back(out_off[s], out_off[s] + out_len[s]);
      total += out_len[s];
      tiles += (out_len[s] + kRestoreTile - 1) / kRestoreTile;
    }
    tpre[ns] = tiles;
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
      if (spans[k].first < spans[k - 1].second) return BSG_EINVAL;
    if (tiles > 0x7fffffffull) return BSG_EINVAL;

    uint64_t blob_bytes = 0, blob_hi = 0;
    if (ps) {  // the pool's invariant: every blob at a multiple of 16 in [0, used)
      if (ps->used > pool_bytes || (verify && ps->used >= (1ull << 40))) return BSG_EINVAL;
      blob_bytes = ps->blob_bytes;
      blob_hi = ps->used;
    }
    for (uint64_t k = 0; k < nblobs && !ps; ++k) {
      if (blobs[k].off > pool_bytes || blobs[k].len > pool_bytes - blobs[k].off) return BSG_EINVAL;
      if (verify && (blobs[k].off % 16 != 0 || blobs[k].len >= (1ull << 40))) return BSG_EINVAL;
      blob_bytes += blobs[k].len;
      blob_hi = std::max<uint64_t>(blob_hi, blobs[k].off + blobs[k].len);
    }
    // the engine hash path's own rules (bsg_engine_hash)
    if (verify && nblobs && (p0 % 16 != 0 || pool_bytes - blob_hi < kReadSlack)) return BSG_EINVAL;

    RestoreHdr* h0 = reinterpret_cast<RestoreHdr*>(hin);
    *h0 = RestoreHdr{};
    h0->missing = h0->mismatch = h0->bad_blob = ~0ull;
    if (nblobs && !ps) std::memcpy(hin + o_blobs, blobs, sizeof(PoolBlob) * nblobs);
    if (nrecs && !d_recs) std::memcpy(hin + o_recs, recs, sizeof(ChunkRec) * nrecs);
    if (ns) {
      std::memcpy(hin + o_off, out_off, 8ull * ns);
      std::memcpy(hin + o_len, out_len, 8ull * ns);
    }

    const uint64_t ns1 = ns ? ns : 1;
    MCHECK(in.ensure(in_bytes));
    if (!ps) MCHECK(tab.reserve(nblobs));
    MCHECK(seg.ensure(8 * (nrecs ? nrecs : 1)));
    MCHECK(runs.ensure(16 * ns1));
    RestoreArgs a{};
    a.pool = d_pool;
    a.pool_bytes = pool_bytes;
    a.blobs = ps ? ps->table : reinterpret_cast<const PoolBlob*>(in.as<uint8_t>() + o_blobs);
    a.nblobs = nblobs;
    a.rec = d_recs ? d_recs : reinterpret_cast<const ChunkRec*>(in.as<uint8_t>() + o_recs);
    a.nrec = nrecs;
    a.out_off = reinterpret_cast<const uint64_t*>(in.as<uint8_t>() + o_off);
    a.out_len = reinterpret_cast<const uint64_t*>(in.as<uint8_t>() + o_len);
    a.tpre = reinterpret_cast<const uint64_t*>(in.as<uint8_t>() + o_tpre);
    a.ns = ns;
    a.tab = ps ? ps->index : tab.p();
    a.tab_mask = ps ? ps->mask : tab.mask();
    a.seg = seg.as<uint64_t>();
    a.sfirst = runs.as<uint64_t>();
    a.slast = runs.as<uint64_t>() + ns1;
    a.out = d_out;
    a.hdr = in.as<RestoreHdr>();

    int rc;
    mark(0);
    HCHECK(hipMemcpyAsync(in.p, hin, in_bytes, hipMemcpyHostToDevice, stream));
    if (!ps) HCHECK(tab.clear(stream));
    HCHECK(hipMemsetAsync(runs.p, 0xFF, 16 * ns1, stream));
    HCHECK(dbg("launch_restore_resolve", stream,
               launch_restore_resolve(a, !ps, stream, v.num_cus)));
    mark(1);
    if (verify && nblobs) {
      if ((rc = need_hasher(v.owner))) return rc;
      rc = hash_batches(
          v.owner, descs, nblobs, d_pool, blob_hi, long_mode(),
          [&](uint64_t b, uint32_t nb, StreamDesc* d) {
            return launch_restore_descs(a, b, nb, d, stream, v.num_cus);
          },
          [&](uint64_t b, uint32_t nb, const ChunkRec* rec, Counters* ctr) {
            return launch_restore_compare(a, b, nb, rec, ctr, stream, v.num_cus);
          });
      if (rc) return rc;
    }
    mark(2);
    RestoreHdr h;
    if ((rc = readback(stream, &h))) return rc;
    ms[0] = elapsed(0, 1);
    ms[1] = elapsed(1, 2);
    ms[2] = 0.f;
    if (h.invalid) return BSG_EINVAL;
    if (info && verify) {
      info->verified = blob_bytes;
      info->bad_blob = h.bad_blob;
    }
    if (h.missing != ~0ull) {
      if (info) info->bad_record = h.missing;
      return BSG_ENOTFOUND;
    }
    if (info) info->bad_record = h.mismatch;
    if (h.mismatch != ~0ull || (verify && h.bad_blob != ~0ull)) return BSG_ECORRUPT;
    if (v.in_flight) return BSG_ESTATE;

    mark(3);
    HCHECK(dbg("launch_restore_scatter", stream, launch_restore_scatter(a, tiles, stream)));
    mark(4);
    if ((rc = readback(stream, &h))) return rc;
    ms[2] = elapsed(3, 4);
    if (info) info->bytes = total;
    return BSG_OK;
  }
};

}  // namespace
