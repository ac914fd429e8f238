// host_blobs.h — bsg_pool_put_blobs / bsg_pool_get: blobs that are not part of a split run put
// into a pool, and blobs got out of one by ref, on the device (included by host_engine.h after
// host_blobpool.h).
#pragma once

namespace {

// The engine's side of both calls. It owns every buffer here and hashes through the engine's
// second engine, so the last run's records, dedup result, tree, walk, restore and gc results stay
// as they are; the put's first-occurrence pass and append are the pool's own (bsg_pool::put_items).
struct BlobWork {
  DevBuf span, refs, descs;                // put: the blobs' spans, their refs, a hash batch
  DevBuf in, res, part, touched, tpre, tlist;  // get: header | refs; idx | out_off; the passes'
  PinBuf h_span, h_in, h_hdr, h_res;
  Marks marks;                       // profile
  float ms[6] = {0, 0, 0, 0, 0, 0};  // profile: hash, dedup + plan, append + gather (the last
                                     //   put); probe + sum, verify, gather (the last get)

  // bsg_pool_put_blobs once the arguments and the states are checked: blob i is d_src[off[i] ..
  // + len[i]), all of them below `hi`. (The caller holds the pool's mutex.)
  int put(const RunView& v, bsg_pool& pool, const uint8_t* d_src, uint64_t hi, const uint64_t* off,
          const uint64_t* len, uint64_t n, uint8_t* refs_out, bsg_pool_put_info* info) {
    const hipStream_t s = v.stream;
    for (int i = 0; i < 3; ++i) ms[i] = 0.f;
    BlobPutArgs b{};
    if (n) {
      MCHECK(span.ensure(sizeof(BlobSpan) * n));
      MCHECK(refs.ensure(32 * n));
      MCHECK(h_span.ensure(sizeof(BlobSpan) * n));
      BlobSpan* hs = h_span.as<BlobSpan>();
      for (uint64_t i = 0; i < n; ++i) hs[i] = BlobSpan{off[i], len[i]};
      if (int rc = need_hasher(v.owner)) return rc;
      b.span = span.as<BlobSpan>();
      b.src = d_src;
      b.src_bytes = hi;
      b.refs = refs.as<uint8_t>();
    }
    const int rc = pool.put_items(
        v, n, true, info,
        [&](PoolArgs& a) {
          a.d.refs = b.refs;
          a.d.stride = 32;
          a.d.lens = reinterpret_cast<const uint8_t*>(b.span) + offsetof(BlobSpan, len);
          a.d.len_stride = sizeof(BlobSpan);
        },
        [&](const PoolArgs& a) {  // the spans up, the hash runs, the refs down
          b.p = a;
          if (v.profile) marks.record(0, s);
          HCHECK(hipMemcpyAsync(span.p, h_span.p, sizeof(BlobSpan) * n, hipMemcpyHostToDevice, s));
          const int hrc = hash_batches(
              v.owner, descs, n, d_src, hi, long_mode(),
              [&](uint64_t b0, uint32_t nb, StreamDesc* d) {
                return launch_blob_descs(b, b0, nb, d, s, v.num_cus);
              },
              [&](uint64_t b0, uint32_t nb, const ChunkRec* rec, Counters* ctr) {
                return launch_blob_refs(b, b0, nb, rec, ctr, s, v.num_cus);
              });
          if (hrc) return hrc;
          if (v.profile) marks.record(1, s);
          // (the put's first readback waits for it, and returns before the capacity is looked at)
          if (refs_out) HCHECK(hipMemcpyAsync(refs_out, refs.p, 32 * n, hipMemcpyDeviceToHost, s));
          return (int)BSG_OK;
        },
        [&](const PoolArgs& a) {
          b.p = a;
          return dbg("launch_pool_gather_blobs", s, launch_pool_gather_blobs(b, s));
        });
    if (rc == BSG_OK && n && v.profile) {
      ms[0] = marks.ms(0, 1);
      ms[1] = pool.ms[0];
      ms[2] = pool.ms[1] + pool.ms[2];
    }
    return rc;
  }

  int readback(hipStream_t s, GetHdr* h) {
    return read_header(h_hdr, in.p, s, h, [](const GetHdr& g) { return g.r.dd.error; }, "pool get");
  }

  // bsg_pool_get once the arguments and the states are checked. Two phases with one readback in
  // between (two more with the flag): the probe and the requests' places, then the gather. Nothing
  // of the pool is written. (The caller holds the pool's mutex.)
  int get(const RunView& v, const bsg_pool& pool, const uint8_t* rq, uint64_t n, uint8_t* d_out,
          uint64_t out_cap, int flags, uint64_t* idx, uint64_t* out_off, bsg_pool_get_info* info) {
    const hipStream_t s = v.stream;
    auto stamp = [&](size_t i) { v.profile ? marks.record(i, s) : void(); };
    for (int i = 3; i < 6; ++i) ms[i] = 0.f;
    const bool verify = (flags & BSG_GET_VERIFY) != 0;
    if (out_off) out_off[0] = 0;
    if (!n) return BSG_OK;

    // the input block: header | refs; the result block: idx | out_off
    const uint64_t in_bytes = sizeof(GetHdr) + 32 * n, res_bytes = 8 * n + 8 * (n + 1);
    MCHECK(h_in.ensure(in_bytes));
    MCHECK(h_hdr.ensure(sizeof(GetHdr) + 16));
    MCHECK(h_res.ensure(res_bytes));
    MCHECK(in.ensure(in_bytes));
    MCHECK(res.ensure(res_bytes));
    MCHECK(part.ensure(8 * sum_parts(std::max(n, pool.nblobs))));
    if (verify) MCHECK(touched.ensure(std::max<uint64_t>(pool.nblobs, 1)));
    {
      GetHdr h0{};
      h0.r.missing = h0.r.mismatch = h0.r.bad_blob = ~0ull;
      std::memcpy(h_in.p, &h0, sizeof h0);
      std::memcpy(h_in.as<uint8_t>() + sizeof(GetHdr), rq, 32 * n);
    }
    GetArgs a{};
    a.pool = pool.bytes.as<const uint8_t>();
    a.pool_bytes = pool.pool_bytes();
    a.table = pool.table.as<const PoolBlob>();
    a.nblobs = pool.nblobs;
    a.index = pool.index.as<const uint64_t>();
    a.index_mask = pool.slots - 1;
    a.refs = in.as<uint8_t>() + sizeof(GetHdr);
    a.n = n;
    a.idx = res.as<uint64_t>();
    a.out_off = res.as<uint64_t>() + n;
    a.part = part.as<uint64_t>();
    a.touched = verify ? touched.as<uint8_t>() : nullptr;
    a.hdr = in.as<GetHdr>();
    a.out = d_out;

    stamp(0);
    HCHECK(hipMemcpyAsync(in.p, h_in.p, in_bytes, hipMemcpyHostToDevice, s));
    if (verify && pool.nblobs) HCHECK(hipMemsetAsync(touched.p, 0, pool.nblobs, s));
    HCHECK(dbg("launch_get_probe", s, launch_get_probe(a, s, v.num_cus)));
    stamp(1);
    HCHECK(hipMemcpyAsync(h_res.p, res.p, res_bytes, hipMemcpyDeviceToHost, s));
    GetHdr h;
    int rc;
    if ((rc = readback(s, &h))) return rc;
    if (v.profile) ms[3] = marks.ms(0, 1);
    const uint64_t* hidx = h_res.as<uint64_t>();
    const uint64_t* hoff = hidx + n;
    const uint64_t total = hoff[n];
    if (h.found > n || total % 16 || h.bytes > total || total - h.bytes > 15 * h.found)
      return BSG_EDEVICE;
    if (idx) std::copy(hidx, hidx + n, idx);
    if (out_off) std::copy(hoff, hoff + n + 1, out_off);
    info->found = h.found;
    info->missing = n - h.found;
    info->bytes = h.bytes;
    info->need_bytes = total;
    if (d_out && total > out_cap) return BSG_ENOMEM;

    // the found blobs, each once: their list and their layout, then the hash runs
    if (verify && h.found) {
      const uint64_t cap = std::min(pool.nblobs, h.found);
      MCHECK(tpre.ensure(8 * (pool.nblobs + 1)));
      MCHECK(tlist.ensure(8 * cap));
      TouchArgs t{};
      t.r.pool = a.pool;
      t.r.pool_bytes = a.pool_bytes;
      t.r.blobs = a.table;
      t.r.nblobs = a.nblobs;
      t.r.hdr = &a.hdr->r;
      t.r.touched = a.touched;
      t.tpre = tpre.as<uint64_t>();
      t.tlist = tlist.as<uint64_t>();
      t.ntouched = cap;
      t.verified = &a.hdr->verified;
      t.part = a.part;
      stamp(2);
      HCHECK(dbg("launch_read_touched", s, launch_read_touched(t, s, v.num_cus)));
      uint64_t* nt = reinterpret_cast<uint64_t*>(h_hdr.as<uint8_t>() + sizeof(GetHdr));
      HCHECK(hipMemcpyAsync(nt, t.tpre + a.nblobs, 8, hipMemcpyDeviceToHost, s));
      if ((rc = readback(s, &h))) return rc;
      // (a pool's blobs meet the hash path's layout rules by construction)
      if (*nt > cap || *nt == 0 || h.r.invalid) return BSG_EDEVICE;
      t.ntouched = *nt;
      if ((rc = hash_touched(v, t, descs, pool.used))) return rc;
      stamp(3);
      if ((rc = readback(s, &h))) return rc;
      if (v.profile) ms[4] = marks.ms(2, 3);
      info->verified = h.verified;
      info->bad_blob = h.r.bad_blob;
      if (h.r.bad_blob != ~0ull) return BSG_ECORRUPT;
    }
    if (!d_out) return BSG_OK;

    a.total = total;
    stamp(4);
    HCHECK(dbg("launch_get_gather", s, launch_get_gather(a, s)));
    stamp(5);
    if ((rc = readback(s, &h))) return rc;
    if (v.profile) ms[5] = marks.ms(4, 5);
    return BSG_OK;
  }
};

}  // namespace
