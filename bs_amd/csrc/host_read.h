// host_read.h — bsg_engine_read / bsg_pool_read: byte ranges of streams read out of a pool on the
// device (included by host_engine.h).
#pragma once

namespace {

// The hash runs of BSG_READ_VERIFY and BSG_MERGE_VERIFY: the blobs of t.tlist[0 .. t.ntouched)
// (launch_read_touched's list, its count read back) hashed through the engine's second engine in
// batches and held to their refs, on v's stream. The smallest failing blob index ends in
// t.r.hdr->bad_blob; the caller reads its header back. blob_hi: the end of the pool's last blob.
inline int hash_touched(const RunView& v, const TouchArgs& t, DevBuf& descs, uint64_t blob_hi) {
  if (!t.ntouched) return BSG_OK;
  if (int rc = need_hasher(v.owner)) return rc;
  return hash_batches(
      v.owner, descs, t.ntouched, t.r.pool, blob_hi, long_mode(),
      [&](uint64_t b, uint32_t nb, StreamDesc* d) {
        return launch_read_descs(t, b, nb, d, v.stream, v.num_cus);
      },
      [&](uint64_t b, uint32_t nb, const ChunkRec* rec, Counters* ctr) {
        return launch_read_compare(t, b, nb, rec, ctr, v.stream, v.num_cus);
      });
}

// One level of the pruned walk: the walk's, and a leaf node's run of followed children.
struct ReadLevel {
  WalkLevel w;
  DevBuf lfirst, lpre;
};

// The read owns every buffer here, its own index included (and hashes the touched blobs through
// the engine's second engine), so the last run's records, dedup result, tree, walk, restore and
// gc results stay as they are. Nothing of it outlives the call.
struct ReadWork {
  DevBuf in, in2, part, recs, seg, runs, touched, tpre, tlist, descs;
  RefTable tab;
  std::vector<ReadLevel> lv;
  PinBuf h_in, h_in2, h_out;
  Marks marks;                       // profile
  float ms[6] = {0, 0, 0, 0, 0, 0};  // profile: index + Roots, levels, placement, resolve +
                                     //   tiling, verify, scatter

  int readback(hipStream_t s, ReadHdr* h) {
    return read_header(h_out, in.p, s, h,
                       [](const ReadHdr& r) { return r.w.dd.error | r.r.dd.error; }, "read");
  }

  static uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? UINT64_MAX : a + b; }

  // The host checks its own arrays; the walk runs level by level as bsg_engine_walk's, with one
  // small readback per level. The sizes come back with the verdicts, and with them what every
  // range gets and where it lies; placement, resolve, tiling and (with the flag) the hash runs of
  // the touched blobs follow, and the scatter is launched only when every verdict is in. With
  // `ps` the table and the index are a bsg_pool's, read where they lie (bsg_pool_read).
  int run(const RunView& v, const uint8_t* d_pool, uint64_t pool_bytes, const bsg_pool_blob* blobs,
          uint64_t nblobs, const bsg_read_range* ranges, uint32_t nr, uint8_t* d_out,
          uint64_t out_cap, const uint64_t* out_off, int flags, int32_t* status, uint64_t* got,
          bsg_read_info* info, const PoolSrc* ps = nullptr) {
    const hipStream_t stream = v.stream;
    auto mark = [&](size_t i) { v.profile ? marks.record(i, stream) : void(); };
    auto elapsed = [&](size_t i, size_t j) { return v.profile ? marks.ms(i, j) : 0.f; };
    for (float& m : ms) m = 0.f;
    const bool verify = (flags & BSG_READ_VERIFY) != 0;
    if ((flags & ~BSG_READ_VERIFY) || nr > 65535) return BSG_EINVAL;
    if ((!d_pool && pool_bytes) || (!blobs && !ps && nblobs) || (!ranges && nr) ||
        (!out_off && nr) || (!d_out && out_cap))
      return BSG_EINVAL;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_pool), p1 = p0 + pool_bytes;
    const uintptr_t ob = reinterpret_cast<uintptr_t>(d_out);
    if (p1 < p0 || ob + out_cap < ob || ob % 16 != 0) return BSG_EINVAL;
    for (uint32_t q = 0; q < nr; ++q) {
      if (out_off[q] % 16 != 0 || out_off[q] > out_cap) return BSG_EINVAL;
      // (a len of 2^63 or more can only be held to the stream's size, below)
      if (ranges[q].len < (1ull << 63) && ranges[q].len > out_cap - out_off[q]) return BSG_EINVAL;
    }
    uint64_t blob_hi = ps ? ps->used : 0;
    for (uint64_t k = 0; k < nblobs && !ps; ++k) {
      if (blobs[k].off > pool_bytes || blobs[k].len > pool_bytes - blobs[k].off) return BSG_EINVAL;
      blob_hi = std::max<uint64_t>(blob_hi, blobs[k].off + blobs[k].len);
    }
    if (ps && ps->used > pool_bytes) return BSG_EINVAL;

    // the input block: header | sizes | status (these three come back) | blobs (the call's own
    // table only) | Roots | windows
    auto pad16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t o_sizes = sizeof(ReadHdr);
    const uint64_t o_status = o_sizes + pad16(8ull * nr);
    const uint64_t o_blobs = o_status + pad16(4ull * nr);
    const uint64_t o_roots = o_blobs + (ps ? 0 : pad16(sizeof(PoolBlob) * nblobs));
    const uint64_t o_win = o_roots + pad16(32ull * nr);
    const uint64_t in_bytes = o_win + pad16(16ull * nr);
    MCHECK(h_in.ensure(in_bytes));
    MCHECK(h_out.ensure(std::max<uint64_t>(o_blobs + 16, 8ull * (nr + 1ull))));
    uint8_t* hin = h_in.as<uint8_t>();
    std::memset(hin, 0, o_blobs);
    {
      ReadHdr* h0 = reinterpret_cast<ReadHdr*>(hin);
      h0->r.missing = h0->r.mismatch = h0->r.bad_blob = ~0ull;
    }
    if (nblobs && !ps) std::memcpy(hin + o_blobs, blobs, sizeof(PoolBlob) * nblobs);
    uint64_t* hwin = reinterpret_cast<uint64_t*>(hin + o_win);
    for (uint32_t q = 0; q < nr; ++q) {
      std::memcpy(hin + o_roots + 32ull * q, ranges[q].root, 32);
      hwin[2 * q] = ranges[q].offset;
      hwin[2 * q + 1] = sat_add(ranges[q].offset, ranges[q].len);
    }

    lv.resize(kWalkMaxDepth + 2);
    MCHECK(in.ensure(in_bytes));
    if (!ps) MCHECK(tab.reserve(nblobs));
    MCHECK(touched.ensure(std::max<uint64_t>(nblobs, 1)));
    MCHECK(lv[0].w.items.ensure(sizeof(WalkItem) * nr));
    WalkArgs base{};
    base.pool = d_pool;
    base.pool_bytes = pool_bytes;
    base.blobs = ps ? ps->table : reinterpret_cast<const PoolBlob*>(in.as<uint8_t>() + o_blobs);
    base.nblobs = nblobs;
    base.roots = in.as<uint8_t>() + o_roots;
    base.ns = nr;
    base.tab = ps ? ps->index : tab.p();
    base.tab_mask = ps ? ps->mask : tab.mask();
    base.hdr = &in.as<ReadHdr>()->w;
    base.sizes = reinterpret_cast<uint64_t*>(in.as<uint8_t>() + o_sizes);
    base.status = reinterpret_cast<uint32_t*>(in.as<uint8_t>() + o_status);
    base.win = reinterpret_cast<const uint64_t*>(in.as<uint8_t>() + o_win);
    base.touched = touched.as<uint8_t>();
    auto level_args = [&](uint32_t L) {
      WalkArgs a = base;
      ReadLevel& l = lv[L];
      a.level = L;
      a.last = L == kWalkMaxDepth;
      a.n = l.w.n;
      a.items = l.w.items.as<WalkItem>();
      a.nodes = l.w.nodes.as<WalkNode>();
      a.call = l.w.call.as<uint64_t>();
      a.cnode = l.w.cnode.as<uint64_t>();
      a.prec = l.w.prec.as<uint64_t>();
      a.lfirst = l.lfirst.as<uint64_t>();
      a.lpre = l.lpre.as<uint64_t>();
      a.part = part.as<uint64_t>();
      return a;
    };

    int rc;
    mark(0);
    HCHECK(hipMemcpyAsync(in.p, hin, in_bytes, hipMemcpyHostToDevice, stream));
    if (nblobs) HCHECK(hipMemsetAsync(touched.p, 0, nblobs, stream));
    if (!ps) {
      HCHECK(tab.clear(stream));
      HCHECK(dbg("launch_ref_index", stream,
                 launch_ref_index(base.blobs, nblobs, base.tab, base.tab_mask, &base.hdr->dd,
                                  stream, v.num_cus)));
    }
    {
      WalkArgs a = base;
      a.items = lv[0].w.items.as<WalkItem>();
      HCHECK(dbg("launch_walk_roots", stream, launch_walk_roots(a, stream, v.num_cus)));
    }
    mark(1);

    // level by level, as the walk: count, the two prefixes, the level's totals back, emit
    ReadHdr h{};
    uint32_t nlv = 0;
    uint64_t n = nr;
    for (uint32_t L = 0; L <= kWalkMaxDepth && n; ++L) {
      ReadLevel& l = lv[L];
      l.w.n = n;
      MCHECK(l.w.nodes.ensure(sizeof(WalkNode) * n));
      MCHECK(l.w.call.ensure(8 * (n + 1)));
      MCHECK(l.w.cnode.ensure(8 * (n + 1)));
      MCHECK(l.w.prec.ensure(8 * (n + 1)));
      MCHECK(l.lfirst.ensure(8 * n));
      MCHECK(l.lpre.ensure(8 * (n + 1)));
      MCHECK(part.ensure(8 * sum_parts(std::max(n, nblobs))));
      WalkArgs a = level_args(L);
      HCHECK(dbg("launch_walk_count", stream, launch_walk_count(a, stream, v.num_cus)));
      if ((rc = readback(stream, &h))) return rc;
      l.w.all = h.w.lvl_all[L];
      l.w.nodekids = h.w.lvl_nodes[L];
      if (l.w.nodekids > l.w.all) return BSG_EDEVICE;
      nlv = L + 1;
      n = a.last ? 0 : l.w.nodekids;
      MCHECK(lv[L + 1].w.items.ensure(sizeof(WalkItem) * n));
      a.nchild = l.w.all;
      a.next = lv[L + 1].w.items.as<WalkItem>();
      a.nnext = n;
      HCHECK(dbg("launch_walk_emit", stream, launch_walk_emit(a, stream, v.num_cus)));
    }
    mark(2);

    // the verdicts: header, sizes and status in one copy
    HCHECK(hipMemcpyAsync(h_out.p, in.p, o_blobs, hipMemcpyDeviceToHost, stream));
    HCHECK(stream_wait(stream));
    h = *h_out.as<ReadHdr>();
    if (h.w.dd.error) {
      std::fprintf(stderr, "bsgpu: read sanity check failed (code %llu)\n",
                   (unsigned long long)h.w.dd.error);
      return BSG_EDEVICE;
    }
    ms[0] = elapsed(0, 1);
    ms[1] = elapsed(1, 2);
    const uint64_t* hsizes = reinterpret_cast<const uint64_t*>(h_out.as<uint8_t>() + o_sizes);
    const uint32_t* hstat = reinterpret_cast<const uint32_t*>(h_out.as<uint8_t>() + o_status);

    // what every range gets, and where: the rules that need the sizes
    std::vector<uint64_t> want(nr);
    std::vector<std::pair<uint64_t, uint64_t>> spans;
    uint64_t total_bytes = 0, tiles = 0;
    for (uint32_t q = 0; q < nr; ++q) {
      const uint64_t size = hsizes[q], at = std::min(ranges[q].offset, size);
      want[q] = std::min(ranges[q].len, size - at);
      if (want[q] > out_cap - out_off[q]) return BSG_EINVAL;
      if (!want[q]) continue;
      const uintptr_t o0 = ob + out_off[q], o1 = o0 + want[q];
      if (pool_bytes && o0 < p1 && p0 < o1) return BSG_EINVAL;  // the output inside the pool
      spans.emplace_back(out_off[q], out_off[q] + want[q]);
      total_bytes += want[q];
      tiles += (want[q] + kRestoreTile - 1) / kRestoreTile;
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
      if (spans[k].first < spans[k - 1].second) return BSG_EINVAL;
    if (tiles > 0x7fffffffull) return BSG_EINVAL;

    uint64_t bad = UINT64_MAX;
    bool missing = false;
    for (uint32_t q = 0; q < nr; ++q) {
      const int32_t st = hstat[q] >= kWalkNotFound ? BSG_ENOTFOUND
                         : hstat[q] == kWalkCorrupt ? BSG_ECORRUPT : BSG_OK;
      if (status) status[q] = st;
      if (st != BSG_OK && bad == UINT64_MAX) bad = q;
      missing = missing || st == BSG_ENOTFOUND;
    }
    if (info) {
      info->bad_range = bad;
      info->nnodes = h.w.nnodes;
      info->depth = (uint32_t)h.w.depth;
    }
    if (missing) return BSG_ENOTFOUND;
    if (bad != UINT64_MAX) return BSG_ECORRUPT;

    // placement: a leaf node's run and the records below every node bottom-up, then top-down
    // every node's first record and the records themselves
    mark(3);
    for (uint32_t L = nlv; L-- > 0;) {
      WalkArgs a = level_args(L);
      if (L + 1 < nlv) {
        a.down_prec = lv[L + 1].w.prec.as<uint64_t>();
        a.down_n = lv[L + 1].w.n;
      }
      HCHECK(dbg("launch_read_nrec", stream, launch_read_nrec(a, stream, v.num_cus)));
    }
    uint64_t total = 0;
    if (nlv) {
      HCHECK(hipMemcpyAsync(h_out.p, lv[0].w.prec.as<uint64_t>() + nr, 8, hipMemcpyDeviceToHost,
                            stream));
      HCHECK(stream_wait(stream));
      total = *h_out.as<uint64_t>();
    }
    uint64_t leaf_kids = 0;
    for (uint32_t L = 0; L < nlv; ++L) leaf_kids += lv[L].w.all - lv[L].w.nodekids;
    if (total > leaf_kids) return BSG_EDEVICE;
    MCHECK(recs.ensure(sizeof(ChunkRec) * std::max<uint64_t>(total, 1)));
    for (uint32_t L = 0; L < nlv; ++L) {
      WalkArgs a = level_args(L);
      if (L) {
        a.up_nodes = lv[L - 1].w.nodes.as<WalkNode>();
        a.up_cnode = lv[L - 1].w.cnode.as<uint64_t>();
        a.up_n = lv[L - 1].w.n;
      }
      a.rec = recs.as<ChunkRec>();
      a.nrec = total;
      HCHECK(dbg("launch_read_place", stream,
                 launch_read_place(a, lv[L].w.all - lv[L].w.nodekids, stream, v.num_cus)));
    }
    mark(4);

    // the second block: out_off | what every range gets | the windows' starts | tile prefix
    const uint64_t o_got = pad16(8ull * nr), o_w0 = 2 * o_got, o_tpre = 3 * o_got;
    const uint64_t in2_bytes = o_tpre + pad16(8ull * (nr + 1ull));
    MCHECK(h_in2.ensure(in2_bytes));
    MCHECK(in2.ensure(in2_bytes));
    {
      uint8_t* h2 = h_in2.as<uint8_t>();
      uint64_t* tp = reinterpret_cast<uint64_t*>(h2 + o_tpre);
      uint64_t t = 0;
      for (uint32_t q = 0; q < nr; ++q) {
        reinterpret_cast<uint64_t*>(h2)[q] = out_off[q];
        reinterpret_cast<uint64_t*>(h2 + o_got)[q] = want[q];
        reinterpret_cast<uint64_t*>(h2 + o_w0)[q] = ranges[q].offset;
        tp[q] = t;
        t += (want[q] + kRestoreTile - 1) / kRestoreTile;
      }
      tp[nr] = t;
    }
    const uint64_t nr1 = nr ? nr : 1;
    MCHECK(seg.ensure(8 * std::max<uint64_t>(total, 1)));
    MCHECK(runs.ensure(16 * nr1));
    TouchArgs t{};
    RestoreArgs& a = t.r;
    a.pool = d_pool;
    a.pool_bytes = pool_bytes;
    a.blobs = base.blobs;
    a.nblobs = nblobs;
    a.rec = recs.as<ChunkRec>();
    a.nrec = total;
    a.out_off = in2.as<const uint64_t>();
    a.out_len = reinterpret_cast<const uint64_t*>(in2.as<uint8_t>() + o_got);
    a.win0 = reinterpret_cast<const uint64_t*>(in2.as<uint8_t>() + o_w0);
    a.tpre = reinterpret_cast<const uint64_t*>(in2.as<uint8_t>() + o_tpre);
    a.ns = nr;
    a.tab = base.tab;
    a.tab_mask = base.tab_mask;
    a.seg = seg.as<uint64_t>();
    a.sfirst = runs.as<uint64_t>();
    a.slast = runs.as<uint64_t>() + nr1;
    a.out = d_out;
    a.hdr = &in.as<ReadHdr>()->r;
    a.touched = touched.as<uint8_t>();
    HCHECK(hipMemcpyAsync(in2.p, h_in2.p, in2_bytes, hipMemcpyHostToDevice, stream));
    HCHECK(hipMemsetAsync(runs.p, 0xFF, 16 * nr1, stream));
    HCHECK(dbg("launch_read_resolve", stream, launch_read_resolve(a, stream, v.num_cus)));
    mark(5);

    // the touched blobs: their list and their layout, then the hash runs
    uint64_t ntouched = 0;
    if (verify && nblobs) {
      const uint64_t cap = std::min(nblobs, h.w.nnodes + total);
      MCHECK(tpre.ensure(8 * (nblobs + 1)));
      MCHECK(tlist.ensure(8 * std::max<uint64_t>(cap, 1)));
      t.tpre = tpre.as<uint64_t>();
      t.tlist = tlist.as<uint64_t>();
      t.ntouched = cap;
      t.verified = &in.as<ReadHdr>()->verified;
      t.part = part.as<uint64_t>();
      HCHECK(dbg("launch_read_touched", stream, launch_read_touched(t, stream, v.num_cus)));
      HCHECK(hipMemcpyAsync(h_out.as<uint8_t>() + sizeof(ReadHdr), tpre.as<uint64_t>() + nblobs, 8,
                            hipMemcpyDeviceToHost, stream));
    }
    if ((rc = readback(stream, &h))) return rc;
    ms[2] = elapsed(3, 4);
    ms[3] = elapsed(4, 5);
    if ((h.r.invalid & 3) || h.r.missing != ~0ull || h.r.mismatch != ~0ull) {
      std::fprintf(stderr, "bsgpu: read: a range's records do not cover it\n");
      return BSG_EDEVICE;
    }
    if (info) info->nleaves = total;
    if (verify && nblobs) {
      ntouched = *reinterpret_cast<const uint64_t*>(h_out.as<uint8_t>() + sizeof(ReadHdr));
      if (ntouched > t.ntouched) return BSG_EDEVICE;
      // the engine hash path's own rules (bsg_engine_hash), for the touched blobs
      if (h.r.invalid || (ntouched && p0 % 16 != 0)) return BSG_EINVAL;
      t.ntouched = ntouched;
      if ((rc = hash_touched(v, t, descs, blob_hi))) return rc;
      mark(6);
      if ((rc = readback(stream, &h))) return rc;
      ms[4] = elapsed(5, 6);
      if (info) {
        info->verified = h.verified;
        info->bad_blob = h.r.bad_blob;
      }
      if (h.r.bad_blob != ~0ull) return BSG_ECORRUPT;
    }
    if (v.in_flight) return BSG_ESTATE;

    mark(7);
    HCHECK(dbg("launch_restore_scatter", stream, launch_restore_scatter(a, tiles, stream)));
    mark(8);
    if ((rc = readback(stream, &h))) return rc;
    ms[5] = elapsed(7, 8);
    if (got) std::copy(want.begin(), want.end(), got);
    if (info) info->bytes = total_bytes;
    return BSG_OK;
  }
};

}  // namespace
