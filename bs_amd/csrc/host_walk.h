// host_walk.h — bsg_engine_walk: split trees read on the device, from Roots to records (included
// by host_engine.h).
#pragma once

namespace {

// One level of the walk: its frontier, what the count pass learnt of it and its prefixes.
struct WalkLevel {
  DevBuf items, nodes, call, cnode, prec;
  uint64_t n = 0;         // frontier entries
  uint64_t all = 0;       // their children
  uint64_t nodekids = 0;  // ... of which `nodes` children
};

// The call owns every buffer here, so the last run's records, dedup result, tree and restore
// buffers stay as they are. The result (records on the device, sizes and counts on the host)
// lives until the next call.
struct WalkWork {
  DevBuf in, part, recs;
  RefTable tab;
  std::vector<WalkLevel> lv;
  PinBuf h_in, h_out;
  std::vector<uint64_t> sizes, counts;  // per stream, of the last successful walk
  uint32_t ns = 0;
  uint64_t nrecs = 0;
  bool valid = false;
  Marks marks;              // profile
  float ms[3] = {0, 0, 0};  // profile: index + Roots, levels, placement

  int readback(hipStream_t s, WalkHdr* h) {
    return read_header(h_out, in.p, s, h, [](const WalkHdr& w) { return w.dd.error; }, "walk");
  }

  // The host checks its own arrays (pointers, the blobs' bounds); every node is validated on the
  // device, level by level, with one small readback per level for the next frontier's size.
  // Nothing of the result is allocated before every stream's verdict is in. With `ps` the table
  // and the index are a bsg_pool's, read where they lie (bsg_pool_walk).
  int run(const RunView& v, const uint8_t* d_pool, uint64_t pool_bytes, const bsg_pool_blob* blobs,
          uint64_t nblobs, const uint8_t* roots, uint32_t nstreams, int flags, int32_t* status,
          bsg_walk_info* info, const PoolSrc* ps = nullptr) {
    const hipStream_t stream = v.stream;
    auto mark = [&](size_t i) { v.profile ? marks.record(i, stream) : void(); };
    valid = false;
    if (flags != 0 || nstreams > 65535) return BSG_EINVAL;
    if ((!d_pool && pool_bytes) || (!blobs && !ps && nblobs) || (!roots && nstreams))
      return BSG_EINVAL;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_pool);
    if (p0 + pool_bytes < p0) return BSG_EINVAL;
    for (uint64_t k = 0; k < nblobs && !ps; ++k)
      if (blobs[k].off > pool_bytes || blobs[k].len > pool_bytes - blobs[k].off) return BSG_EINVAL;
    if (ps && ps->used > pool_bytes) return BSG_EINVAL;

    // the input block: header | sizes | status | blobs (the call's own table only) | Roots (the
    // first three come back)
    auto pad16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t o_sizes = sizeof(WalkHdr);
    const uint64_t o_status = o_sizes + pad16(8ull * nstreams);
    const uint64_t o_blobs = o_status + pad16(4ull * nstreams);
    const uint64_t o_roots = o_blobs + (ps ? 0 : pad16(sizeof(PoolBlob) * nblobs));
    const uint64_t in_bytes = o_roots + pad16(32ull * nstreams);
    MCHECK(h_in.ensure(in_bytes));
    MCHECK(h_out.ensure(std::max<uint64_t>(o_blobs, 8ull * (nstreams + 1ull))));
    uint8_t* hin = h_in.as<uint8_t>();
    std::memset(hin, 0, o_blobs);
    if (nblobs && !ps) std::memcpy(hin + o_blobs, blobs, sizeof(PoolBlob) * nblobs);
    if (nstreams) std::memcpy(hin + o_roots, roots, 32ull * nstreams);

    lv.resize(kWalkMaxDepth + 2);
    MCHECK(in.ensure(in_bytes));
    if (!ps) MCHECK(tab.reserve(nblobs));
    MCHECK(lv[0].items.ensure(sizeof(WalkItem) * nstreams));
    WalkArgs base{};
    base.pool = d_pool;
    base.pool_bytes = pool_bytes;
    base.blobs = ps ? ps->table : reinterpret_cast<const PoolBlob*>(in.as<uint8_t>() + o_blobs);
    base.nblobs = nblobs;
    base.roots = in.as<uint8_t>() + o_roots;
    base.ns = nstreams;
    base.tab = ps ? ps->index : tab.p();
    base.tab_mask = ps ? ps->mask : tab.mask();
    base.hdr = in.as<WalkHdr>();
    base.sizes = reinterpret_cast<uint64_t*>(in.as<uint8_t>() + o_sizes);
    base.status = reinterpret_cast<uint32_t*>(in.as<uint8_t>() + o_status);
    auto level_args = [&](uint32_t L) {
      WalkArgs a = base;
      WalkLevel& l = lv[L];
      a.level = L;
      a.last = L == kWalkMaxDepth;
      a.n = l.n;
      a.items = l.items.as<WalkItem>();
      a.nodes = l.nodes.as<WalkNode>();
      a.call = l.call.as<uint64_t>();
      a.cnode = l.cnode.as<uint64_t>();
      a.prec = l.prec.as<uint64_t>();
      a.part = part.as<uint64_t>();
      return a;
    };

    int rc;
    mark(0);
    HCHECK(hipMemcpyAsync(in.p, hin, in_bytes, hipMemcpyHostToDevice, stream));
    if (!ps) {
      HCHECK(tab.clear(stream));
      HCHECK(dbg("launch_ref_index", stream,
                 launch_ref_index(base.blobs, nblobs, base.tab, base.tab_mask, &base.hdr->dd,
                                  stream, v.num_cus)));
    }
    {
      WalkArgs a = base;
      a.items = lv[0].items.as<WalkItem>();
      HCHECK(dbg("launch_walk_roots", stream, launch_walk_roots(a, stream, v.num_cus)));
    }
    mark(1);

    // level by level: count, the two prefixes, the level's totals back, emit
    WalkHdr h{};
    uint32_t nlv = 0;
    uint64_t n = nstreams;
    for (uint32_t L = 0; L <= kWalkMaxDepth && n; ++L) {
      WalkLevel& l = lv[L];
      l.n = n;
      MCHECK(l.nodes.ensure(sizeof(WalkNode) * n));
      MCHECK(l.call.ensure(8 * (n + 1)));
      MCHECK(l.cnode.ensure(8 * (n + 1)));
      MCHECK(l.prec.ensure(8 * (n + 1)));
      MCHECK(part.ensure(8 * sum_parts(n)));
      WalkArgs a = level_args(L);
      HCHECK(dbg("launch_walk_count", stream, launch_walk_count(a, stream, v.num_cus)));
      if ((rc = readback(stream, &h))) return rc;
      l.all = h.lvl_all[L];
      l.nodekids = h.lvl_nodes[L];
      if (l.nodekids > l.all) return BSG_EDEVICE;
      nlv = L + 1;
      n = a.last ? 0 : l.nodekids;
      MCHECK(lv[L + 1].items.ensure(sizeof(WalkItem) * n));
      a.nchild = l.all;
      a.next = lv[L + 1].items.as<WalkItem>();
      a.nnext = n;
      HCHECK(dbg("launch_walk_emit", stream, launch_walk_emit(a, stream, v.num_cus)));
    }
    mark(2);

    // the verdicts: header, sizes and status in one copy
    HCHECK(hipMemcpyAsync(h_out.p, in.p, o_blobs, hipMemcpyDeviceToHost, stream));
    HCHECK(stream_wait(stream));
    h = *h_out.as<WalkHdr>();
    if (h.dd.error) {
      std::fprintf(stderr, "bsgpu: walk sanity check failed (code %llu)\n",
                   (unsigned long long)h.dd.error);
      return BSG_EDEVICE;
    }
    ms[0] = v.profile ? marks.ms(0, 1) : 0.f;
    ms[1] = v.profile ? marks.ms(1, 2) : 0.f;
    ms[2] = 0.f;
    const uint64_t* hs0 = reinterpret_cast<const uint64_t*>(h_out.as<uint8_t>() + o_sizes);
    std::vector<uint64_t> hsizes(hs0, hs0 + nstreams);  // (h_out is read into again below)
    const uint32_t* hstat = reinterpret_cast<const uint32_t*>(h_out.as<uint8_t>() + o_status);
    uint64_t bad = UINT64_MAX, total_bytes = 0;
    bool missing = false;
    for (uint32_t s = 0; s < nstreams; ++s) {
      const int32_t st = hstat[s] >= kWalkNotFound ? BSG_ENOTFOUND
                         : hstat[s] == kWalkCorrupt ? BSG_ECORRUPT : BSG_OK;
      if (status) status[s] = st;
      if (st != BSG_OK && bad == UINT64_MAX) bad = s;
      missing = missing || st == BSG_ENOTFOUND;
      total_bytes += hsizes[s];
    }
    if (info) {
      info->bad_stream = bad;
      info->nnodes = h.nnodes;
      info->depth = (uint32_t)h.depth;
    }
    if (missing) return BSG_ENOTFOUND;
    if (bad != UINT64_MAX) return BSG_ECORRUPT;
    if (v.in_flight) return BSG_ESTATE;

    // placement: the records below every node bottom-up, then top-down every node's first
    // record and the records themselves
    mark(3);
    for (uint32_t L = nlv; L-- > 0;) {
      WalkArgs a = level_args(L);
      if (L + 1 < nlv) {
        a.down_prec = lv[L + 1].prec.as<uint64_t>();
        a.down_n = lv[L + 1].n;
      }
      HCHECK(dbg("launch_walk_nrec", stream, launch_walk_nrec(a, stream, v.num_cus)));
    }
    uint64_t total = 0;
    std::vector<uint64_t> cnt(nstreams);
    if (nlv) {
      HCHECK(hipMemcpyAsync(h_out.p, lv[0].prec.p, 8ull * (nstreams + 1ull),
                            hipMemcpyDeviceToHost, stream));
      HCHECK(stream_wait(stream));
      const uint64_t* pre = h_out.as<uint64_t>();
      for (uint32_t s = 0; s < nstreams; ++s) cnt[s] = pre[s + 1] - pre[s];
      total = pre[nstreams];
    }
    MCHECK(recs.ensure(sizeof(ChunkRec) * total));
    for (uint32_t L = 0; L < nlv; ++L) {
      WalkArgs a = level_args(L);
      if (L) {
        a.up_nodes = lv[L - 1].nodes.as<WalkNode>();
        a.up_cnode = lv[L - 1].cnode.as<uint64_t>();
        a.up_n = lv[L - 1].n;
      }
      a.nchild = lv[L].all - lv[L].nodekids;
      a.rec = recs.as<ChunkRec>();
      a.nrec = total;
      HCHECK(dbg("launch_walk_place", stream, launch_walk_place(a, stream, v.num_cus)));
    }
    mark(4);
    if ((rc = readback(stream, &h))) return rc;
    ms[2] = v.profile ? marks.ms(3, 4) : 0.f;

    sizes = std::move(hsizes);
    counts = std::move(cnt);
    ns = nstreams;
    nrecs = total;
    valid = true;
    if (info) {
      info->nrecs = total;
      info->bytes = total_bytes;
    }
    return BSG_OK;
  }
};

}  // namespace
