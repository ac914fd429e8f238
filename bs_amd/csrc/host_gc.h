// host_gc.h — bsg_engine_gc_mark / bsg_engine_copy_gc / bsg_engine_gc_compact: a pool
// garbage-collected on the device from its Roots (included by host_engine.h).
#pragma once

namespace {

// The mark owns every buffer here, its own index included, so the last run's records, dedup
// result, tree, walk and restore buffers stay as they are. The result (live, the three prefixes
// and the blob table on the device, the totals on the host) lives until the next mark.
struct GcWork {
  DevBuf in, part, live, state, rblob, rstatus, rank, noff, noff16, mtab;
  RefTable tab;
  std::vector<WalkLevel> lv;  // (prec unused)
  PinBuf h_in, h_out;
  std::vector<PoolBlob> blobs;  // the marked pool's table (empty if it is a bsg_pool's: d_blobs)
  const uint8_t* d_pool = nullptr;
  const PoolBlob* d_blobs = nullptr;  // the table and the index the mark read: its own upload and
  uint64_t* d_tab = nullptr;          // `tab`, or a bsg_pool's
  uint64_t d_mask = 0;
  bool from_pool = false;
  uint64_t pool_bytes = 0, nblobs = 0;
  uint64_t nlive = 0, end = 0, end16 = 0;
  bool valid = false;
  Marks marks;              // profile
  float ms[3] = {0, 0, 0};  // profile: index + Roots, levels, offsets
  float compact_ms = 0;

  int readback(hipStream_t s, GcHdr* h) {
    return read_header(h_out, in.p, s, h, [](const GcHdr& g) { return g.w.dd.error; }, "gc");
  }

  GcArgs base_args() const {
    GcArgs a{};
    a.w.pool = d_pool;
    a.w.pool_bytes = pool_bytes;
    a.w.blobs = d_blobs;
    a.w.nblobs = nblobs;
    a.w.ns = 1;  // the count pass's one stream: its size and status go to the header's spare words
    a.w.tab = d_tab;
    a.w.tab_mask = d_mask;
    a.g = in.as<GcHdr>();
    a.w.hdr = &a.g->w;
    a.w.sizes = &a.g->size0;
    a.w.status = &a.g->status0;
    a.w.part = part.as<uint64_t>();
    a.live = live.as<uint8_t>();
    a.state = state.as<uint32_t>();
    a.rblob = rblob.as<uint64_t>();
    a.rstatus = rstatus.as<uint32_t>();
    a.rank = rank.as<uint64_t>();
    a.noff = noff.as<uint64_t>();
    a.noff16 = noff16.as<uint64_t>();
    a.part = part.as<uint64_t>();
    return a;
  }

  // The host checks its own arrays; every node is validated on the device, level by level, with
  // one small readback per level for the next frontier's size. Nothing is published before the
  // verdict is in. With `ps` the table and the index are a bsg_pool's, read where they lie: no
  // table is uploaded, no index built, and the pool's invariant stands for the loop over the blobs.
  int mark(const RunView& v, const uint8_t* pool, uint64_t pbytes, const bsg_pool_blob* tbl,
           uint64_t n_blobs, const uint8_t* roots, uint64_t nroots, int flags, int32_t* status,
           bsg_gc_info* info, const PoolSrc* ps = nullptr) {
    const hipStream_t stream = v.stream;
    auto stamp = [&](size_t i) { v.profile ? marks.record(i, stream) : void(); };
    valid = false;
    if ((flags & ~BSG_GC_MISSING_LEAVES) || nroots > 0xffffffffull) return BSG_EINVAL;
    if ((!pool && pbytes) || (!tbl && !ps && n_blobs) || (!roots && nroots)) return BSG_EINVAL;
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(pool);
    if (p0 + pbytes < p0) return BSG_EINVAL;
    for (uint64_t k = 0; k < n_blobs && !ps; ++k)
      if (tbl[k].off > pbytes || tbl[k].len > pbytes - tbl[k].off) return BSG_EINVAL;
    if (ps && ps->used > pbytes) return BSG_EINVAL;

    // the input block: header | blobs (the call's own table only) | Roots (the first comes back)
    auto pad16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t ob = sizeof(GcHdr);
    const uint64_t o_roots = ob + (ps ? 0 : pad16(sizeof(PoolBlob) * n_blobs));
    const uint64_t in_bytes = o_roots + pad16(32 * nroots);
    MCHECK(h_in.ensure(in_bytes));
    MCHECK(h_out.ensure(std::max<uint64_t>(sizeof(GcHdr) + 24, 4 * nroots)));
    uint8_t* hin = h_in.as<uint8_t>();
    GcHdr h{};
    h.bad_form = h.bad_miss = ~0ull;
    std::memcpy(hin, &h, sizeof h);
    if (n_blobs && !ps) std::memcpy(hin + ob, tbl, sizeof(PoolBlob) * n_blobs);
    if (nroots) std::memcpy(hin + o_roots, roots, 32 * nroots);

    lv.resize(kWalkMaxDepth + 2);
    MCHECK(in.ensure(in_bytes));
    if (!ps) MCHECK(tab.reserve(n_blobs));
    MCHECK(live.ensure(n_blobs));
    MCHECK(state.ensure(4 * n_blobs));
    MCHECK(rblob.ensure(8 * nroots));
    MCHECK(rstatus.ensure(4 * nroots));
    MCHECK(rank.ensure(8 * (n_blobs + 1)));
    MCHECK(noff.ensure(8 * (n_blobs + 1)));
    MCHECK(noff16.ensure(8 * (n_blobs + 1)));
    MCHECK(part.ensure(8 * sum_parts(std::max(n_blobs, nroots))));
    MCHECK(lv[0].items.ensure(sizeof(WalkItem) * nroots));
    d_pool = pool;
    pool_bytes = pbytes;
    nblobs = n_blobs;
    from_pool = ps != nullptr;
    d_blobs = ps ? ps->table : reinterpret_cast<const PoolBlob*>(in.as<uint8_t>() + ob);
    d_tab = ps ? ps->index : tab.p();
    d_mask = ps ? ps->mask : tab.mask();
    GcArgs base = base_args();
    base.roots = in.as<uint8_t>() + o_roots;
    base.nroots = nroots;
    base.forgive = (flags & BSG_GC_MISSING_LEAVES) != 0;
    auto level_args = [&](uint32_t L) {
      GcArgs a = base;
      WalkLevel& l = lv[L];
      a.w.level = L;
      a.w.last = L == kWalkMaxDepth;
      a.w.n = l.n;
      a.w.items = l.items.as<WalkItem>();
      a.w.nodes = l.nodes.as<WalkNode>();
      a.w.call = l.call.as<uint64_t>();
      a.w.cnode = l.cnode.as<uint64_t>();
      return a;
    };

    int rc;
    stamp(0);
    HCHECK(hipMemcpyAsync(in.p, hin, in_bytes, hipMemcpyHostToDevice, stream));
    if (!ps) HCHECK(tab.clear(stream));
    if (n_blobs) {
      HCHECK(hipMemsetAsync(live.p, 0, n_blobs, stream));
      HCHECK(hipMemsetAsync(state.p, 0, 4 * n_blobs, stream));
    }
    if (!ps)
      HCHECK(dbg("launch_ref_index", stream,
                 launch_ref_index(base.w.blobs, n_blobs, base.w.tab, base.w.tab_mask,
                                  &base.w.hdr->dd, stream, v.num_cus)));
    {
      GcArgs a = base;
      a.w.items = lv[0].items.as<WalkItem>();
      HCHECK(dbg("launch_gc_roots", stream, launch_gc_roots(a, stream, v.num_cus)));
    }
    stamp(1);

    // level by level: count, the two prefixes, the level's totals back, emit. A frontier is the
    // `nodes` entries of the level above (the Roots at level 0), never more.
    uint32_t nlv = 0;
    uint64_t n = nroots, leaf_kids = 0;
    for (uint32_t L = 0; L <= kWalkMaxDepth && n; ++L) {
      WalkLevel& l = lv[L];
      l.n = n;
      MCHECK(l.nodes.ensure(sizeof(WalkNode) * n));
      MCHECK(l.call.ensure(8 * (n + 1)));
      MCHECK(l.cnode.ensure(8 * (n + 1)));
      MCHECK(part.ensure(8 * sum_parts(std::max(n, std::max(n_blobs, nroots)))));
      base.w.part = base.part = part.as<uint64_t>();
      GcArgs a = level_args(L);
      HCHECK(dbg("launch_walk_count", stream, launch_walk_count(a.w, stream, v.num_cus)));
      if ((rc = readback(stream, &h))) return rc;
      l.all = h.w.lvl_all[L];
      l.nodekids = h.w.lvl_nodes[L];
      if (l.nodekids > l.all) return BSG_EDEVICE;
      leaf_kids += l.all - l.nodekids;
      nlv = L + 1;
      n = a.w.last ? 0 : l.nodekids;
      MCHECK(lv[L + 1].items.ensure(sizeof(WalkItem) * n));
      a.w.nchild = l.all;
      a.w.next = lv[L + 1].items.as<WalkItem>();
      a.w.nnext = n;
      HCHECK(dbg("launch_gc_emit", stream, launch_gc_emit(a, stream, v.num_cus)));
    }
    HCHECK(dbg("launch_gc_status", stream, launch_gc_status(base, stream, v.num_cus)));
    stamp(2);

    // the verdicts: every Root's status, then the header
    if (nroots)
      HCHECK(hipMemcpyAsync(h_out.p, rstatus.p, 4 * nroots, hipMemcpyDeviceToHost, stream));
    HCHECK(stream_wait(stream));
    uint64_t bad = UINT64_MAX;
    const uint32_t* hstat = h_out.as<uint32_t>();
    for (uint64_t r = 0; r < nroots; ++r) {
      const int32_t st = hstat[r] >= kWalkNotFound ? BSG_ENOTFOUND
                         : hstat[r] == kWalkCorrupt ? BSG_ECORRUPT : BSG_OK;
      if (status) status[r] = st;
      if (st != BSG_OK && bad == UINT64_MAX) bad = r;
    }
    if ((rc = readback(stream, &h))) return rc;
    ms[0] = v.profile ? marks.ms(0, 1) : 0.f;
    ms[1] = v.profile ? marks.ms(1, 2) : 0.f;
    ms[2] = 0.f;
    if (info) {
      info->bad_root = bad;
      info->bad_blob = h.bad_form != ~0ull ? h.bad_form : h.bad_miss;
      info->nnodes = h.w.nnodes;
      info->depth = (uint32_t)h.w.depth;
    }
    if (h.verdict >= kWalkNotFound) return BSG_ENOTFOUND;
    if (h.verdict == kWalkCorrupt) return BSG_ECORRUPT;
    if (bad != UINT64_MAX || h.bad_form != ~0ull || h.bad_miss != ~0ull) return BSG_EDEVICE;
    if (v.in_flight) return BSG_ESTATE;

    // forgiven misses: the `leaves` children of every level once more, into a table of their own
    stamp(3);
    if (h.leaf_miss) {
      const uint64_t slots = pow2_at_least(std::max<uint64_t>(64, 2 * leaf_kids));
      MCHECK(mtab.ensure(8 * slots));
      HCHECK(hipMemsetAsync(mtab.p, 0xFF, 8 * slots, stream));
      for (uint32_t L = 0; L < nlv; ++L) {
        GcArgs a = level_args(L);
        a.w.nchild = lv[L].all;
        a.mtab = mtab.as<uint64_t>();
        a.mmask = slots - 1;
        HCHECK(dbg("launch_gc_missing", stream, launch_gc_missing(a, stream, v.num_cus)));
      }
    }
    HCHECK(dbg("launch_gc_offsets", stream, launch_gc_offsets(base, stream, v.num_cus)));
    stamp(4);
    // the totals: the header, and the last word of each prefix
    uint64_t* tot = reinterpret_cast<uint64_t*>(h_out.as<uint8_t>() + sizeof(GcHdr));
    DevBuf* pre[3] = {&rank, &noff, &noff16};
    for (int i = 0; i < 3; ++i)
      HCHECK(hipMemcpyAsync(tot + i, pre[i]->as<uint64_t>() + n_blobs, 8, hipMemcpyDeviceToHost,
                            stream));
    if ((rc = readback(stream, &h))) return rc;
    ms[2] = v.profile ? marks.ms(3, 4) : 0.f;
    if (tot[0] > n_blobs || h.end > tot[1] || h.end16 > tot[2]) return BSG_EDEVICE;

    blobs.clear();
    if (!ps)
      blobs.assign(reinterpret_cast<const PoolBlob*>(tbl),
                   reinterpret_cast<const PoolBlob*>(tbl) + n_blobs);
    uint64_t all_bytes = ps ? ps->blob_bytes : 0;
    for (const PoolBlob& b : blobs) all_bytes += b.len;
    nlive = tot[0];
    end = h.end;
    end16 = h.end16;
    valid = true;
    if (info) {
      info->nlive = nlive;
      info->live_bytes = tot[1];
      info->ndead = n_blobs - nlive;
      info->dead_bytes = all_bytes - tot[1];
      info->missing_leaves = h.missing_leaves;
    }
    return BSG_OK;
  }

  // live[] and the live blobs' table in the variant `flags` names, to host memory
  int copy(uint8_t* out_live, uint64_t cap_live, bsg_pool_blob* table, uint64_t cap_table,
           int flags) {
    if (flags & ~BSG_GC_ALIGN16) return BSG_EINVAL;
    if (!valid) return BSG_ESTATE;
    if ((!out_live && !table) || !nblobs) return BSG_OK;
    std::vector<uint8_t> lv8(nblobs);
    HCHECK(hipMemcpy(lv8.data(), live.p, nblobs, hipMemcpyDeviceToHost));
    const uint64_t nl = std::min(cap_live, nblobs);
    if (out_live && nl) std::memcpy(out_live, lv8.data(), nl);
    if (!table || !cap_table) return BSG_OK;
    if (from_pool) {  // the marked entries, from the pool (they never change while it lives)
      blobs.resize(nblobs);
      HCHECK(hipMemcpy(blobs.data(), d_blobs, sizeof(PoolBlob) * nblobs, hipMemcpyDeviceToHost));
      from_pool = false;
    }
    std::vector<uint64_t> off(nblobs + 1);
    HCHECK(hipMemcpy(off.data(), (flags & BSG_GC_ALIGN16) ? noff16.p : noff.p, 8 * (nblobs + 1),
                     hipMemcpyDeviceToHost));
    uint64_t j = 0;
    for (uint64_t k = 0; k < nblobs && j < cap_table; ++k) {
      if (!lv8[k]) continue;
      table[j].off = off[k];
      table[j].len = blobs[k].len;
      std::memcpy(table[j].ref, blobs[k].ref, 32);
      ++j;
    }
    return BSG_OK;
  }

  // The sweep. In-place compaction is out of scope: the output may not touch the pool.
  int compact(const RunView& v, const uint8_t* pool, uint64_t pbytes, uint8_t* d_out,
              uint64_t cap, int flags, uint64_t* out_bytes) {
    if (out_bytes) *out_bytes = 0;
    if (!valid || v.in_flight) return BSG_ESTATE;
    if (flags & ~BSG_GC_ALIGN16) return BSG_EINVAL;
    const uint64_t total = (flags & BSG_GC_ALIGN16) ? end16 : end;
    if (pool != d_pool || pbytes != pool_bytes || !d_out ||
        reinterpret_cast<uintptr_t>(d_out) % 16 != 0 || cap < total)
      return BSG_EINVAL;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + total;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_pool), s1 = s0 + pool_bytes;
    if (o1 < o0 || (total && o0 < s1 && s0 < o1)) return BSG_EINVAL;
    GcArgs a = base_args();
    a.coff = (flags & BSG_GC_ALIGN16) ? a.noff16 : a.noff;
    a.total = total;
    a.out = d_out;
    if (v.profile) marks.record(5, v.stream);
    HCHECK(dbg("launch_gc_compact", v.stream, launch_gc_compact(a, v.stream)));
    if (v.profile) marks.record(6, v.stream);
    GcHdr h;
    if (int rc = readback(v.stream, &h)) {
      valid = false;
      return rc;
    }
    compact_ms = v.profile ? marks.ms(5, 6) : 0.f;
    if (out_bytes) *out_bytes = total;
    return BSG_OK;
  }
};

}  // namespace
