// host_tree.h — bsg_engine_trees: split.Writer's tree per stream of the last finished split run
// (included by host_engine.h).
#pragma once

namespace {

// The sizes of one bsg_engine_trees call: the run's own (known when it finished), then the node
// count and height bound from the counting pass, then the arena size from the layout passes.
struct TreePlan {
  uint32_t ns = 0;       // streams of the run
  uint64_t M = 0;        // its records
  uint32_t fanout = 8;
  uint64_t nn = 0;       // listed nodes of all streams
  uint32_t H = 1;        // heights of the tallest tree
  uint64_t arena = 0;    // blob bytes (16-byte aligned blobs), without the read slack
};

// The tree work owns every buffer here; its node blobs are hashed by the engine's second engine
// (it shares nothing with the run's buffers, so the records stay).
struct TreeWork {
  DevBuf hdr, cstart, rmax, kcnt, tmp, close, shbase, meta, pc, pn, aoff, part, descs, arena,
      nodes, roots, ncount;
  PinBuf h_hdr;
  TreePlan plan;        // the last result's sizes
  bool valid = false;   // set by run(), cleared by the next one that fails
  Marks marks;          // profile: start, layout done, per height emit / hash done, end
  float ms[4] = {0, 0, 0, 0};  // profile: counting + layout, emit, hash, whole call

  bool current(bool run_done) const { return valid && run_done; }  // (a new run clears run_done)

  TreeArgs args(const RunView& v, const TreePlan& tp) const {
    TreeArgs a{};
    a.rec = v.rec;
    a.M = tp.M;
    a.scount = v.scount;
    a.ns = tp.ns;
    a.fanout = tp.fanout;
    a.H = tp.H;
    a.nn = tp.nn;
    a.arena_bytes = tp.arena;
    a.hdr = hdr.as<TreeHdr>();
    a.cstart = cstart.as<uint64_t>();
    a.rmax = rmax.as<uint32_t>();
    a.kcnt = kcnt.as<uint8_t>();
    a.tmp = tmp.as<uint64_t>();
    a.close = close.as<uint64_t>();
    a.shbase = shbase.as<uint64_t>();
    a.meta = meta.as<TreeNodeMeta>();
    a.pc = pc.as<uint64_t>();
    a.pn = pn.as<uint64_t>();
    a.aoff = aoff.as<uint64_t>();
    a.part = part.as<uint64_t>();
    a.arena = arena.as<uint8_t>();
    a.nodes = nodes.as<TreeNode>();
    a.roots = roots.as<uint8_t>();
    a.ncount = ncount.as<uint64_t>();
    return a;
  }

  int readback(hipStream_t s, TreeHdr* h) {
    return read_header(h_hdr, hdr.p, s, h, [](const TreeHdr& t) { return t.error; }, "tree");
  }

  int run(const RunView& v) {
    if (!v.usable) return BSG_ESTATE;
    int rc;
    valid = false;
    const hipStream_t stream = v.stream;
    TreePlan tp;
    tp.ns = v.ns;
    tp.M = v.nrec;
    tp.fanout = v.fanout ? v.fanout : 8;
    const uint64_t nn1 = tp.ns ? tp.ns : 1, m1 = tp.M ? tp.M : 1;
    const bool prof = v.profile != 0;
    size_t nev = 0;

    // counting: chunk ranges, Root heights, node total
    HCHECK(hdr.ensure(sizeof(TreeHdr)));
    HCHECK(h_hdr.ensure(sizeof(TreeHdr)));
    HCHECK(cstart.ensure(8 * (nn1 + 1)));
    HCHECK(rmax.ensure(4 * nn1));
    HCHECK(kcnt.ensure(m1));
    HCHECK(tmp.ensure(8 * (m1 + 1)));
    HCHECK(pc.ensure(8 * (m1 + 1)));
    HCHECK(part.ensure(8 * sum_parts(std::max<uint64_t>(m1, nn1))));
    HCHECK(roots.ensure(32 * nn1));
    HCHECK(ncount.ensure(8 * nn1));
    if (prof) marks.record(nev++, stream);
    HCHECK(hipMemsetAsync(hdr.p, 0, sizeof(TreeHdr), stream));
    HCHECK(hipMemsetAsync(rmax.p, 0, 4 * nn1, stream));
    HCHECK(dbg("launch_tree_count", stream, launch_tree_count(args(v, tp), stream, v.num_cus)));
    TreeHdr h;
    if ((rc = readback(stream, &h))) return rc;
    tp.nn = h.nnodes;
    tp.H = (uint32_t)h.max_r + 1;
    if (tp.H > kTreeMaxHeights) return BSG_EDEVICE;

    if (tp.nn) {
      // layout: every node's children, listed place, blob length and arena offset
      HCHECK(close.ensure(8 * tp.nn));
      HCHECK(shbase.ensure(8 * ((uint64_t)tp.ns * tp.H + 1)));
      HCHECK(meta.ensure(sizeof(TreeNodeMeta) * tp.nn));
      HCHECK(pn.ensure(8 * (tp.nn + 1)));
      HCHECK(aoff.ensure(8 * (tp.nn + 1)));
      HCHECK(nodes.ensure(sizeof(TreeNode) * tp.nn));
      HCHECK(part.ensure(8 * sum_parts(std::max<uint64_t>(
                                 std::max<uint64_t>(m1, tp.nn), (uint64_t)tp.ns * tp.H))));
      HCHECK(dbg("launch_tree_layout", stream, launch_tree_layout(args(v, tp), stream, v.num_cus)));
      if ((rc = readback(stream, &h))) return rc;
      if (h.hoff[tp.H] != tp.nn) return BSG_EDEVICE;
      tp.arena = h.arena_bytes;
      HCHECK(arena.ensure(tp.arena + kReadSlack));
      HCHECK(hipMemsetAsync(arena.p, 0, tp.arena + kReadSlack, stream));
      if (prof) marks.record(nev++, stream);
      if ((rc = need_hasher(v.owner))) return rc;
      // height by height: emit the blobs, hash them, refs into the listed records (where the
      // next height's emit reads them)
      TreeArgs ta = args(v, tp);
      for (ta.h = 0; ta.h < tp.H; ++ta.h) {
        const uint64_t u0 = h.hoff[ta.h], n = h.hoff[ta.h + 1] - u0;
        const uint64_t children = ta.h ? u0 - h.hoff[ta.h - 1] : tp.M;
        HCHECK(dbg("launch_tree_emit", stream, launch_tree_emit(ta, children, stream, v.num_cus)));
        if (prof) marks.record(nev++, stream);
        rc = hash_batches(
            v.owner, descs, n, arena.as<uint8_t>(), tp.arena,
            n <= kTreeWaveNodes ? 2 : long_mode(),
            [&](uint64_t b, uint32_t nb, StreamDesc* d) {
              return launch_tree_descs(ta, u0 + b, nb, d, stream, v.num_cus);
            },
            [&](uint64_t b, uint32_t nb, const ChunkRec* rec, Counters* ctr) {
              return launch_tree_refs(ta, u0 + b, nb, rec, ctr, stream, v.num_cus);
            });
        if (rc) return rc;
        if (prof) marks.record(nev++, stream);
      }
    }
    HCHECK(dbg("launch_tree_roots", stream, launch_tree_roots(args(v, tp), stream, v.num_cus)));
    if (prof) marks.record(nev++, stream);
    if ((rc = readback(stream, &h))) return rc;
    if (prof) {
      ms[0] = ms[1] = ms[2] = 0.f;
      if (tp.nn) {
        ms[0] = marks.ms(0, 1);
        for (uint32_t k = 0; k < tp.H; ++k) {
          ms[1] += marks.ms(1 + 2 * k, 2 + 2 * k);
          ms[2] += marks.ms(2 + 2 * k, 3 + 2 * k);
        }
      }
      ms[3] = marks.ms(0, nev - 1);
    }
    plan = tp;
    valid = true;
    return BSG_OK;
  }
};

}  // namespace
