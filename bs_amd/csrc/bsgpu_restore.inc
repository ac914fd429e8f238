// bsgpu_restore.inc — split.Reader for many streams at once, on the device (bsg_engine_restore):
// the inverse of bsg_engine_dedup + bsg_engine_pack_unique. A pool holds every distinct blob
// once; records (stream, offset, len, ref) say which blob lies where; the streams are written
// out in place. Included from bsgpu_kernels.hip, inside namespace bsg. From
// bsgpu_engine_common.inc it takes the pool's index (launch_ref_index, pool_lookup), ref_eq,
// seg_find and, for k_rs_scatter, gather_tile. DESIGN §4.9.
//
// Nothing is written to the output before every check has passed: index, resolve, the tiling
// check and (optionally) the pool's SHA-256 verification only fill the call's own buffers and
// lower the verdict words of RestoreHdr; the host reads the header and launches the scatter
// only if all is well. Every probe and search is bounded, and every index or offset read from
// device memory is checked against its range before it forms an address.

__device__ __forceinline__ void rs_error(RestoreHdr* h, uint64_t code) { dd_error(&h->dd, code); }

__device__ __forceinline__ void rs_lower(uint64_t* w, uint64_t v) {
  atomicMin(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
}

// ---- resolve: record i -> its blob's pool offset, or the smallest failing record ---------------
__global__ __launch_bounds__(256) void k_rs_resolve(RestoreArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrec; i += stride) {
    const uint64_t f = pool_lookup(a.blobs, a.nblobs, a.tab, a.tab_mask,
                                   reinterpret_cast<const uint64_t*>(a.rec[i].ref), &a.hdr->dd);
    uint64_t so = 0;
    if (f == kDedupEmpty) {
      rs_lower(&a.hdr->missing, i);
    } else if (a.blobs[f].len != a.rec[i].len) {
      rs_lower(&a.hdr->mismatch, i);
    } else {
      so = a.blobs[f].off;
      if (so > a.pool_bytes || a.rec[i].len > a.pool_bytes - so) {  // (the host checked the blobs)
        rs_error(a.hdr, 4);
        so = 0;
      }
    }
    a.seg[i] = so;
  }
}

// ---- tiling: stream-major, ascending, every stream covered exactly -----------------------------
// Pairwise over neighbours: streams never descend, a stream's records follow each other without
// gap or overlap, a stream's first record starts at 0. Where that holds every stream has one run
// of records, so its first and last index are each written once.
__global__ __launch_bounds__(256) void k_rs_check(RestoreArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrec; i += stride) {
    const uint64_t off = a.rec[i].offset, len = a.rec[i].len;
    const uint32_t s = a.rec[i].stream;
    bool bad = s >= a.ns || len == 0;
    if (!bad) {
      const uint64_t slen = a.out_len[s];
      bad = off > slen || len > slen - off;
    }
    bool first = i == 0;
    if (i) {
      const uint32_t ps = a.rec[i - 1].stream;
      const uint64_t pend = a.rec[i - 1].offset + a.rec[i - 1].len;
      if (ps > s) bad = true;
      else if (ps == s) bad = bad || pend != off;
      else first = true;
      if (ps != s && ps < a.ns) a.slast[ps] = i - 1;
    }
    if (first) {
      bad = bad || off != 0;
      if (s < a.ns) a.sfirst[s] = i;
    }
    if (i + 1 == a.nrec && s < a.ns) a.slast[s] = i;
    if (bad) atomicOr(reinterpret_cast<unsigned long long*>(&a.hdr->invalid), 1ull);
  }
}

__global__ __launch_bounds__(256) void k_rs_streams(RestoreArgs a) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.ns; s += gridDim.x * blockDim.x) {
    const uint64_t f = a.sfirst[s], l = a.slast[s], slen = a.out_len[s];
    bool bad;
    if (slen == 0) {
      bad = f != kDedupEmpty || l != kDedupEmpty;
    } else {
      bad = f >= a.nrec || l >= a.nrec || f > l;
      if (!bad)
        bad = a.rec[f].stream != s || a.rec[l].stream != s || a.rec[f].offset != 0 ||
              a.rec[l].offset + a.rec[l].len != slen;
    }
    if (bad) atomicOr(reinterpret_cast<unsigned long long*>(&a.hdr->invalid), 2ull);
  }
}

// ---- verify: the pool's blobs as the descriptors of a hash run, its records against the refs ---
// blob k as a hash run's descriptor (empty, and the error flag, if it breaks the hash path's rules)
__device__ __forceinline__ StreamDesc rs_blob_desc(const RestoreArgs& a, uint64_t k) {
  uint64_t off = a.blobs[k].off, len = a.blobs[k].len;
  if ((off & 15) || off > a.pool_bytes || len > a.pool_bytes - off || len >= (1ull << 40)) {
    rs_error(a.hdr, 8);
    off = 0;
    len = 0;
  }
  StreamDesc sd = {};
  sd.data_off = off;
  sd.len = len;
  sd.finalize = 1;
  sd.mid[0] = 0x6a09e667; sd.mid[1] = 0xbb67ae85; sd.mid[2] = 0x3c6ef372; sd.mid[3] = 0xa54ff53a;
  sd.mid[4] = 0x510e527f; sd.mid[5] = 0x9b05688c; sd.mid[6] = 0x1f83d9ab; sd.mid[7] = 0x5be0cd19;
  return sd;
}

__global__ __launch_bounds__(256) void k_rs_descs(RestoreArgs a, uint64_t b0, uint32_t n,
                                                  StreamDesc* d) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x)
    d[b] = rs_blob_desc(a, b0 + b);
}

__global__ __launch_bounds__(256) void k_rs_compare(RestoreArgs a, uint64_t b0, uint32_t n,
                                                    const ChunkRec* hashed, const Counters* hctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && (hctr->error || hctr->overflow))
    rs_error(a.hdr, 16 | (hctr->error << 16));
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    const PoolBlob* pb = a.blobs + b0 + b;
    if (hashed[b].len != pb->len) rs_error(a.hdr, 32);
    if (!ref_eq(reinterpret_cast<const uint64_t*>(hashed[b].ref),
                reinterpret_cast<const uint64_t*>(pb->ref)))
      rs_lower(&a.hdr->bad_blob, b0 + b);
  }
}

// ---- scatter -----------------------------------------------------------------------------------
// Partitioned by output tiles of kRestoreTile bytes per stream. A workgroup finds its stream and
// tile in the tile prefix and its first and last record by offset. A segment is a record: its
// blob's bytes in the pool, its bytes of the stream (out + out_off[s] is 16-byte aligned);
// gather_tile does the rest.
struct RsOffset {  // seg_find's key: a record's offset in its stream
  const ChunkRec* rec;
  __device__ uint64_t operator()(uint64_t k) const { return rec[k].offset; }
};

// the segment of stream s (slen bytes) that holds byte `pos`, among records [*k, k1]. With a
// window (a.win0) pos and the segment are output positions: output byte p is stream byte w0 + p,
// a record that starts before the window gives its bytes from w0 on, one that ends after it its
// bytes up to the window's end, and no byte outside a blob is read.
__device__ __forceinline__ bool rs_locate(const RestoreArgs& a, uint32_t s, uint64_t slen,
                                          uint64_t* k, uint64_t k1, uint64_t pos, GatherSeg* g) {
  const uint64_t w0 = a.win0 ? a.win0[s] : 0;
  const uint64_t sp = w0 + pos;  // (the tiling check: the window lies inside the records)
  *k = seg_find(*k, k1 + 1, sp, RsOffset{a.rec});
  const uint64_t off = a.rec[*k].offset, len = a.rec[*k].len, so = a.seg[*k];
  g->src = nullptr;
  bool bad = a.rec[*k].stream != s || sp < pos || sp < off || sp - off >= len ||
             so > a.pool_bytes || len > a.pool_bytes - so;
  if (!a.win0) bad = bad || off > slen || len > slen - off;
  else bad = bad || off + len < off || pos >= slen;
  if (bad) {
    rs_error(a.hdr, 256);
    return false;
  }
  if (!a.win0) {
    g->src = a.pool + so;
    g->b0 = off;
    g->b1 = off + len;
    return true;
  }
  const uint64_t skip = off < w0 ? w0 - off : 0;  // the record's bytes before the window
  g->src = a.pool + so + skip;
  g->b0 = off + skip - w0;
  g->b1 = min(off + len - w0, slen);
  return true;
}

__global__ __launch_bounds__(256) void k_rs_scatter(RestoreArgs a) {
  __shared__ uint64_t sh[6];
  if (threadIdx.x == 0) {
    const uint64_t b = blockIdx.x;
    const uint64_t s = seg_find(0, a.ns, b, [&a](uint64_t k) { return a.tpre[k]; });
    const uint64_t slen = a.out_len[s], r0 = a.sfirst[s], r1 = a.slast[s];
    const uint64_t t0 = a.tpre[s] <= b ? (b - a.tpre[s]) * kRestoreTile : ~0ull;
    const uint64_t w0 = a.win0 ? a.win0[s] : 0;  // (bsg_engine_read: the tile's stream bytes)
    sh[0] = 0;
    if (t0 >= slen || r0 > r1 || r1 >= a.nrec || w0 + slen < w0) {
      rs_error(a.hdr, 128);
    } else {
      const uint64_t t1 = min(t0 + (uint64_t)kRestoreTile, slen);
      sh[0] = 1;
      sh[1] = s;
      sh[2] = t0;
      sh[3] = t1;
      sh[4] = seg_find(r0, r1 + 1, w0 + t0, RsOffset{a.rec});
      sh[5] = seg_find(sh[4], r1 + 1, w0 + t1 - 1, RsOffset{a.rec});
    }
  }
  __syncthreads();
  if (!sh[0]) return;
  const uint32_t s = (uint32_t)sh[1];
  const uint64_t t0 = sh[2], t1 = sh[3], k1 = sh[5];
  const uint64_t slen = a.out_len[s], oo = a.out_off[s];
  if (oo & 15) {
    if (threadIdx.x == 0) rs_error(a.hdr, 64);
    return;
  }
  uint64_t k = sh[4];
  gather_tile<false>(a.out + oo, t0, t1, slen, [&](uint64_t pos, GatherSeg* g) {
    return rs_locate(a, s, slen, &k, k1, pos, g);
  });
}

// ---- launchers ---------------------------------------------------------------------------------
hipError_t launch_restore_resolve(const RestoreArgs& a, bool index, hipStream_t s, int num_cus) {
  if (index) {  // (false: a.tab is a bsg_pool's own index)
    const hipError_t e =
        launch_ref_index(a.blobs, a.nblobs, a.tab, a.tab_mask, &a.hdr->dd, s, num_cus);
    if (e != hipSuccess) return e;
  }
  if (a.nrec) {
    const uint32_t g = engine_grid(a.nrec, num_cus);
    hipLaunchKernelGGL(k_rs_resolve, dim3(g), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rs_check, dim3(g), dim3(256), 0, s, a);
  }
  if (a.ns)
    hipLaunchKernelGGL(k_rs_streams, dim3(engine_grid(a.ns, num_cus)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_restore_descs(const RestoreArgs& a, uint64_t b0, uint32_t n, StreamDesc* d,
                                hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_rs_descs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, b0, n, d);
  return hipGetLastError();
}

hipError_t launch_restore_compare(const RestoreArgs& a, uint64_t b0, uint32_t n,
                                  const ChunkRec* hashed, const Counters* hctr, hipStream_t s,
                                  int num_cus) {
  hipLaunchKernelGGL(k_rs_compare, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, b0, n,
                     hashed, hctr);
  return hipGetLastError();
}

// a.tpre[a.ns] tiles (host copy: `tiles`)
hipError_t launch_restore_scatter(const RestoreArgs& a, uint64_t tiles, hipStream_t s) {
  if (!tiles) return hipSuccess;
  if (tiles > 0x7fffffffull || !a.ns) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rs_scatter, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}
