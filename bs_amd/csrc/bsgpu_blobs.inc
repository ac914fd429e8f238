// bsgpu_blobs.inc — store/mem's Put and Get by ref for a pool that lives in device memory
// (bsg_pool_put_blobs, bsg_pool_get): bs.PutMulti and bs.GetMulti for blobs that are not part of
// a split run. Included from bsgpu_kernels.hip after bsgpu_read.inc, inside namespace bsg.
// DESIGN §4.16.
//
// A put is bsg_engine_pool_put with the caller's blobs as its items: the hash runs give every
// blob's ref (k_bl_descs, k_bl_refs), launch_dedup, k_pool_plan, k_pool_append and k_pool_where run
// as they are over refs[] and the spans' lens, and the gather takes a blob's bytes from its span
// (k_pool_gather_blobs, the tile loop of k_pool_gather). A get probes every request in the pool's
// index (k_bl_probe), sums the found blobs' padded lens into the requests' places (launch_sum) and,
// once the host has held the total to the output's capacity, gathers by output tiles (k_bl_gather).
// With BSG_GET_VERIFY the touched-list passes of bsgpu_read.inc hash the found blobs in between.
//
// Every loop is bounded, every span, index and offset read from device memory is checked against a
// host-known bound before it forms an address, and a get writes nothing of the pool.

// ---- put: the hash runs ------------------------------------------------------------------------
// item i's span (an empty one, and the error flag, if it breaks the rules the host held it to)
__device__ __forceinline__ BlobSpan bl_span(const BlobPutArgs& a, uint64_t i) {
  BlobSpan sp = {0, 0};
  if (i < a.p.d.n) sp = a.span[i];
  if (i >= a.p.d.n || (sp.off & 15) || sp.len >= (1ull << 40) || sp.off > a.src_bytes ||
      sp.len > a.src_bytes - sp.off) {
    dd_error(a.p.d.hdr, 1 << 16);
    sp.off = sp.len = 0;
  }
  return sp;
}

__global__ __launch_bounds__(256) void k_bl_descs(BlobPutArgs a, uint64_t b0, uint32_t n,
                                                  StreamDesc* d) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    const BlobSpan sp = bl_span(a, b0 + b);
    StreamDesc sd = {};
    sd.data_off = sp.off;
    sd.len = sp.len;
    sd.finalize = 1;
    sd.mid[0] = 0x6a09e667; sd.mid[1] = 0xbb67ae85; sd.mid[2] = 0x3c6ef372; sd.mid[3] = 0xa54ff53a;
    sd.mid[4] = 0x510e527f; sd.mid[5] = 0x9b05688c; sd.mid[6] = 0x1f83d9ab; sd.mid[7] = 0x5be0cd19;
    d[b] = sd;
  }
}

// the batch's refs into refs[], each record held to its blob's len
__global__ __launch_bounds__(256) void k_bl_refs(BlobPutArgs a, uint64_t b0, uint32_t n,
                                                 const ChunkRec* hashed, const Counters* hctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && (hctr->error || hctr->overflow))
    dd_error(a.p.d.hdr, (1 << 17) | (hctr->error << 20));
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
    const uint64_t i = b0 + b;
    if (i >= a.p.d.n || hashed[b].len != a.span[i].len) {
      dd_error(a.p.d.hdr, 1 << 18);
      continue;
    }
    const uint64_t* r = reinterpret_cast<const uint64_t*>(hashed[b].ref);
    uint64_t* o = reinterpret_cast<uint64_t*>(a.refs + 32 * i);
    for (int w = 0; w < 4; ++w) o[w] = r[w];
  }
}

// ---- put: the new blobs' bytes -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pool_gather_blobs(BlobPutArgs a) {
  pool_gather_tiles(a.p, [&a](uint64_t u, uint64_t len) -> const uint8_t* {
    const BlobSpan sp = a.span[u];  // (u < d.n: the tile loop's check)
    if (sp.len == len && sp.off <= a.src_bytes && len <= a.src_bytes - sp.off)
      return a.src + sp.off;
    dd_error(a.p.d.hdr, 1 << 12);
    return nullptr;
  });
}

// ---- get: probe and places -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bl_probe(GetArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t found = 0, bytes = 0;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.n; q += stride) {
    const uint64_t f = pool_lookup(a.table, a.nblobs, a.index, a.index_mask,
                                   reinterpret_cast<const uint64_t*>(a.refs + 32 * q),
                                   &a.hdr->r.dd);
    a.idx[q] = f;  // (kDedupEmpty: the pool lacks the ref)
    if (f == kDedupEmpty) continue;
    ++found;
    bytes += a.table[f].len;
    if (a.touched) a.touched[f] = 1;
  }
  mg_add(&a.hdr->found, found);
  mg_add(&a.hdr->bytes, bytes);
}

struct BvLen16 {  // what request q takes of the output
  __device__ uint64_t operator()(const GetArgs& a, uint64_t q) const {
    const uint64_t f = a.idx[q];
    return f < a.nblobs ? align16(a.table[f].len) : 0;
  }
};

// ---- get: the found blobs' bytes -------------------------------------------------------------------
// Partitioned by output tiles of kPoolTile bytes, as k_pool_gather. Segment q is request q: its
// blob's bytes at out_off[q], then the zero bytes (at most 15) up to out_off[q + 1]; a missing ref
// and an empty blob have no bytes, and seg_find steps over them. A pool's blobs start at multiples
// of 16 and so does every segment, so a whole vector is one aligned load.
__global__ __launch_bounds__(256) void k_bl_gather(GetArgs a) {
  const uint64_t t0 = (uint64_t)blockIdx.x * kPoolTile;
  if (t0 >= a.total || !a.n) return;
  const uint64_t t1 = min(t0 + (uint64_t)kPoolTile, a.total);
  const auto off = [&a](uint64_t q) { return a.out_off[q]; };
  __shared__ uint64_t seg[2];
  if (threadIdx.x == 0) {
    seg[0] = seg_find(0, a.n, t0, off);
    seg[1] = seg_find(seg[0], a.n, t1 - 1, off);
  }
  __syncthreads();
  const uint64_t q1 = seg[1];
  uint64_t q = seg[0];
  DedupHdr* eh = &a.hdr->r.dd;
  gather_tile<false>(a.out, t0, t1, a.total, [&](uint64_t pos, GatherSeg* g) {
    q = seg_find(q, q1 + 1, pos, off);
    const uint64_t o = a.out_off[q], nx = a.out_off[q + 1], f = a.idx[q];
    g->src = nullptr;
    if (pos < o || pos >= nx || nx > a.total || f >= a.nblobs) {
      dd_error(eh, 1 << 19);
      return false;
    }
    const uint64_t boff = a.table[f].off, len = a.table[f].len;
    if (align16(len) != nx - o || (boff & 15) || boff > a.pool_bytes || len > a.pool_bytes - boff) {
      dd_error(eh, 1 << 19);
      return false;
    }
    if (pos - o < len) {
      g->src = a.pool + boff;
      g->b0 = o;
      g->b1 = o + len;
    } else {
      g->src = a.hdr->zero;
      g->b0 = o + len;
      g->b1 = nx;
    }
    return true;
  });
}

// ---- launchers -----------------------------------------------------------------------------------
hipError_t launch_blob_descs(const BlobPutArgs& a, uint64_t b0, uint32_t n, StreamDesc* d,
                             hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_bl_descs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, b0, n, d);
  return hipGetLastError();
}

hipError_t launch_blob_refs(const BlobPutArgs& a, uint64_t b0, uint32_t n, const ChunkRec* hashed,
                            const Counters* hctr, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_bl_refs, dim3(engine_grid(n, num_cus)), dim3(256), 0, s, a, b0, n, hashed,
                     hctr);
  return hipGetLastError();
}

hipError_t launch_pool_gather_blobs(const BlobPutArgs& a, hipStream_t s) {
  if (!a.p.total16) return hipSuccess;
  const uint64_t tiles = (a.p.total16 + kPoolTile - 1) / kPoolTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pool_gather_blobs, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

// a.n >= 1; idx, out_off[0 .. n] and the header's counts
hipError_t launch_get_probe(const GetArgs& a, hipStream_t s, int num_cus) {
  hipLaunchKernelGGL(k_bl_probe, dim3(engine_grid(a.n, num_cus)), dim3(256), 0, s, a);
  return launch_sum<BvLen16>(a, a.n, a.out_off, s);
}

hipError_t launch_get_gather(const GetArgs& a, hipStream_t s) {
  if (!a.total) return hipSuccess;
  const uint64_t tiles = (a.total + kPoolTile - 1) / kPoolTile;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bl_gather, dim3((uint32_t)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}
