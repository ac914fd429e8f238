"""Engine and hasher results on sparse, reordered and aliased layouts (tests/layouts.py).

include/bsgpu.h lets the caller choose where the bytes lie: a base plus arbitrary off[i], len[i].
Every comparison here is per stream, on the stream's own bytes, against oracle.split,
oracle.writer_root or hashlib; the bytes between and after the streams are poisoned 0x00, 0xFF
and random, and all three must give the oracle's answer. Parts:
  a. Engine.run / Engine.hash on the small layouts, also from allocation + 4096 and + 16;
  b. the host batch and the hashers on host layouts, byte-unaligned;
  c. the hashers with a device base (bsg_hasher::sum's device branch), at every start residue;
  d. k_sha's address regions on sparse layouts of one ~4 GiB allocation;
  e. refusals: what engine_batch and bsg_hasher::sum return BSG_EINVAL for, before any launch.
"""
import hashlib

import numpy as np
import pytest

import layouts as LY
from bs_amd.synth import splitmix_array

pytestmark = pytest.mark.gpu

PARAMS = [(8, 64), (12, 256)]
EINVAL = -22
_WANT = {}


def _want(oracle, table, seed, n, bits, mn):
    """(chunks, Root) of the stream splitmix_array(seed, n): computed once, shared, read-only."""
    key = (seed, n, bits, mn)
    if key not in _WANT:
        d = splitmix_array(seed, n)
        ch = oracle.split(table, d, bits=bits, min_size=mn)
        ch.setflags(write=False)
        root, _ = oracle.writer_root(table, d, bits=bits, min_size=mn, fanout=8)
        _WANT[key] = (ch, root)
    return _WANT[key]


def _check_records(recs, counts, streams, oracle, table, bits, mn):
    assert len(counts) == len(streams)
    k = 0
    for s, (o, n, seed) in enumerate(streams):
        want, _ = _want(oracle, table, seed, n, bits, mn)
        c = int(counts[s])
        got = recs[k:k + c]
        k += c
        assert c == len(want), (s, o, n)
        assert (got["stream"] == s).all(), (s, o, n)
        for f in ("offset", "len", "level", "ref"):
            assert (got[f] == want[f]).all(), (s, o, n, f)
        assert n == 0 or int(got["len"].sum()) == n
    assert k == len(recs)


def _check_run(eng, streams, oracle, table, bits, mn):
    """Records, counts, the stream field and the Roots of a finished Engine.run."""
    assert eng.nchunks == sum(len(_want(oracle, table, sd, n, bits, mn)[0])
                              for _, n, sd in streams)
    _check_records(eng.chunks(), eng.counts(), streams, oracle, table, bits, mn)
    roots = eng.trees()[0]
    for s, (o, n, seed) in enumerate(streams):
        assert roots[s].tobytes() == _want(oracle, table, seed, n, bits, mn)[1], (s, o, n)


def _sha(seed, n):
    return hashlib.sha256(splitmix_array(seed, n).tobytes()).digest()


def _check_hash(eng, streams):
    """Record i of a finished Engine.hash: blob i's ref, offset 0, len[i]."""
    recs = eng.chunks()
    assert len(recs) == len(streams)
    for i, (o, n, seed) in enumerate(streams):
        assert recs[i]["ref"].tobytes() == _sha(seed, n), (i, o, n)
        assert int(recs[i]["len"]) == n and int(recs[i]["offset"]) == 0


def _split_cols(streams):
    return [o for o, _, _ in streams], [n for _, n, _ in streams]


# ---- a. engine run and hash on the small layouts ---------------------------------------------
@pytest.mark.parametrize("bits,mn", PARAMS)
@pytest.mark.parametrize("name", LY.SMALL)
def test_engine_run_small_layouts(gpu, oracle, table, name, bits, mn):
    lay = LY.build(name)
    size, streams, _ = lay
    off, lens = _split_cols(streams)
    eng = gpu.Engine()
    buf = gpu.DeviceBuffer(size + 4096)
    try:
        for poison in LY.POISONS:  # one engine, one buffer: all three equal the oracle
            buf.from_host(LY.fill(lay, poison))
            eng.run(buf.ptr, off, lens, bits=bits, min_size=mn)
            eng.finish()
            _check_run(eng, streams, oracle, table, bits, mn)
        for lead, poison in ((4096, 0xFF), (16, "random")):  # d_data inside the allocation
            host = np.concatenate([LY.fill((lead, [], ""), poison), LY.fill(lay, poison)])
            buf.from_host(host)
            eng.run(buf.ptr + lead, off, lens, bits=bits, min_size=mn)
            eng.finish()
            _check_run(eng, streams, oracle, table, bits, mn)
    finally:
        buf.free()
        eng.close()


@pytest.mark.parametrize("name", LY.SMALL)
def test_engine_hash_small_layouts(gpu, name):
    lay = LY.build(name)
    size, streams, _ = lay
    off, lens = _split_cols(streams)
    eng = gpu.Engine()
    buf = gpu.DeviceBuffer(size + 4096)
    try:
        for long_mode in (0, 1):  # the engine's own choice of SHA-256 path, then all per-lane
            with gpu.debug_knob(gpu.KNOB_LONG_MODE, long_mode):
                for poison in LY.POISONS:
                    buf.from_host(LY.fill(lay, poison))
                    eng.hash(buf.ptr, off, lens)
                    assert eng.finish() == len(streams)
                    _check_hash(eng, streams)
                for lead, poison in ((4096, 0x00), (16, 0xFF)):
                    host = np.concatenate([LY.fill((lead, [], ""), poison),
                                           LY.fill(lay, poison)])
                    buf.from_host(host)
                    eng.hash(buf.ptr + lead, off, lens)
                    assert eng.finish() == len(streams)
                    _check_hash(eng, streams)
    finally:
        buf.free()
        eng.close()


# ---- b. host batch and hashers on host layouts -------------------------------------------------
@pytest.mark.parametrize("name", LY.SMALL)
def test_split_hash_batch_at_unaligned_host_offsets(gpu, oracle, table, name):
    """bsg_split_hash_batch copies each stream to the device itself, so host offsets need no
    alignment: every offset moved by 1, 2, 3 and 7 bytes."""
    lay = LY.build(name)
    _, streams, _ = lay
    off, lens = _split_cols(streams)
    for k, delta in enumerate((1, 2, 3, 7)):
        poison = LY.POISONS[k % 3]
        host = np.concatenate([LY.fill((delta, [], ""), poison), LY.fill(lay, poison)])
        for bits, mn in PARAMS:
            recs, counts = gpu.split_hash_batch_at(host, [o + delta for o in off], lens,
                                                   bits=bits, min_size=mn)
            _check_records(recs, counts, streams, oracle, table, bits, mn)


@pytest.mark.parametrize("name", ["gaps", "descending", "aliased"])
def test_hashers_host_base(gpu, name):
    """Hasher.sum_at and sha256_batch_at over a host base. The whole layout holds a blob of
    16 KiB or more, which sends a small batch to the hasher's engine; without the long blobs it
    goes to k_sha_blobs, one blob per lane, from a private copy of base[0 .. hi)."""
    lay = LY.build(name)
    _, streams, _ = lay
    short = [s for s in streams if s[1] < 16 << 10]
    assert 2 <= len(short) < len(streams)
    h = gpu.Hasher()
    try:
        for k, delta in enumerate((0, 1, 2, 3, 7)):
            poison = LY.POISONS[k % 3]
            host = np.concatenate([LY.fill((delta, [], ""), poison), LY.fill(lay, poison)])
            for sel in (streams, short):
                off = [o + delta for o, _, _ in sel]
                lens = [n for _, n, _ in sel]
                want = [_sha(seed, n) for _, n, seed in sel]
                assert h.sum_at(host, off, lens) == want, (delta, len(sel))
                assert gpu.sha256_batch_at(host, off, lens) == want, (delta, len(sel))
                assert gpu.sha256_batch_at(host.ctypes.data, off, lens) == want
    finally:
        h.free()


# ---- c. hashers with a device base -----------------------------------------------------------
BLOB_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 4095]
RESIDUES = [0, 1, 2, 3, 5, 15, 63]  # mod 64: every residue mod 4; 0, 5, 15 mod 16; 63 mod 64


def _blob_layout():
    """Every BLOB_LENS length at every start residue, ascending, with poisoned gaps of 0 .. 126
    bytes. No slack: bsg_hasher::sum hashes a device base from a private copy of base[0 .. hi)
    with its own read slack (bsgpu_host.cpp), so the caller's allocation may end at the last
    blob's last byte, and here it does."""
    blobs, o = [], 0
    for i, n in enumerate(BLOB_LENS):
        for j, r in enumerate(RESIDUES):
            blobs.append((o + r, n, 9000 + 16 * i + j))
            o = (o + r + n + 63) // 64 * 64 + 64 * ((i + j) % 2)
    hi = max(p + n for p, n, _ in blobs)
    assert {p % 4 for p, _, _ in blobs} == {0, 1, 2, 3}
    assert {0, 5, 15} <= {p % 16 for p, _, _ in blobs} and 63 in {p % 64 for p, _, _ in blobs}
    return hi, blobs


def _blob_queries(blobs):
    """{order: [(off, len, expected ref)]}: ascending, descending, aliased (every blob twice,
    prefixes, and tails from interior offsets of every residue mod 4)."""
    plain = [(p, n, _sha(seed, n)) for p, n, seed in blobs]
    ali = list(plain) + list(plain)
    for p, n, seed in blobs:
        if n >= 120:
            d = splitmix_array(seed, n).tobytes()
            for cut in (1, 2, 3, 5, 64):
                ali.append((p, n - cut, hashlib.sha256(d[:n - cut]).digest()))
                ali.append((p + cut, n - cut, hashlib.sha256(d[cut:]).digest()))
    return {"ascending": plain, "descending": plain[::-1], "aliased": ali}


def test_hashers_device_base(gpu):
    hi, blobs = _blob_layout()
    queries = _blob_queries(blobs)
    L = gpu.lib()
    ptr = L.bsg_device_malloc(0, hi)  # ends at the last blob's last byte (see _blob_layout)
    assert ptr
    h = gpu.Hasher()
    try:
        for poison in LY.POISONS:
            host = np.ascontiguousarray(LY.fill((hi + LY.READ_SLACK, blobs, ""), poison)[:hi])
            assert L.bsg_memcpy(0, ptr, host.ctypes.data, hi, 0) == 0
            for order, q in queries.items():
                off, lens, want = [x[0] for x in q], [x[1] for x in q], [x[2] for x in q]
                assert h.sum_at(ptr, off, lens) == want, (poison, order)
                assert gpu.sha256_batch_at(ptr, off, lens) == want, (poison, order)
    finally:
        h.free()
        L.bsg_device_free(0, ptr)


# ---- d. regions on sparse layouts --------------------------------------------------------------
SPARSE_R = {"three_groups": 3, "empty_region": 3, "last_region": 3, "border_inside": 2,
            "past_4gib": 5, "few_jobs": 1}


@pytest.fixture(scope="module")
def big(gpu):
    """One allocation of 4 GiB + 8 MiB; the tests write only their streams and the slack."""
    buf = gpu.DeviceBuffer(LY.SPARSE_SIZE - LY.READ_SLACK)
    yield buf
    buf.free()


def _predict(first_bytes, jobs, span, case):
    """R and the jobs per region the oracle's chunk starts predict; the case's conditions are
    asserted here, before the GPU's answer is looked at."""
    assert span > LY.REGION_BYTES
    R = LY.expected_nregions(span, jobs)
    assert R == SPARSE_R[case], (jobs, span)
    assert R == min(-(-span // (1 << 30)), max(jobs // 4096, 1))  # waves / 16 = 64 does not bind
    sizes = np.bincount([LY.expected_region(int(x), R, span) for x in first_bytes], minlength=R)
    assert int(sizes.sum()) == jobs
    return R, sizes


def _check_regions(eng, jobs, R, sizes):
    d = eng.diag()
    assert d["nlong"] == 0 and d["nshort"] == jobs  # every job per-lane
    reg = eng.regions()
    assert reg["nregions"] == R
    assert reg["off"][0] == 0 and reg["off"][R] == jobs
    assert list(np.diff(reg["off"])) == list(sizes)


def _sparse_run(gpu, oracle, table, big, case, long_mode=1):
    lay = LY.sparse(case)
    _, streams, _ = lay
    off, lens = _split_cols(streams)
    span = LY.span_of(streams)
    first, longest = [], 0
    for o, n, seed in streams:
        ch = _want(oracle, table, seed, n, 8, 64)[0]
        first.append(o + ch["offset"].astype(np.int64))
        longest = max(longest, int(ch["len"].max()))
    first = np.concatenate(first)
    assert longest + 9 <= 1023 * 64  # no chunk reaches the wave path's 1,024 blocks
    R, sizes = _predict(first, len(first), span, case)
    for lo, b in LY.pieces(lay, 0xFF):
        big.from_host(b, lo)
    eng = gpu.Engine()
    try:
        with gpu.debug_knob(gpu.KNOB_LONG_MODE, long_mode):
            eng.run(big.ptr, off, lens, bits=8, min_size=64)
            eng.finish()
        _check_regions(eng, len(first), R, sizes)
        _check_run(eng, streams, oracle, table, 8, 64)
    finally:
        eng.close()
    return first, R, sizes, span


def test_regions_three_groups(gpu, oracle, table, big):
    first, R, sizes, _ = _sparse_run(gpu, oracle, table, big, "three_groups")
    assert int(first.min()) == 0  # a job at d_data itself (job_region's o <= 0)
    assert (sizes >= 4096).all()


def test_regions_three_groups_auto_mode(gpu, oracle, table, big):
    _sparse_run(gpu, oracle, table, big, "three_groups", long_mode=0)


def test_regions_empty_region(gpu, oracle, table, big):
    _, _, sizes, _ = _sparse_run(gpu, oracle, table, big, "empty_region")
    assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0


def test_regions_all_in_last_region(gpu, oracle, table, big):
    _, _, sizes, _ = _sparse_run(gpu, oracle, table, big, "last_region")
    assert list(sizes[:2]) == [1, 0] and sizes[2] >= 2 * 4096


def test_regions_border_inside_a_stream(gpu, oracle, table, big):
    _, streams, _ = LY.sparse("border_inside")
    o, n, seed = streams[0]
    ch = _want(oracle, table, seed, n, 8, 64)[0]
    span = LY.span_of(streams)
    border = -(-span // 2)  # the first offset of region 1 when R = 2
    lo = o + ch["offset"].astype(np.int64)
    hi = lo + ch["len"].astype(np.int64)
    assert ((lo < border) & (hi > border)).sum() == 1  # one chunk straddles: region 0
    assert (hi <= border).sum() > 4096 and (lo >= border).sum() > 4096
    _, R, sizes, _ = _sparse_run(gpu, oracle, table, big, "border_inside")
    assert R == 2 and sizes[0] == (lo < border).sum()


def test_regions_data_off_past_4gib(gpu, oracle, table, big):
    first, R, sizes, _ = _sparse_run(gpu, oracle, table, big, "past_4gib")
    assert int(first.max()) > (1 << 32) + (3 << 20)
    assert list(sizes[1:4]) == [0, 0, 0] and sizes[0] > 4096 and sizes[4] > 4096


def test_regions_few_jobs_one_region(gpu, oracle, table, big):
    first, R, _, span = _sparse_run(gpu, oracle, table, big, "few_jobs")
    assert R == 1 and len(first) < 8192 and span > LY.REGION_BYTES


def test_regions_hash_chunks_as_blobs(gpu, oracle, table, big):
    """three_groups through Engine.hash: every oracle chunk a blob in a 16-aligned slot of its
    own, each group's slots packed from the group's first offset on."""
    _, streams, _ = LY.sparse("three_groups")
    blobs, host, cur, base = [], {}, None, None  # blobs: (off, len, bytes)
    for o, n, seed in streams:
        if cur is None or o >= cur + (64 << 20):  # a new group
            cur = base = o
            host[base] = []
        d = splitmix_array(seed, n)
        for c in _want(oracle, table, seed, n, 8, 64)[0]:
            b = d[int(c["offset"]):int(c["offset"]) + int(c["len"])]
            blobs.append((cur, len(b), b))
            host[base].append((cur - base, b))
            cur = LY.align16(cur + len(b)) + (16 if len(blobs) % 7 == 0 else 0)
    # last: a 64-byte blob and an empty one at its end, off == span (job_region's R - 1 clamp;
    # in a hash run an empty blob is a job too)
    tail = splitmix_array(4242, 64)
    blobs += [(cur, 64, tail), (cur + 64, 0, tail[:0])]
    host[base].append((cur - base, tail))
    assert len(host) == 3 and 12288 <= len(blobs) <= 65535
    for base, parts in host.items():
        end = max(p + len(b) for p, b in parts) + LY.READ_SLACK
        assert base + end <= LY.SPARSE_SIZE
        piece = np.full(end, 0xFF, dtype=np.uint8)
        for p, b in parts:
            piece[p:p + len(b)] = b
        big.from_host(piece, base)
    off, lens = [x[0] for x in blobs], [x[1] for x in blobs]
    span = max(o + n for o, n in zip(off, lens))
    assert off[-1] == span and off[0] == 0
    R, sizes = _predict(off, len(blobs), span, "three_groups")
    want = [hashlib.sha256(b.tobytes()).digest() for _, _, b in blobs]
    eng = gpu.Engine()
    try:
        with gpu.debug_knob(gpu.KNOB_LONG_MODE, 1):
            eng.hash(big.ptr, off, lens)
            assert eng.finish() == len(blobs)
        _check_regions(eng, len(blobs), R, sizes)
        recs = eng.chunks()
        bad = [i for i in range(len(blobs)) if recs[i]["ref"].tobytes() != want[i]]
        assert not bad, (len(bad), bad[:8])
        assert (recs["len"] == np.array(lens, dtype=np.uint64)).all()
    finally:
        eng.close()


# ---- e. refusals -----------------------------------------------------------------------------
def _refused(call, *args, **kw):
    with pytest.raises(Exception) as ei:
        call(*args, **kw)
    assert getattr(ei.value, "code", None) == EINVAL, ei.value


def test_engine_refuses_bad_layouts(gpu, oracle, table):
    """engine_batch's checks: BSG_EINVAL before anything is enqueued, and the engine then does
    an ordinary run."""
    lay = LY.gaps()
    size, streams, _ = lay
    off, lens = _split_cols(streams)
    buf = gpu.DeviceBuffer(size)
    buf.from_host(LY.fill(lay, 0xFF))
    eng = gpu.Engine()
    bad = [("d_data + 1", buf.ptr + 1, [0], [64]),
           ("d_data + 4", buf.ptr + 4, [0], [64]),
           ("d_data + 8", buf.ptr + 8, [0], [64]),
           ("off + len wraps", buf.ptr, [0, 2**64 - 16], [64, 32]),
           ("len = 2^40", buf.ptr, [0], [1 << 40]),
           ("empty stream past the allocation", buf.ptr, [0, 1 << 30], [64, 0]),
           ("empty stream at the top of the address space", buf.ptr, [0, 2**64 - 16], [64, 0]),
           ("off % 16", buf.ptr, [8], [64])]
    try:
        for what, ptr, o, n in bad:
            _refused(eng.run, ptr, o, n, bits=8, min_size=64)
            _refused(eng.hash, ptr, o, n)
            with pytest.raises(gpu.BsgError):  # nothing was enqueued
                eng.finish()
            eng.run(buf.ptr, off, lens, bits=8, min_size=64)
            eng.finish()
            _check_run(eng, streams, oracle, table, 8, 64)
        eng.hash(buf.ptr, off, lens)
        assert eng.finish() == len(streams)
        _check_hash(eng, streams)
    finally:
        buf.free()
        eng.close()


def test_hashers_refuse_wrapped_offsets(gpu):
    lay = LY.gaps()
    size, streams, _ = lay
    short = [s for s in streams if s[1] < 16 << 10]
    off, lens = _split_cols(short)
    want = [_sha(seed, n) for _, n, seed in short]
    host = LY.fill(lay, 0xFF)
    buf = gpu.DeviceBuffer(size)
    buf.from_host(host)
    h = gpu.Hasher()
    try:
        for base in (host, buf.ptr):
            _refused(h.sum_at, base, [0, 2**64 - 8], [64, 64])
            _refused(gpu.sha256_batch_at, base, [0, 2**64 - 8], [64, 64])
            assert h.sum_at(base, off, lens) == want
            assert gpu.sha256_batch_at(base, off, lens) == want
    finally:
        h.free()
        buf.free()
