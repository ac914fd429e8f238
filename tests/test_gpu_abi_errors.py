"""C-ABI error behaviour on the device (mirrors the reference's error conventions: Write after
Close fails, a missing root fails NewReader with bs.ErrNotFound) and the persistent hasher."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check_chunks(data: bytes, ch) -> None:
    assert b"".join(data[int(c["offset"]):int(c["offset"] + c["len"])] for c in ch) == data
    for c in ch:
        blob = data[int(c["offset"]):int(c["offset"] + c["len"])]
        assert bytes(c["ref"]) == hashlib.sha256(blob).digest()


def test_write_after_close_and_late_knobs(gpu):
    from bs_amd.synth import splitmix_bytes
    L = gpu.lib()
    a, b = splitmix_bytes(1, 300_000), splitmix_bytes(2, 200_000)
    w = gpu.StreamingSplitter()
    w.write(a)
    assert L.bsg_set_tile(w.h, 1 << 20) == -22        # tile fixed once bytes arrived
    assert L.bsg_set_carry_cap(w.h, 0) == -22
    w.close()
    assert L.bsg_write(w.h, b"y", 1) == -71           # BSG_ESTATE: Write after Close
    assert L.bsg_close(w.h) == 0                      # Close is idempotent
    _check_chunks(a, w.drain())
    w.reset()                                         # a reset context takes a new stream
    w.write(b)
    w.close()
    _check_chunks(b, w.drain())
    w.free()


def test_reset_equals_fresh(gpu, oracle, table):
    """bsg_reset leaves nothing of the previous stream: after stream A (at offsets past 2^40,
    written in uneven pieces), stream B through write_window / write_commit on the same context
    gives the oracle's chunks, which are also those of a fresh context given the same calls, and
    the counters read zero before B's first byte. The tile set before A is a setting, not stream
    state: it still applies, so B (3 MiB + 17 bytes) crosses three 1 MiB tile boundaries, ends
    on a short final tile, and no host-to-device copy exceeds a 1 MiB stage."""
    from bs_amd.synth import splitmix_array
    L = gpu.lib()
    n, tile = (3 << 20) + 17, 1 << 20
    a, b = splitmix_array(4101, n), splitmix_array(4102, n)

    def raw_stats(w):
        st = gpu.StreamStats()
        assert L.bsg_stream_stats_get(w.h, ctypes.byref(st)) == 0
        return st

    def run_b(w):
        done = 0
        while done < n:
            win = w.window()
            k = min(len(win), n - done, 700_001)
            win[:k] = memoryview(b)[done:done + k]
            w.commit(k)
            done += k
        w.close()
        return w.drain(), raw_stats(w)

    def same(ch, want, base=0):
        assert len(ch) == len(want)
        assert (ch["offset"] == want["offset"] + np.uint64(base)).all()
        for f in ("len", "level", "ref"):
            assert (ch[f] == want[f]).all(), f

    w = gpu.StreamingSplitter(bits=13, min_size=256, tile=tile)
    w.set_stream_base(1 << 40)
    got, at = [], 0
    for k in (1, 999_999, 64, 1 << 20, n):
        w.write(memoryview(a)[at:at + k])
        got.append(w.drain())
        at += k
    w.close()
    got.append(w.drain())
    same(np.concatenate(got), oracle.split(table, a, bits=13, min_size=256), base=1 << 40)
    assert raw_stats(w).h2d_bytes == n

    w.reset()
    st = raw_stats(w)
    for f in ("host_bytes", "host_copy_ns", "stage_wait_ns", "h2d_bytes", "h2d_copies",
              "h2d_busy_ns", "h2d_span_ns", "last_tile_ns", "tail_ns", "src_nodes"):
        assert getattr(st, f) == 0, f
    assert list(st.copy_bytes_node) == [0, 0, 0, 0]
    ch_reset, st_reset = run_b(w)
    w.free()

    fresh = gpu.StreamingSplitter(bits=13, min_size=256, tile=tile)
    ch_fresh, st_fresh = run_b(fresh)
    fresh.free()

    want = oracle.split(table, b, bits=13, min_size=256)
    same(ch_reset, want)                               # offsets from 0 again: the base is gone
    same(ch_fresh, want)
    assert st_reset.h2d_bytes == n
    assert st_reset.h2d_copies >= -(-n // tile)        # a stage is one tile at most: >= 4 copies
    assert st_reset.h2d_copies == st_fresh.h2d_copies


def test_reader_missing_root(gpu):
    st = gpu.MemStore()
    with pytest.raises(gpu.BsgError) as ei:
        gpu.Reader(st, bytes(32))
    assert ei.value.code == gpu.NOT_FOUND


def test_persistent_hasher_batches(gpu):
    L = gpu.lib()
    L.bsg_hasher_new.restype = ctypes.c_void_p
    L.bsg_hasher_new.argtypes = [ctypes.c_int]
    L.bsg_hasher_sum.restype = ctypes.c_int
    L.bsg_hasher_sum.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.bsg_hasher_free.argtypes = [ctypes.c_void_p]
    h = L.bsg_hasher_new(0)
    assert h
    rng = np.random.default_rng(11)
    try:
        for n in (1, 7, 300):  # the buffers grow and are reused across calls
            blobs = [rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes()
                     for _ in range(n)]
            packed = b"".join(blobs)
            off = np.cumsum([0] + [len(b) for b in blobs[:-1]]).astype(np.uint64)
            ln = np.array([len(b) for b in blobs], dtype=np.uint64)
            out = ctypes.create_string_buffer(32 * n)
            assert L.bsg_hasher_sum(h, packed or b"\0", off.ctypes.data, ln.ctypes.data, n,
                                    out) == 0
            assert [out.raw[32 * i:32 * i + 32] for i in range(n)] == \
                [hashlib.sha256(b).digest() for b in blobs]
    finally:
        L.bsg_hasher_free(h)


def test_close_in_steps(gpu, oracle, table):
    """bsg_close_begin + bsg_close_step: the tiles still on the device finish one per step, and
    the chunks of all steps are exactly those of bsg_close (the oracle's); a step before begin is
    BSG_ESTATE, a step after the last returns 0 tiles left."""
    import ctypes
    from bs_amd.synth import splitmix_array
    L = gpu.lib()
    d = splitmix_array(77, (9 << 20) + 4321)
    w = gpu.StreamingSplitter(bits=13, min_size=256, tile=1 << 20)
    left = ctypes.c_size_t(5)
    assert L.bsg_close_step(w.h, ctypes.byref(left)) == -71 and left.value == 0
    got = []
    for i in range(0, len(d), 3 << 20):
        w.write(memoryview(d)[i:i + (3 << 20)])
        got.append(w.drain())
    steps = list(w.close_steps())
    assert len(steps) >= 2                           # several tiles were still on the device
    got += steps
    assert L.bsg_close_step(w.h, ctypes.byref(left)) == 0 and left.value == 0
    assert L.bsg_write(w.h, b"y", 1) == -71
    w.free()
    want = oracle.split(table, d, bits=13, min_size=256)
    ch = np.concatenate(got)
    assert len(ch) == len(want)
    for f in ("offset", "len", "level", "ref"):
        assert (ch[f] == want[f]).all(), f
    e = gpu.StreamingSplitter()                      # an empty stream: nothing on the device
    assert all(len(x) == 0 for x in e.close_steps())
    e.free()


def test_engine_destroy_frees_every_pass(gpu, table):
    """bsg_engine_destroy frees what every pass of the engine allocated. One engine runs a 64 KiB
    planted stream, builds its trees, dedups into a ref set, packs, and restores with verify (so
    the tree, dedup and restore workspaces and the second engine all hold buffers); the device
    pointers the ABI exposes are noted, the engine destroyed and the set freed. A second engine,
    warmed with the same zero-length hash run beforehand so that it allocates nothing now, must
    refuse each noted pointer as d_data (BSG_EINVAL: not a live HIP allocation; checked before
    any launch, so the pointer is never read). A pointer it accepts was leaked."""
    import planting as P
    import restore_cases as RC
    L = gpu.lib()
    bits = 8
    data = P.level_stream(table, bits, np.tile([0, 0, 9, 0, 1, 0, 17, 0], 128))
    assert data.size == 64 << 10
    src = gpu.DeviceBuffer(data.size)
    src.from_host(data)
    out = gpu.DeviceBuffer(data.size)
    zero = (ctypes.c_uint64 * 1)(0)
    zp = ctypes.cast(zero, ctypes.POINTER(ctypes.c_uint64))

    def hash_at(eng, ptr):
        return L.bsg_engine_hash(eng.h, ptr, zp, zp, 1)

    probe = gpu.Engine()
    assert hash_at(probe, src.ptr) == 0
    probe.finish()

    eng, rset = gpu.Engine(), gpu.RefSet()
    eng.run(src.ptr, [0], [data.size], bits=bits, min_size=64)
    assert eng.finish() == 1024
    recs = eng.chunks()
    roots, _, nodes, _ = eng.trees()
    assert len(roots) == 1 and len(nodes) > 1
    _, uniq, _ = eng.dedup(rset)
    assert 0 < eng.nunique < len(recs) and rset.count() == eng.nunique
    packed = gpu.DeviceBuffer(eng.unique_bytes)
    eng.pack_unique(packed)
    u = uniq.astype(np.int64)
    blobs = RC.make_blobs(recs["offset"][u], recs["len"][u], recs["ref"][u])
    info = eng.restore(src, blobs, recs, out, [0], [data.size], verify=True)
    assert info["bytes"] == data.size and info["verified"] == eng.unique_bytes
    assert (out.to_host() == data).all()

    names = ("chunks", "tree_nodes", "tree_arena", "roots", "dedup_first", "dedup_uniq",
             "dedup_pack_off")
    ptrs = {n: getattr(L, f"bsg_engine_{n}_device")(eng.h) for n in names}
    assert all(ptrs.values()), ptrs
    eng.close()
    rset.free()
    for n, p in ptrs.items():
        assert hash_at(probe, p) == -22, n             # BSG_EINVAL: freed with the engine
    assert hash_at(probe, src.ptr) == 0                # the probe still works
    probe.finish()
    probe.close()
    for b in (src, out, packed):
        b.free()


def test_engine_profile_modes(gpu):
    """bsg_engine_profile: 1 times every stage, 2 only the SHA-256 stage (the scan and selection
    stages read -1), 0 off (stage_ms refused); other modes are refused."""
    from bs_amd.synth import splitmix_array
    L = gpu.lib()
    data = splitmix_array(5, 3 << 20)
    buf = gpu.DeviceBuffer(len(data) + 4096)
    buf.from_host(data)
    eng = gpu.Engine()
    assert L.bsg_engine_profile(eng.h, 3) == -22 and L.bsg_engine_profile(eng.h, -1) == -22
    for mode in (1, 2):
        eng.profile(mode)
        eng.run(buf.ptr, [0], [len(data)])
        eng.finish()
        ms = eng.stage_ms()
        assert ms[2] > 0
        assert (ms[0] > 0 and ms[1] > 0) if mode == 1 else (ms[0] == -1 and ms[1] == -1)
    eng.profile(0)
    st = (ctypes.c_float * 3)()
    assert L.bsg_engine_stage_ms(eng.h, st) == -22
    eng.close()
    buf.free()
