"""bsg_engine_restore on the device against the model of restore_cases.py: the return code, the
bsg_restore_info and every byte of an output buffer pre-filled with 0xA5, guards included."""
import numpy as np
import pytest

import dedup_cases as DC
import restore_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _dedup_arrays(gpu, eng, n, nu):
    """The engine's dedup result as it stands (no new bsg_engine_dedup)."""
    first = np.zeros(max(n, 1), dtype=np.uint64)
    uniq = np.zeros(max(nu, 1), dtype=np.uint64)
    pack_off = np.zeros(nu + 1, dtype=np.uint64)
    rc = gpu.lib().bsg_engine_copy_dedup(eng.h, first.ctypes.data, n, uniq.ctypes.data,
                                         pack_off.ctypes.data, nu)
    assert rc == 0
    return first[:n].tolist(), uniq[:nu].tolist(), pack_off.tolist()


# ---- 1. round trip through dedup + pack_unique ---------------------------------------------------
def test_round_trip(gpu, eng, oracle, table):
    streams, bits, mn = DC.edited_copies()
    host, off, lens = DC.place(streams)
    src = gpu.DeviceBuffer(host.size)
    src.from_host(host)
    eng.run(src.ptr, off, lens, bits=bits, min_size=mn)
    eng.finish()
    recs = eng.chunks()
    want = DC.oracle_records(oracle, table, streams, bits, mn)
    assert len(recs) == len(want) and (recs["ref"] == want["ref"]).all()
    first, uniq, pack_off = eng.dedup()
    assert eng.nunique < len(recs)
    packed = gpu.DeviceBuffer(eng.unique_bytes)
    eng.pack_unique(packed)
    u = uniq.astype(np.int64)
    blobs = RC.make_blobs(pack_off[:-1], recs["len"][u], recs["ref"][u])
    c = RC.case(packed.to_host(), blobs, recs, lens, order=[1, 0], want=streams)
    before = _dedup_arrays(gpu, eng, len(recs), eng.nunique)

    # restore from the packed buffer itself (tight: pool_bytes is the packed size), then split
    # the restored bytes again
    cap = c["cap"]
    out = gpu.DeviceBuffer(RC.GUARD + cap + RC.GUARD)
    out.from_host(np.full(out.nbytes, RC.FILL, dtype=np.uint8))
    info = eng.restore(packed, blobs, recs, out.ptr + RC.GUARD, c["out_off"], lens,
                       pool_bytes=eng.unique_bytes, out_cap=cap)
    assert info == {"bad_record": RC.NONE, "bad_blob": RC.NONE, "bytes": sum(lens), "verified": 0}
    got = out.to_host()
    model = RC.expected(c["pool"], blobs, recs, c["out_off"], lens,
                        np.full(cap, RC.FILL, dtype=np.uint8), False)
    assert model[0] == RC.OK
    assert (got[RC.GUARD:RC.GUARD + cap] == model[2]).all()
    assert (got[:RC.GUARD] == RC.FILL).all() and (got[RC.GUARD + cap:] == RC.FILL).all()
    RC.check_streams(c, got[RC.GUARD:RC.GUARD + cap])

    # the run, its records and its dedup result are as they were
    again = eng.chunks()
    assert again.tobytes() == recs.tobytes()
    assert _dedup_arrays(gpu, eng, len(recs), eng.nunique) == before

    eng.run(out.ptr, [RC.GUARD + o for o in c["out_off"]], lens, bits=bits, min_size=mn)
    eng.finish()
    assert eng.chunks().tobytes() == recs.tobytes()
    for b in (src, packed, out):
        b.free()


# ---- 2. many records, one blob -----------------------------------------------------------------
def test_many_records_one_blob(gpu, eng, oracle, table):
    streams, bits, mn = DC.zeros()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    pool, blobs = RC.packed_pool(streams, recs)
    assert len(blobs) <= 2 < len(recs)
    c = RC.case(pool, blobs, recs, [len(d) for d in streams], want=streams)
    rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
    RC.check_streams(c, out)


# ---- 3. segment edges --------------------------------------------------------------------------
def test_segment_edges(gpu, eng):
    c = RC.segment_edges()
    rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
    RC.check_streams(c, out)
    assert info["bytes"] == sum(c["out_len"])


# ---- 4. source residues ------------------------------------------------------------------------
def test_source_residues(gpu, eng):
    for r in range(16):
        c = RC.source_residue(r)
        rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
        RC.check_streams(c, out)


# ---- 5. verify on an aligned pool --------------------------------------------------------------
def test_verify(gpu, eng, oracle, table):
    streams, bits, mn = DC.edited_copies()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    pool, blobs = RC.aligned_pool(RC.unique_datas(streams, recs))
    assert (blobs["ref"] == recs["ref"][DC.expected(recs)[1].astype(np.int64)]).all()
    c = RC.case(pool, blobs, recs, [len(d) for d in streams], verify=True, want=streams)
    rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
    assert info["verified"] == int(blobs["len"].sum())
    RC.check_streams(c, out)

    bad = pool.copy()
    bad[int(blobs[7]["off"]) + int(blobs[7]["len"]) - 1] ^= 0x01
    bad[int(blobs[3]["off"])] ^= 0x80
    d = dict(c, pool=bad)
    rc, info, out = RC.run(gpu, eng, d, expect=RC.ECORRUPT)
    assert info["bad_blob"] == 3 and info["bytes"] == 0 and (out == RC.FILL).all()
    # unverified, the damaged bytes arrive
    rc, info, out = RC.run(gpu, eng, d, verify=False, expect=RC.OK)
    i3 = int(DC.expected(recs)[1][3])
    where = c["out_off"][int(recs[i3]["stream"])] + int(recs[i3]["offset"])
    assert out[where] == streams[int(recs[i3]["stream"])][int(recs[i3]["offset"])] ^ 0x80


# ---- 6. one blob more than two hash batches' worth less one ------------------------------------
def test_verify_batch_boundary(gpu, eng):
    c = RC.many_blobs(65537)
    rc, info, out = RC.run(gpu, eng, c, expect=RC.OK)
    assert info["verified"] == 16 * 65537
    RC.check_streams(c, out)
    bad = c["pool"].copy()
    bad[16 * 65536 + 15] ^= 0x10
    rc, info, out = RC.run(gpu, eng, dict(c, pool=bad), expect=RC.ECORRUPT)
    assert info["bad_blob"] == 65536 and (out == RC.FILL).all()


# ---- 7. missing and mismatched -----------------------------------------------------------------
def test_missing_and_mismatched(gpu, eng):
    c = RC.small_valid()
    recs, blobs = c["recs"], c["blobs"]

    def first_with(k):
        return next(i for i in range(len(recs))
                    if recs[i]["ref"].tobytes() == blobs[k]["ref"].tobytes())

    rc, info, out = RC.run(gpu, eng, dict(c, blobs=np.delete(blobs, [1, 4])),
                           expect=RC.ENOTFOUND)
    assert info["bad_record"] == min(first_with(1), first_with(4)) and (out == RC.FILL).all()
    off = blobs.copy()
    off[3]["len"] -= 1
    rc, info, out = RC.run(gpu, eng, dict(c, blobs=off), expect=RC.ECORRUPT)
    assert info["bad_record"] == first_with(3) and (out == RC.FILL).all()
    rc, info, out = RC.run(gpu, eng, dict(c, blobs=np.delete(off, [5])), expect=RC.ENOTFOUND)
    assert info["bad_record"] == first_with(5) and (out == RC.FILL).all()
    # two blobs under one ref: the smaller index is used
    two = np.concatenate([blobs, blobs[1:2]])
    two[-1]["off"] = blobs[2]["off"]
    rc, info, out = RC.run(gpu, eng, dict(c, blobs=two), expect=RC.OK)
    RC.check_streams(c, out)
    rc, info, out = RC.run(gpu, eng, dict(c, blobs=two), verify=True, expect=RC.ECORRUPT)
    assert info["bad_blob"] == len(two) - 1
