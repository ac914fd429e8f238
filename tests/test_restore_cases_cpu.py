"""The model of restore_cases.py, without a device: it restores the oracle's records of the
dedup_cases inputs from a pool made with DC.packed to the original bytes, reports every error
class with the right index, and the case builders have the properties they claim."""
import ctypes

import numpy as np
import pytest

import dedup_cases as DC
import restore_cases as RC
from bs_amd import bsgpu

CASES = ["edited_copies", "residues", "tiny_chunks", "zeros", "one_chunk_streams",
         "long_among_short"]


def _model(c, **kw):
    out0 = np.full(c["cap"], RC.FILL, dtype=np.uint8)
    return RC.expected(c["pool"], c["blobs"], c["recs"], c["out_off"], c["out_len"], out0,
                       kw.pop("verify", c["verify"]), **kw)


def _restored(c, out):
    for s, d in enumerate(c["want"]):
        o = c["out_off"][s]
        assert out[o:o + len(d)].tobytes() == bytes(d), s
    keep = np.ones(c["cap"], dtype=bool)
    for o, n in zip(c["out_off"], c["out_len"]):
        keep[o:o + n] = False
    assert (out[keep] == RC.FILL).all()


def test_struct_sizes():
    assert bsgpu.POOL_BLOB_DTYPE.itemsize == 48
    assert ctypes.sizeof(bsgpu.RestoreInfo) == 32
    with open(bsgpu.HEADER_PATH) as f:
        text = f.read()
    assert "} bsg_pool_blob; /* 48 bytes */" in text
    assert "bsg_engine_restore" in bsgpu.exported_symbols_from_header()


@pytest.mark.parametrize("name", CASES)
def test_round_trip_from_packed(oracle, table, name):
    streams, bits, mn = getattr(DC, name)()
    recs = DC.oracle_records(oracle, table, streams, bits, mn)
    pool, blobs = RC.packed_pool(streams, recs)
    assert len(blobs) <= len(recs) and len(pool) == int(blobs["len"].sum())
    lens = [len(d) for d in streams]
    order = list(np.random.default_rng(3).permutation(len(lens)))
    c = RC.case(pool, blobs, recs, lens, order=order, want=streams)
    rc, info, out = _model(c)
    assert rc == RC.OK
    assert info == {"bad_record": RC.NONE, "bad_blob": RC.NONE, "bytes": sum(lens), "verified": 0}
    _restored(c, out)


def test_verify_and_first_of_equal_refs():
    c = RC.small_valid()
    rc, info, out = _model(c, verify=True)
    assert rc == RC.OK and info["verified"] == int(c["blobs"]["len"].sum())
    _restored(c, out)
    # a second blob with blob 1's ref and other bytes: the smaller index is used, and verify
    # names the later one
    blobs = np.concatenate([c["blobs"], c["blobs"][1:2]])
    blobs[-1]["off"] = c["blobs"][2]["off"]
    d = dict(c, blobs=blobs)
    rc, info, out = _model(d)
    assert rc == RC.OK
    _restored(c, out)
    rc, info, out = _model(d, verify=True)
    assert rc == RC.ECORRUPT and info["bad_blob"] == len(blobs) - 1
    assert (out == RC.FILL).all()


def test_error_classes():
    c = RC.small_valid()
    n = len(c["recs"])
    # not found: the smallest record of a dropped blob
    d = dict(c, blobs=np.delete(c["blobs"], [1, 4]))
    rc, info, out = _model(d)
    first = min(i for i in range(n) if c["recs"][i]["ref"].tobytes()
                in (c["blobs"][1]["ref"].tobytes(), c["blobs"][4]["ref"].tobytes()))
    assert (rc, info["bad_record"]) == (RC.ENOTFOUND, first) and (out == RC.FILL).all()
    # a record and its blob disagree on len
    blobs = c["blobs"].copy()
    blobs[3]["len"] -= 1
    rc, info, out = _model(dict(c, blobs=blobs))
    i3 = next(i for i in range(n) if c["recs"][i]["ref"].tobytes() == blobs[3]["ref"].tobytes())
    assert (rc, info["bad_record"]) == (RC.ECORRUPT, i3) and (out == RC.FILL).all()
    # both: not found wins
    rc, info, out = _model(dict(c, blobs=np.delete(blobs, [5])))
    i5 = next(i for i in range(n)
              if c["recs"][i]["ref"].tobytes() == c["blobs"][5]["ref"].tobytes())
    assert (rc, info["bad_record"]) == (RC.ENOTFOUND, i5)
    # a damaged blob: seen only with verify
    pool = c["pool"].copy()
    pool[int(c["blobs"][4]["off"]) + 2] ^= 1
    pool[int(c["blobs"][2]["off"])] ^= 0x80
    rc, info, out = _model(dict(c, pool=pool), verify=True)
    assert (rc, info["bad_blob"], info["bytes"]) == (RC.ECORRUPT, 2, 0) and (out == RC.FILL).all()
    rc, info, out = _model(dict(c, pool=pool))
    assert rc == RC.OK and info["bad_blob"] == RC.NONE
    o = c["out_off"][0] + 47
    assert out[o] == c["want"][0][47] ^ 0x80
    # the layout rules: EINVAL, whatever else is wrong
    recs = c["recs"].copy()
    recs[1]["offset"] += 1
    assert _model(dict(c, recs=recs, blobs=np.delete(c["blobs"], [1])))[0] == RC.EINVAL
    assert _model(c, out_shift=8)[0] == RC.EINVAL
    end = int((c["blobs"]["off"] + c["blobs"]["len"]).max())
    assert _model(c, verify=True, pool_bytes=end + 255)[0] == RC.EINVAL
    assert _model(c, verify=True, pool_bytes=end + 256)[0] == RC.OK
    assert _model(c, pool_bytes=end)[0] == RC.OK
    assert _model(c, pool_bytes=end - 1)[0] == RC.EINVAL


def test_builders():
    c = RC.segment_edges()
    assert c["out_len"][:8] == [0, 1, 15, 16, 17, RC.T - 1, RC.T, RC.T + 1]
    assert c["out_len"][8] > 3 * RC.T and RC.T % 16 == 0
    rc, info, out = _model(c)
    assert rc == RC.OK
    _restored(c, out)
    for r in (0, 7, 15):
        c = RC.source_residue(r)
        assert (c["blobs"]["off"] % 16 == r).all()
        assert sorted(set(c["blobs"]["len"].tolist())) == list(RC.RESIDUE_LENS)
        assert len(c["recs"]) == 40
        rc, info, out = _model(c)
        assert rc == RC.OK
        _restored(c, out)
    c = RC.many_blobs(70)
    assert len(set(r.tobytes() for r in c["blobs"]["ref"])) == 70
    rc, info, out = _model(c)
    assert rc == RC.OK and info["verified"] == 70 * 16
    _restored(c, out)
