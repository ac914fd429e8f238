"""Every BSG_EINVAL rule of bsg_engine_restore as a one-line mutation of a valid call
(restore_cases.small_valid), and BSG_ESTATE on an engine with an unfinished run. Each call
must leave its output buffer, guards included, exactly as it was."""
import ctypes

import numpy as np
import pytest

import restore_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(gpu):
    e = gpu.Engine()
    yield e
    e.close()


def _recs(c, f):
    r = c["recs"].copy()
    f(r)
    return dict(c, recs=r)


def _swap(r):
    r[[3, 4]] = r[[4, 3]]


def _gap(r):            # record 1 starts one byte late (a gap before it, an overlap after it)
    r[1]["offset"] += 1


def _overlap(r):        # record 4 reaches one byte into record 5
    r[4]["len"] += 1


def _first(r):          # stream 2 starts at 1 (and every later record follows on)
    r["offset"][3:] += 1


def _short(r):
    r[7]["len"] -= 1


def _long(r):
    r[7]["len"] += 1


def _stream(r):         # stream == nstreams
    r[7]["stream"] = 3


def _zero(r):
    r[2]["len"] = 0


RECORD_RULES = {"gap": _gap, "overlap": _overlap, "swapped": _swap, "first_offset": _first,
                "short_end": _short, "long_end": _long, "stream_out_of_range": _stream,
                "zero_len": _zero}


@pytest.mark.parametrize("name", sorted(RECORD_RULES))
def test_record_rules(gpu, eng, name):
    c = RC.small_valid()
    assert len(c["recs"]) == 8 and c["recs"][3]["stream"] == 2
    RC.run(gpu, eng, _recs(c, RECORD_RULES[name]), expect=RC.EINVAL)


def test_valid_call(gpu, eng):
    c = RC.small_valid()
    for verify in (False, True):
        rc, info, out = RC.run(gpu, eng, c, verify=verify, expect=RC.OK)
        RC.check_streams(c, out)


def test_records_for_an_empty_stream(gpu, eng):
    c = RC.small_valid()
    lens = list(c["out_len"])
    lens[0] = 0
    RC.run(gpu, eng, dict(c, out_len=lens), expect=RC.EINVAL)
    # and a stream with bytes but no records
    lens = list(c["out_len"])
    lens[1] = 16
    RC.run(gpu, eng, dict(c, out_len=lens), expect=RC.EINVAL)


def test_output_rules(gpu, eng):
    c = RC.small_valid()
    RC.run(gpu, eng, c, out_shift=8, expect=RC.EINVAL)                 # d_out
    off = list(c["out_off"])
    off[0] += 8
    RC.run(gpu, eng, dict(c, out_off=off), expect=RC.EINVAL)           # out_off
    off = list(c["out_off"])
    off[0] = off[2] + 16                                               # stream 0 inside stream 2
    RC.run(gpu, eng, dict(c, out_off=off), expect=RC.EINVAL)
    RC.run(gpu, eng, dict(c, cap=max(o + n for o, n in zip(c["out_off"], c["out_len"])) - 1),
           expect=RC.EINVAL)                                           # past out_cap
    off = list(c["out_off"])
    off[2] = (1 << 64) - 16                                            # out_off + out_len wraps
    RC.run(gpu, eng, dict(c, out_off=off), expect=RC.EINVAL)


def test_output_inside_the_pool(gpu, eng):
    c = RC.small_valid()
    pool = np.concatenate([c["pool"], np.full(c["cap"], RC.FILL, dtype=np.uint8)])
    buf = gpu.DeviceBuffer(len(pool))
    try:
        buf.from_host(pool)
        for at, nbytes, want in ((len(c["pool"]), len(pool), RC.EINVAL),         # inside
                                 (len(c["pool"]) - 32, len(c["pool"]), RC.EINVAL),  # its end
                                 (len(c["pool"]), len(c["pool"]), RC.OK)):       # right after
            model = RC.expected(pool, c["blobs"], c["recs"], c["out_off"], c["out_len"],
                                pool[at:at + c["cap"]], False, pool_bytes=nbytes, out_in_pool=at)
            assert model[0] == want
            rc = RC.OK
            try:
                eng.restore(buf.ptr, c["blobs"], c["recs"], buf.ptr + at, c["out_off"],
                            c["out_len"], pool_bytes=nbytes, out_cap=c["cap"])
            except gpu.BsgError as e:
                rc = e.code
            assert rc == want
            got = buf.to_host()
            assert (got[:at] == pool[:at]).all()
            assert (got[at:at + c["cap"]] == model[2]).all()
    finally:
        buf.free()


def test_pool_rules(gpu, eng):
    c = RC.small_valid()
    end = int((c["blobs"]["off"] + c["blobs"]["len"]).max())
    RC.run(gpu, eng, c, pool_bytes=end - 1, expect=RC.EINVAL)          # a blob past pool_bytes
    RC.run(gpu, eng, c, pool_bytes=end, expect=RC.OK)
    RC.run(gpu, eng, c, verify=True, pool_bytes=end + 255, expect=RC.EINVAL)   # no slack
    RC.run(gpu, eng, c, verify=True, pool_bytes=end + 256, expect=RC.OK)
    # verify with a blob at offset 8 (its bytes moved there, so only the alignment is wrong)
    blobs = c["blobs"].copy()
    pool = c["pool"].copy()
    last = len(blobs) - 1
    o, n = int(blobs[last]["off"]), int(blobs[last]["len"])
    pool[o + 8:o + 8 + n] = c["pool"][o:o + n]
    blobs[last]["off"] = o + 8
    assert (o + 8) % 16 == 8
    d = dict(c, pool=pool, blobs=blobs)
    RC.run(gpu, eng, d, verify=True, expect=RC.EINVAL)
    rc, info, out = RC.run(gpu, eng, d, verify=False, expect=RC.OK)
    RC.check_streams(c, out)


def test_null_pointers(gpu, eng):
    c = RC.small_valid()
    L = gpu.lib()
    buf = gpu.DeviceBuffer(4096)
    try:
        oo = np.asarray(c["out_off"], dtype=np.uint64)
        ol = np.asarray(c["out_len"], dtype=np.uint64)
        args = [eng.h, buf.ptr, 1024, c["blobs"].ctypes.data, len(c["blobs"]),
                c["recs"].ctypes.data, len(c["recs"]), buf.ptr + 2048, 1024,
                oo.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                ol.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 3, 0, None]
        for k in (0, 1, 3, 5, 7, 9, 10):
            a = list(args)
            a[k] = None
            assert L.bsg_engine_restore(*a) == RC.EINVAL, k
        a = list(args)
        a[12] = 2  # an unknown flag
        assert L.bsg_engine_restore(*a) == RC.EINVAL
        # nothing to do is not an error
        assert L.bsg_engine_restore(eng.h, None, 0, None, 0, None, 0, None, 0, None, None, 0, 0,
                                    None) == RC.OK
    finally:
        buf.free()


def test_unfinished_run(gpu, eng):
    c = RC.small_valid()
    data = np.arange(1 << 16, dtype=np.uint32).view(np.uint8)
    src = gpu.DeviceBuffer(data.size)
    src.from_host(data)
    eng.run(src.ptr, [0], [data.size], bits=8, min_size=64)
    obuf = gpu.DeviceBuffer(c["cap"])
    pbuf = gpu.DeviceBuffer(len(c["pool"]))
    try:
        obuf.from_host(np.full(c["cap"], RC.FILL, dtype=np.uint8))
        pbuf.from_host(c["pool"])
        with pytest.raises(gpu.BsgError) as ei:
            eng.restore(pbuf, c["blobs"], c["recs"], obuf, c["out_off"], c["out_len"],
                        pool_bytes=len(c["pool"]))
        assert ei.value.code == RC.ESTATE and ei.value.info["bytes"] == 0
        assert (obuf.to_host() == RC.FILL).all()
        # the layout rules still come first
        with pytest.raises(gpu.BsgError) as ei:
            eng.restore(pbuf, c["blobs"], c["recs"][:-1], obuf, c["out_off"], c["out_len"],
                        pool_bytes=len(c["pool"]))
        assert ei.value.code == RC.EINVAL
        n = eng.finish()
        assert n == len(eng.chunks()) > 1
        info = eng.restore(pbuf, c["blobs"], c["recs"], obuf, c["out_off"], c["out_len"],
                           pool_bytes=len(c["pool"]))
        assert info["bytes"] == sum(c["out_len"])
        RC.check_streams(c, obuf.to_host())
        assert len(eng.chunks()) == n  # the run's records stay
    finally:
        obuf.free()
        pbuf.free()
        src.free()
