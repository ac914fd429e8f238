"""bsg_engine_trees: split.Writer's tree and Root per stream of an engine run, built on the
device. Roots are compared with the C oracle's Writer (fold "nonempty"), node sets with the walk
from Root through py_tree_root's store: ref -> blob bytes exactly equal, heights and order as
include/bsgpu.h specifies."""
import ctypes
import hashlib

import numpy as np
import pytest

import tree_form as TF
from bs_amd.synth import splitmix_array
from conftest import load_json

pytestmark = pytest.mark.gpu


def _run(gpu, eng, streams, bits, min_size, fanout):
    """One engine run over host streams packed at 16-byte offsets; returns the device buffer."""
    off, o = [], 0
    for d in streams:
        off.append(o)
        o += (len(d) + 15) & ~15
    host = np.zeros(max(o, 16), dtype=np.uint8)
    for d, p in zip(streams, off):
        host[p:p + len(d)] = d
    buf = gpu.DeviceBuffer(host.size)
    buf.from_host(host)
    eng.run(buf.ptr, off, [len(d) for d in streams], bits=bits, min_size=min_size, fanout=fanout)
    eng.finish()
    return buf


def _per_stream(eng, nodes, counts):
    """Node records split by stream (they are stream-major), checked against the counts."""
    out, k = [], 0
    for s, c in enumerate(counts):
        part = nodes[k:k + int(c)]
        assert (part["stream"] == s).all()
        out.append(part)
        k += int(c)
    assert k == len(nodes)
    return out


def _blob(arena, nd):
    assert int(nd["blob_off"]) % 16 == 0
    return arena[int(nd["blob_off"]):int(nd["blob_off"]) + int(nd["blob_len"])].tobytes()


def _check_nodes(oracle, data, recs, fanout, root, snodes, arena):
    """One stream's listed nodes against the oracle's TreeBuilder over the same records."""
    data = bytes(data)
    pieces = [(data[int(r["offset"]):int(r["offset"]) + int(r["len"])], int(r["level"]))
              for r in recs]
    store = {}
    want_root = oracle.py_tree_root(pieces, fanout=fanout, store=store)
    assert root == want_root
    want = TF.walk(oracle, store, want_root)
    got = {}
    for nd in snodes:
        b = _blob(arena, nd)
        assert hashlib.sha256(b).digest() == nd["ref"].tobytes()
        got[nd["ref"].tobytes()] = (b, int(nd["height"]))
    assert len(got) == len(snodes)  # no blob listed twice
    assert got == want
    # order: height ascending, then stream offset ascending (the closed form's order); Root last
    _, form = TF.closed_form([(r["ref"].tobytes(), int(r["len"]), int(r["level"])) for r in recs],
                             fanout)
    assert [nd["ref"].tobytes() for nd in snodes] == [f["ref"] for f in form]
    if len(snodes):
        assert snodes[-1]["ref"].tobytes() == root
    TF.check_listing(recs, fanout, root, snodes, arena)
    return want


def _trees(eng):
    roots, counts, nodes, arena = eng.trees()
    recs, rc = eng.chunks(), eng.counts()
    starts = np.concatenate([[0], np.cumsum(rc)]).astype(np.int64)
    per = [recs[starts[s]:starts[s + 1]] for s in range(len(rc))]
    return roots, counts, _per_stream(eng, nodes, counts), arena, per


def test_fixture_streams(gpu, oracle, table):
    """tree_root_variants.json: the last chunk closing a level while higher levels wait, 3- and
    4-level trees, the single-child prune. Each parameter set's streams in one run."""
    cases = load_json("tree_root_variants.json")["cases"]
    assert sorted(c["length"] for c in cases) == [820, 979, 9107, 187986, 5022232]
    groups = {}
    for c in cases:
        assert c["generator"] == "splitmix64" and c["seed"] == 1
        groups.setdefault((c["bits"], c["min_size"], c["fanout"]), []).append(c)
    assert sorted(groups) == [(4, 64, 2), (4, 1024, 8), (6, 64, 3)]
    eng = gpu.Engine()
    try:
        for (bits, mn, fan), cs in sorted(groups.items()):
            data = [splitmix_array(1, c["length"]) for c in cs]
            buf = _run(gpu, eng, data, bits, mn, fan)
            roots, counts, snodes, arena, per = _trees(eng)
            for s, c in enumerate(cs):
                assert roots[s].tobytes().hex() == c["root_nonempty"], c["name"]
                if c["length"] <= 200_000:
                    want = _check_nodes(oracle, data[s], per[s], fan, roots[s].tobytes(),
                                        snodes[s], arena)
                    assert 1 + max(h for _, h in want.values()) <= c["tree_levels"]
            buf.free()
    finally:
        eng.close()


EDGE_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097, 65_535, 65_537, 131_079, 300_000]


@pytest.mark.parametrize("bits,mn,fan", [(4, 64, 2), (16, 1024, 8)])
def test_edge_lengths_one_batch(gpu, oracle, table, bits, mn, fan):
    data = [splitmix_array(seed, n) for seed in (3, 11, 29) for n in EDGE_LENS]
    assert len(data) == 42
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, data, bits, mn, fan)
        roots, counts, snodes, arena, per = _trees(eng)
        for s, d in enumerate(data):
            want, _ = oracle.writer_root(table, d, bits=bits, min_size=mn, fanout=fan)
            assert roots[s].tobytes() == want, (s, len(d))
            if len(d) == 0:
                assert want == bytes(32) and counts[s] == 0
            if len(d) <= 65_536:
                _check_nodes(oracle, d, per[s], fan, want, snodes[s], arena)
            if len(per[s]) == 1:  # one chunk: a node with one leaf and no offset field
                assert counts[s] == 1 and snodes[s][0]["height"] == 0
                ref = per[s][0]["ref"].tobytes()
                assert _blob(arena, snodes[s][0]) == \
                    b"\x12\x22\x0a\x20" + ref + b"\x20" + TF.varint(len(d))
        buf.free()
    finally:
        eng.close()


def test_deep_tree(gpu, oracle, table):
    d = splitmix_array(5, 64 << 10)
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, [d], 2, 64, 1)
        roots, counts, snodes, arena, per = _trees(eng)
        want = _check_nodes(oracle, d, per[0], 1, roots[0].tobytes(), snodes[0], arena)
        assert 1 + max(h for _, h in want.values()) >= 8
        assert roots[0].tobytes() == oracle.writer_root(table, d, bits=2, min_size=64, fanout=1)[0]
        buf.free()
    finally:
        eng.close()


def test_uniform_tree_after_rerun(gpu, oracle, table):
    """256 KiB of zeros: every chunk 1,024 bytes at level 16, every chunk closes heights 0 and 1;
    the candidates (one per byte) overflow the estimate and finish() re-runs the run."""
    d = np.zeros(256 << 10, dtype=np.uint8)
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, [d], 16, 1024, 8)
        assert eng.candidates > 1 << 16  # past the first run's candidate capacity
        roots, counts, snodes, arena, per = _trees(eng)
        assert len(per[0]) == 256 and (per[0]["len"] == 1024).all() and (per[0]["level"] == 16).all()
        assert roots[0].tobytes() == oracle.writer_root(table, d)[0]
        _check_nodes(oracle, d, per[0], 8, roots[0].tobytes(), snodes[0], arena)
        assert [int((snodes[0]["height"] == h).sum()) for h in range(3)] == [256, 256, 1]
        buf.free()
    finally:
        eng.close()


def test_one_wide_node(gpu, oracle, table):
    d = splitmix_array(9, 2 << 20)
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, [d], 4, 64, 1000)
        roots, counts, snodes, arena, per = _trees(eng)
        assert len(snodes[0]) == 1 and counts[0] == 1
        blob = _blob(arena, snodes[0][0])
        assert len(blob) > 300_000
        leaves = [(r["ref"].tobytes(), int(r["offset"])) for r in per[0]]
        assert blob == TF.node_blob([], leaves, 0, len(d))
        assert roots[0].tobytes() == hashlib.sha256(blob).digest()
        assert roots[0].tobytes() == \
            oracle.writer_root(table, d, bits=4, min_size=64, fanout=1000)[0]
        buf.free()
    finally:
        eng.close()


def test_past_2_28(gpu, oracle, table):
    """One 320 MiB stream at the defaults: 5-byte varint offsets, a run with early chains."""
    n = 320 << 20
    buf = gpu.DeviceBuffer(n)
    eng = gpu.Engine()
    try:
        gpu.fill_splitmix(buf.ptr, n, 77)
        gpu.synchronize()
        eng.run(buf.ptr, [0], [n])
        eng.finish()
        roots, counts, nodes, arena = eng.trees()
        assert int(counts[0]) == len(nodes) >= 2
        d = buf.to_host()
        assert roots[0].tobytes() == oracle.writer_root(table, d)[0]
        assert nodes[-1]["ref"].tobytes() == roots[0].tobytes()
    finally:
        eng.close()
        buf.free()


def test_engine_reuse_and_states(gpu, oracle, table):
    L = gpu.lib()
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    eng = gpu.Engine()
    try:
        assert L.bsg_engine_trees(eng.h, ctypes.byref(nn), ctypes.byref(nb)) == -71  # no run yet
        assert L.bsg_engine_trees(eng.h, None, ctypes.byref(nb)) == -22
        a = [splitmix_array(s, n) for s, n in ((1, 70_000), (2, 0), (3, 5_000))]
        buf_a = _run(gpu, eng, a, 6, 64, 2)
        first = eng.trees()
        again = eng.trees()  # twice on one run: identical output
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()
        for s, d in enumerate(a):
            assert first[0][s].tobytes() == \
                oracle.writer_root(table, d, bits=6, min_size=64, fanout=2)[0]
        # caps below the totals: no more than asked is written, still BSG_OK
        nodes, arena = first[2], first[3]
        assert len(nodes) >= 4 and len(arena) >= 64
        out = np.full(len(nodes) * 56, 0xEE, dtype=np.uint8)
        ar = np.full(len(arena), 0xEE, dtype=np.uint8)
        assert L.bsg_engine_copy_tree_nodes(eng.h, out.ctypes.data, 2, ar.ctypes.data, 48) == 0
        assert out[:112].tobytes() == nodes[:2].tobytes() and (out[112:] == 0xEE).all()
        assert ar[:48].tobytes() == arena[:48].tobytes() and (ar[48:] == 0xEE).all()

        b = [splitmix_array(40 + s, 3_000 + 977 * s) for s in range(7)]  # other parameters, count
        buf_b = _run(gpu, eng, b, 5, 128, 3)
        roots = eng.trees()[0]
        for s, d in enumerate(b):
            assert roots[s].tobytes() == \
                oracle.writer_root(table, d, bits=5, min_size=128, fanout=3)[0]

        eng.hash(buf_b.ptr, [0], [3_000])
        eng.finish()
        assert L.bsg_engine_trees(eng.h, ctypes.byref(nn), ctypes.byref(nb)) == -71  # a hash run
        r = np.zeros(32 * 7, dtype=np.uint8)
        assert L.bsg_engine_copy_roots(eng.h, r.ctypes.data, None, 7) == -71

        # the engine is unharmed: a plain run's records still equal the oracle's
        buf_c = _run(gpu, eng, a, 16, 1024, 8)
        recs, rc = eng.chunks(), eng.counts()
        k = 0
        for s, d in enumerate(a):
            want = oracle.split(table, d)
            got = recs[k:k + int(rc[s])]
            assert len(got) == len(want)
            for f in ("offset", "len", "level", "ref"):
                assert (got[f] == want[f]).all()
            k += int(rc[s])
        for x in (buf_a, buf_b, buf_c):
            x.free()
    finally:
        eng.close()


def test_many_small_streams(gpu, oracle, table):
    """3,000 streams of 2-6 KiB: past the 2,047-stream LDS cache of the scan."""
    rng = np.random.default_rng(8)
    lens = rng.integers(2 << 10, (6 << 10) + 1, 3000)
    data = [splitmix_array(1000 + s, int(n)) for s, n in enumerate(lens)]
    eng = gpu.Engine()
    try:
        buf = _run(gpu, eng, data, 8, 64, 2)
        roots, counts, nodes, arena = eng.trees()
        assert int(counts.sum()) == len(nodes) and (counts >= 1).all()
        for s, d in enumerate(data):
            assert roots[s].tobytes() == \
                oracle.writer_root(table, d, bits=8, min_size=64, fanout=2)[0], s
        buf.free()
    finally:
        eng.close()
