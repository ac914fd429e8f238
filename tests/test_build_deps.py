"""bs_amd.build._stale(): the library's dependencies are what its sources #include, found by
scanning them, so a regenerated .inc or an edited header rebuilds libbsgpu.so. Nothing is
compiled or touched here: the modification times are faked."""
import os
import re

import pytest

from bs_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reached() -> set:
    """Files reached from B.SOURCES through quoted includes (this test's own scan)."""
    todo = {os.path.join(B.CSRC, f) for f in B.SOURCES}
    seen = set()
    while todo:
        path = os.path.realpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for line in open(path, encoding="utf-8", errors="replace"):
            m = re.match(r'\s*#\s*include\s*"([^"]+)"', line)
            if m:
                todo.add(os.path.join(os.path.dirname(path), m.group(1)))
    return seen


DEPS = sorted(_reached())
LIB_TIME = 1_000_000.0


@pytest.fixture
def consulted(monkeypatch):
    """Fakes the library (present, LIB_TIME old) and every file's mtime (older, except those in
    the returned dict's "newer"); records the files whose time was asked for."""
    state = {"asked": set(), "newer": set()}
    real_exists = os.path.exists

    def getmtime(path):
        path = os.path.realpath(path)
        if path == os.path.realpath(B.LIB):
            return LIB_TIME
        state["asked"].add(path)
        return LIB_TIME + 1 if path in state["newer"] else LIB_TIME - 1

    monkeypatch.setattr(os.path, "getmtime", getmtime)
    monkeypatch.setattr(os.path, "exists", lambda p: p == B.LIB or real_exists(p))
    return state


def test_stale_consults_what_the_sources_include(consulted):
    assert B._stale() is False                         # nothing newer than the library
    assert consulted["asked"] == set(DEPS)
    names = {os.path.relpath(d, ROOT) for d in DEPS}
    assert {os.path.join("bs_amd", "csrc", f) for f in B.SOURCES} <= names
    for want in ("bs_amd/csrc/scan_block_loop.inc", "bs_amd/csrc/sha256_oct_solo_loop.inc",
                 "include/bsgpu.h"):
        assert want in names, want


@pytest.mark.parametrize("dep", DEPS, ids=[os.path.basename(d) for d in DEPS])
def test_stale_when_one_dependency_is_newer(consulted, dep):
    consulted["newer"] = {dep}
    assert B._stale() is True
