"""The build's file lists against the source directory: every translation unit is compiled exactly once, and every header counts in the
staleness test (a header that does not would leave old objects linked into a library that then gets tested).  File names only."""
import os

from cremage_amd import build


def _csrc(suffix):
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith(suffix))


def test_every_hip_source_is_built_exactly_once():
    assert sorted(build.SOURCES) == _csrc(".hip")
    assert len(set(build.SOURCES)) == len(build.SOURCES)


def test_every_header_is_in_the_staleness_test():
    watched = {os.path.realpath(h) for h in build.HEADERS}
    for h in _csrc(".h"):
        assert os.path.realpath(os.path.join(build.CSRC, h)) in watched, h
    assert os.path.realpath(os.path.join(build.HERE, "..", "include", "crg_hip.h")) in watched
    assert all(os.path.isfile(h) for h in build.HEADERS)


def test_special_flags_name_existing_sources():
    assert set(build.EXTRA_FLAGS) <= set(build.SOURCES)
    assert build.BUDGET_CHECKED <= set(build.SOURCES)
