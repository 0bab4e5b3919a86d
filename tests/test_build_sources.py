"""The build recipe's file lists against the directory (no GPU, no build): a unit missing from SOURCES is not linked, and a
header missing from HEADERS leaves stale objects behind when it changes."""
import os

import slam.net_amd.build as b


def test_sources_are_the_hip_files():
    assert len(b.SOURCES) == len(set(b.SOURCES))
    assert set(b.SOURCES) == {f for f in os.listdir(b.CSRC) if f.endswith(".hip")}


def test_every_other_file_is_a_header():
    others = {f for f in os.listdir(b.CSRC) if not f.endswith(".hip")}
    assert others and others <= set(b.HEADERS)
    assert all(os.path.isfile(os.path.join(b.CSRC, h)) for h in b.HEADERS)
    assert any(os.path.basename(h) == "slamhip.h" for h in b.HEADERS)
