"""The build script knows every source: no file under minbft_amd/csrc can
change without the library being rebuilt, and no unit can be left out of it."""
import os

from minbft_amd import build


def test_every_source_is_a_build_input():
    files = sorted(f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp", ".h", ".inc")))
    assert files
    inputs = {os.path.normpath(p) for p in build._inputs()}
    orphans = [f for f in files if os.path.normpath(os.path.join(build.CSRC, f)) not in inputs]
    assert orphans == [], f"not an input of build.up_to_date(): {orphans}"
    assert sorted(f for f in files if f.endswith(".hip")) == sorted(build.DEVICE_SOURCES)
    assert sorted(f for f in files if f.endswith(".cpp")) == sorted(build.HOST_SOURCES)
