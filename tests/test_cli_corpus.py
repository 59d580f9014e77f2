"""The command lines of the analysis programs (no GPU): tests/golden/cli_corpus.json holds what every program of
2022a-genome-dynamics_amd/host answered -- exit status, stdout, stderr -- to the command lines that tests/golden/make_cli_corpus.py
expands from its tables, recorded before the programs moved onto one option scanner (host/gd_cli_args.hpp).  Every entry is
replayed and the three fields compared for equality.  No line of the corpus reaches a device or names an existing file."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

PKG = "2022a-genome-dynamics_amd"
HOST = os.path.join(ROOT, PKG, "host")
needs_h5 = pytest.mark.skipif(not os.path.exists("/opt/conda/include/hdf5.h"), reason="HDF5 C library not in this image")
GROUPS = ("FLOW", "RDF", "LAMINA", "CMAP", "HIC", "MSD", "DCORR", "DMAP")

# The one permitted change: gd_particle_flow and gd_grid_flow looked for an option's value before they looked the option up, so
# an unknown option as the last token was answered "argument --x: expected one argument".  They now answer what every sibling
# and argparse itself answer.  (program, args) -> the option named
FLOW_LAST_TOKEN = {
    ("gd_particle_flow", ("--dry-run", "--scan-radius", "1.5", "out.h5", "traj.h5", "--bogus")): "--bogus",
    ("gd_grid_flow", ("--dry-run", "--scan-radius", "1.5", "--grid-interval", "0.5", "--x-range", "-1,1", "--y-range", "-2,2", "--z-range", "0,0.5",
                      "out.h5", "traj.h5", "--bogus")): "--bogus",
}


def _corpus():
    with open(os.path.join(ROOT, "tests", "golden", "cli_corpus.json")) as f:
        return json.load(f)


def _programs_of_makefile():
    text = open(os.path.join(HOST, "Makefile")).read()
    return [p for g in GROUPS for p in re.search(rf"^{g} = (.*)$", text, flags=re.M).group(1).split()]


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-s", "-C", HOST, "h5lib/libhdf5.so", *_programs_of_makefile()])
    return HOST


def test_every_program_has_entries():
    listed = _programs_of_makefile()
    assert len(listed) == 17
    recorded = {e["program"] for e in _corpus()}
    assert recorded == set(listed)
    for key in FLOW_LAST_TOKEN:
        assert sum((e["program"], tuple(e["args"])) == key for e in _corpus()) == 1, key


@needs_h5
def test_replay(programs, tmp_path):
    wrong = []
    for e in _corpus():
        r = subprocess.run([os.path.join(programs, e["program"]), *e["args"]], capture_output=True, text=True, cwd=tmp_path, timeout=60)
        expected = dict(e)
        option = FLOW_LAST_TOKEN.get((e["program"], tuple(e["args"])))
        if option:
            was = f"argument {option}: expected one argument"
            assert e["stderr"].count(was) == 1
            expected["stderr"] = e["stderr"].replace(was, f"unrecognized arguments: {option}")
        got = {"program": e["program"], "args": e["args"], "status": r.returncode, "stdout": r.stdout, "stderr": r.stderr}
        if got != expected:
            wrong.append((expected, got))
    assert not wrong, f"{len(wrong)} of the corpus differ, the first: {wrong[0]}"
    assert os.listdir(tmp_path) == []
