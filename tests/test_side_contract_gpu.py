"""The contract of the run-time libraries on the MI355X: a side library the Net runtime routes layers to is opened at the first Reshape that
needs it and not before, and a tree without it refuses that Reshape and names the file.  One case per routed library, each in fresh child
processes (tests/side_missing_child.py holds the nets: one layer on an 8-channel 8x8 input at batch 1)."""
import glob
import os
import shutil
import subprocess
import sys

import pytest

import side_contract
import side_missing_child
from feathercnn_amd import _lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240


def test_every_routed_library_has_a_case():
    assert set(side_missing_child.NETS) == {n for n, row in _lib.LIBRARIES.items() if row.route}


@pytest.mark.parametrize("name", list(side_missing_child.NETS))
def test_missing_library_is_an_error_at_reshape(cuda, tmp_path, name):
    """The tree's libraries in a directory without libfeather_<name>.so: a net that does not need it runs and never maps it -- with the
    library's switch on --, one that needs it fails at its first Reshape with FHIP_E_UNSUPPORTED and a message that names the missing file,
    and still nothing is mapped.  With the whole tree the same nets run, and the library is mapped from the first of them on."""
    missing = _lib.path(name)
    libs = glob.glob(os.path.join(os.path.dirname(_lib.lib_path()), "libfeather_*.so"))
    assert missing in libs and len(libs) >= len(_lib.LIBRARIES)
    for f in libs:
        if f != missing:
            shutil.copy(f, tmp_path / os.path.basename(f))
    needing = list(side_missing_child.NETS[name][2])
    for without in (True, False):
        env = dict(os.environ, PYTHONPATH=side_contract.ROOT)
        if without:
            env["FEATHER_HIP_LIB"] = str(tmp_path / os.path.basename(_lib.lib_path()))
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(HERE, "side_missing_child.py"), name],
                           capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in ["plain"] + needing}
        assert lines["plain"] == "plain ran unmapped", r.stdout  # the switch alone opens nothing
        for tag in needing:
            if without:
                assert lines[tag].startswith(tag + " refused:") and os.path.basename(missing) in lines[tag] and "code -1" in lines[tag], r.stdout
                assert lines[tag].endswith(" unmapped"), r.stdout
            else:
                assert lines[tag] == f"{tag} ran mapped", r.stdout
