"""The instantiation list read from the shipped library (tests/kernel_instances.py) and the sweep table (tests/instance_cases.py) agree."""
import os
import re
import subprocess
import tempfile

import pytest

import kernel_instances as KI
import side_contract
from instance_cases import CASES, EXCLUDED
from test_guarded_cpu import EXCLUDED_REASON_MIN, _kernels

LLVM = "/opt/rocm/llvm/bin"


@pytest.fixture(scope="module")
def names():
    if not os.path.exists(KI.LIB):
        pytest.fail(f"{KI.LIB} is missing: run build() first")
    return KI.instances()


def test_list_parses(names):
    assert len(names) >= 150, names
    side_contract.main_library_holds(names)
    for n in names:
        assert not n.startswith("void ") and "(" not in n, n


def test_normalise():
    assert KI.normalise("void fhip::k<8, true>(float const*, int)") == "fhip::k<8, true>"
    assert KI.normalise("void fhip::g<fhip::S<1, 2>, fhip::P<3, false> >(fhip::Q)") == "fhip::g<fhip::S<1, 2>, fhip::P<3, false> >"
    assert KI.base("fhip::stream_gemm_kernel<8, true, false, true>") == "stream_gemm_kernel"


def test_base_names_match_the_source_scan(names):
    assert {KI.base(n) for n in names} == _kernels()


def test_count_matches_llvm_readelf(names):
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.fail(f"{readelf} not found")  # only a cross-check: the list itself never needs it
    with tempfile.TemporaryDirectory() as d:
        mangled = set()
        for i, obj in enumerate(KI.code_objects()):
            p = os.path.join(d, f"co{i}.o")
            open(p, "wb").write(obj)
            out = subprocess.run([readelf, "-sW", p], capture_output=True, text=True, check=True).stdout
            mangled |= set(re.findall(r"\s(\S+)\.kd\s*$", out, re.M))
    assert len(mangled) == len(names)


def test_every_instantiation_has_a_case(names):
    targeted = {t for c in CASES for t in c.targets}
    missing = sorted(n for n in names if n not in targeted and KI.base(n) not in EXCLUDED)
    assert not missing, f"instantiations without a sweep case in tests/instance_cases.py: {missing}"
    assert all(len(why) >= EXCLUDED_REASON_MIN for why in EXCLUDED.values())
    assert set(EXCLUDED) <= {KI.base(n) for n in names}


def test_no_case_targets_a_missing_instantiation(names):
    have = set(names)
    bad = sorted({t for c in CASES for t in c.targets} - have)
    assert not bad, f"sweep cases target instantiations the library does not hold: {bad}"
    assert all(c.targets for c in CASES), [c.name for c in CASES if not c.targets]
    assert len({c.name for c in CASES}) == len(CASES)
