"""The layering of csrc/: a translation unit sees only the kernels it launches, and the CPU probes of the sizing functions see none.

A non-template `inline __global__` function is compiled into the device code of every unit that includes its header, launched or not
("Header map").  Which file includes which is the whole mechanism, so this asks the preprocessor (`hipcc --cuda-host-only -MM`
with the library's flags: no code is generated, well under a second per file) for the dependency lists.  No GPU."""

import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join("tscode_amd", "csrc")

# the headers of the prune's pair kernels and pass machinery: what a unit that has nothing to do with the prune must not depend on
PRUNE_HEADERS = ["pair_stages.hpp", "pass_state.hpp", "rmsd.hpp", "rmsd_tile.hpp", "sieve.hpp", "mm.hpp", "mm_record.hpp", "cull.hpp", "cull_mm.hpp",
                 "local_pass.hpp", "descriptor.hpp", "descriptor_kernels.hpp", "descriptor_basis.hpp", "describe.hpp", "sample_moments.hpp",
                 "pass_plan.hpp", "prune_host.hpp", "prune_api.hpp", "shapes.hpp"]


def _dependencies(source):
    from tscode_amd.build import CFLAGS, _hipcc
    out = subprocess.run([_hipcc()] + CFLAGS + ["--cuda-host-only", "-MM", source], check=True, cwd=ROOT, capture_output=True, text=True).stdout
    words = out.replace("\\\n", " ").split()[1:]
    return sorted({os.path.normpath(w) for w in words if not os.path.isabs(w)} - {os.path.normpath(source)})


@pytest.mark.parametrize("unit", ["topology.hip", "nci.hip", "orbitals.hip", "torsions.hip", "xchg.hip"])
def test_units_outside_the_prune_depend_on_none_of_its_headers(unit):
    deps = _dependencies(os.path.join(CSRC, unit))
    assert os.path.join(CSRC, "host.hpp") in deps, deps
    for name in PRUNE_HEADERS:
        assert os.path.exists(os.path.join(ROOT, CSRC, name)), f"{name}: listed here, gone from csrc/"
    assert not {os.path.basename(d) for d in deps} & set(PRUNE_HEADERS), deps


@pytest.mark.parametrize("probe", ["pass_plan_check.cpp", "prune_batch_plan_check.cpp"])
def test_plan_probes_include_no_header_that_defines_a_kernel(probe):
    deps = _dependencies(os.path.join("tools", "probe", probe))
    assert os.path.join(CSRC, "pass_plan.hpp") in deps and os.path.join(CSRC, "shapes.hpp") in deps, deps
    with_kernels = [d for d in deps if "__global__" in open(os.path.join(ROOT, d)).read()]
    assert not with_kernels, with_kernels
