"""The per-conformer code of csrc/orbitals.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, against the fixtures.

    python tools/orbitals_host_check.py [--keep DIR]

Builds tools/probe/orbitals_host_check.cpp (a stand-alone program with its own main; hipcc, host code with -fsanitize=address,undefined)
and runs it on every G23 case with suprafacial off and on, on the cases of tests/test_orbitals.py that no fixture reaches, on swept
molecules of 5, 64 and 200 atoms, on propenal with the sigmatropic override and with four reactive atoms.  Every run must end clean and
its output must equal the NumPy restatement of tests/test_orbitals.py: discrete outputs exactly, coordinates to 1e-9 A.  Needs no GPU:
the recipes come from tscode_amd.reactive_atoms.orbital_recipes, which does not load the library."""

import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_orbitals as T  # noqa: E402  (the restatement and the inputs; NumPy only)

from tscode_amd.build import _hipcc  # noqa: E402
from tscode_amd.reactive_atoms import orbital_recipes  # noqa: E402


def run(exe, work, x, host, suprafacial):
    x = np.ascontiguousarray(x, dtype=np.float64)
    C, n = x.shape[:2]
    rec = host["recipes"]
    R = len(rec)
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<qiiii", C, n, R, host["sigmatropic_mode"], int(suprafacial)))
        f.write(rec.tobytes())
        f.write(x.tobytes())
    subprocess.run([exe, src, dst], check=True)
    raw = np.fromfile(dst, dtype=np.uint8)
    shapes = [("centers", (C, R, 4, 3), np.float64), ("orb_vecs", (C, R, 4, 3), np.float64), ("n_lobes", (C, R), np.uint8), ("kind", (C, R), np.uint8),
              ("sigmatropic", (C,), np.uint8)]
    if R <= 2:
        shapes += [("pivot", (C, 16, 3), np.float64), ("meanpoint", (C, 16, 3), np.float64), ("lobe_index", (C, 16, 2), np.int8), ("n_pivots", (C,), np.uint8)]
    out, pos = {}, 0
    for name, shape, dtype in shapes:
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = raw[pos:pos + size].view(dtype).reshape(shape)
        pos += size
    assert pos == len(raw), "the program wrote another number of bytes than the header documents"
    out["sigmatropic"] = out["sigmatropic"].astype(bool)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the program and its files (default: a temporary one)")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="orbitals_host_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "orbitals_host_check")
    subprocess.run([_hipcc(), "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "probe", "orbitals_host_check.cpp")], check=True, cwd=ROOT)
    done = 0
    for case in T.CASES:
        g = T.g23(case)
        opts = T.case_options(g)
        host = orbital_recipes(g.atomnos, g.reactive, g.edges, orb_dim=opts["orb_dim"], leaving_group=opts["leaving_group"], sp_seed=g.seed)
        for supra in (False, True):
            T.assert_equal_outputs(run(exe, work, g.coords, host, supra), T.restated(case, supra))
            done += 1
    for name in T.EXTRAS:
        x = T.extra_case(name)
        T.assert_equal_outputs(run(exe, work, x["coords"], orbital_recipes(x["z"], x["reactive"], x["edges"], **x["product"]), False), x["expect"])
        done += 1
    for n in T.SWEEP_N:
        for case in T.SWEEP_MOLS[n]:
            for supra in (False, True):
                x, z, edges, reactive, e, reps = T.sweep_input(case, n, 300, supra)
                host = orbital_recipes(z, reactive, edges, sp_seed=T.sweep_core(case)["seed"])
                T.assert_equal_outputs(run(exe, work, x, host, supra), T.tiled(e, reps, 300))
                done += 1
    g = T.g23("propenal")
    host = orbital_recipes(g.atomnos, g.reactive, g.edges, sigmatropic=True)
    T.assert_equal_outputs(run(exe, work, g.coords, host, False), T.restate(g.coords, g.atomnos, g.edges, g.reactive, sigmatropic=True))
    host = orbital_recipes(g.atomnos, [0, 1, 2, 3], g.edges)
    T.assert_equal_outputs(run(exe, work, g.coords, host, False), T.restate(g.coords, g.atomnos, g.edges, [0, 1, 2, 3]), pivots=False)
    print(f"orbitals_host_check: {done + 2} runs equal the restatement, every one clean under ASan and UBSan ({exe})")


if __name__ == "__main__":
    main()
