"""CPU tests of the energy diagnostics (bh_energy, bh_download_potential): the ABI surface, and the fp64 reference the
GPU tests (tests/test_gpu_energy.py) hold the potentials to — checked here against a direct sum and against the
oracle's own fp64 walk, so that the yardstick is known to be right before anything is measured with it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import oracle_pipeline
from potential_ref import direct_potential_f64, potential_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bh_energy", "bh_download_potential")


def test_new_symbols_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bh.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bh_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(pkg.LIB_PATH)
    bound = {s[0] for s in __import__("nbody_barnes_hut_cuda_amd")._lib.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound
        assert hasattr(raw, name), name


def test_energy_stats_layout_matches_the_c_compiler(pkg, tmp_path):
    L = __import__("nbody_barnes_hut_cuda_amd")._lib
    src = tmp_path / "sz.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include <stddef.h>', '#include "bh.h"', "int main(void) {",
        '  printf("size %zu\\n", sizeof(bh_energy_stats));',
        '  printf("potential %zu\\n", offsetof(bh_energy_stats, potential));',
        '  printf("angular_momentum %zu\\n", offsetof(bh_energy_stats, angular_momentum));',
        '  printf("com %zu\\n", offsetof(bh_energy_stats, com));',
        '  printf("n %zu\\n", offsetof(bh_energy_stats, n));',
        '  printf("params %zu\\n", sizeof(bh_params));',
        '  printf("stats %zu\\n", sizeof(bh_stats));',
        "  return 0; }"]))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    E = L.BhEnergyStats
    assert int(out["size"]) == C.sizeof(E) == 13 * 8 + 8 * 4
    assert int(out["potential"]) == E.potential.offset
    assert int(out["angular_momentum"]) == E.angular_momentum.offset
    assert int(out["com"]) == E.com.offset
    assert int(out["n"]) == E.n.offset
    # additive change: the existing structs keep their sizes, the ABI version stays
    assert int(out["params"]) == C.sizeof(L.BhParams) and int(out["stats"]) == C.sizeof(L.BhStats)
    assert L.lib.bh_abi_version() == 6


def test_null_context_is_a_bad_argument(pkg):
    L = __import__("nbody_barnes_hut_cuda_amd")._lib
    st = L.BhEnergyStats()
    phi = np.zeros(4, np.float32)
    assert L.lib.bh_energy(None, C.byref(st)) == -1
    assert L.lib.bh_energy(None, None) == -1
    assert L.lib.bh_download_potential(None, phi.ctypes.data_as(L._F)) == -1


def _ic(pkg, n, seed=7):
    return pkg.plummer(n, seed=seed)


def _tree(orc, ic, **kw):
    p = orc.params(**kw)
    return oracle_pipeline(orc, ic, p), p


def test_reference_walk_at_theta_0_is_the_direct_sum(pkg, orc):
    """theta = 0 opens every cell: the walk must add exactly the direct sum's terms (1e-12 relative: fp64 sums in
    different orders)"""
    n = 3000
    ic = _ic(pkg, n)
    for kw in (dict(), dict(leaf_cap=4, max_depth=3)):
        t, p = _tree(orc, ic, theta=0.0, **kw)
        xyzm = t["xyzm"]
        ref = potential_f64(t["rec"], xyzm, p.G, 0.0, p.eps2)
        phi, sabs, k = direct_potential_f64(xyzm[:, 0], xyzm[:, 1], xyzm[:, 2], xyzm[:, 3], p.G, p.eps2)
        rel = np.abs(ref["phi"] - phi) / np.abs(phi)
        assert rel.max() <= 1e-12, (kw, rel.max())
        assert (ref["k"] == k).all(), kw
        assert np.allclose(ref["sabs"], sabs, rtol=1e-12, atol=0)


@pytest.mark.parametrize("theta", [0.5, 1.0])
@pytest.mark.parametrize("kw", [dict(), dict(key_curve=1), dict(leaf_cap=4, max_depth=3)])
def test_reference_walk_takes_the_oracle_walks_interactions(pkg, orc, theta, kw):
    """per body, the walk takes as many terms as oracle.force_f64 (the fp64 force walk of the same tree) wherever the
    MAC is not a tie, and finds the same MAC margin"""
    n = 6000
    ic = _ic(pkg, n, seed=11)
    t, p = _tree(orc, ic, theta=theta, **kw)
    ref = potential_f64(t["rec"], t["xyzm"], p.G, theta, p.eps2)
    f = orc.force_f64(t["rec"], t["xyzm"], p)
    tie = f["margin"] < 1e-5
    assert tie.mean() < 0.05
    assert (ref["k"][~tie] == f["k"][~tie]).all()
    assert np.allclose(ref["margin"], f["margin"], rtol=1e-9, atol=0)
    assert (ref["k"] < n).all() and (ref["phi"] < 0).all()


def test_reference_walk_samples_agree_with_the_whole_walk(pkg, orc):
    """a sampled walk (idx, as the large GPU cases use) gives the rows of the whole walk"""
    n = 4000
    t, p = _tree(orc, _ic(pkg, n, seed=3), theta=0.5)
    whole = potential_f64(t["rec"], t["xyzm"], p.G, 0.5, p.eps2)
    idx = np.arange(5, n, 37)
    part = potential_f64(t["rec"], t["xyzm"], p.G, 0.5, p.eps2, idx=idx, chunk=17)
    assert np.array_equal(part["k"], whole["k"][idx])
    assert np.allclose(part["phi"], whole["phi"][idx], rtol=1e-13, atol=0)
