"""bh_energy / bh_download_potential on the GPU: the potentials against fp64 references (tests/potential_ref.py — a direct
sum at theta = 0, the fp64 walk of the context's own tree above), the walk against the force_variant = 1 force walk bit
for bit, the system sums against numpy, physics sanity on an equilibrium Plummer sphere, the run left unperturbed, the
error paths and bh_bench --energy."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import TIE_MARGIN, oparams, special_ics
from potential_ref import direct_potential_f64, phi_bound, potential_f64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = ["coincident", "collinear", "outlier", "pairs", "tiny", "grid", "zero_mass"]
# Population limits on |phi - phi_ref| / |phi_ref| of the non-tie bodies: twice the largest MI355X figure over the cases
# of this file (every check prints its figures).  Measured: median 1.44e-6 (20,000 bodies, theta 0), 99.99th percentile
# 8.21e-6 (the same); on the edge inputs at most 2.9e-7 / 1.8e-6, except the "outlier" body at 1e6, whose |phi| is ~400
# times below the self term it is corrected by (99.99th percentile 9.9e-5: still 0.034 of its per-body bound).  The
# per-body bound (potential_ref.phi_bound) was met with at most 0.18 of its allowance.
PHI_MED, PHI_P9999 = 2.9e-6, 1.7e-5
EDGE_P9999 = 2e-4
TIE_PHI_REL = 1.4e-5        # tie bodies (a cell decided the other way): measured 6.8e-6 at most (the 1e-3 cap of the
                            # issue's estimate is far above)


def _engine(pkg, ic, **kw):
    e = pkg.Engine(len(ic[0]), **kw)
    e.upload(*ic)
    return e


def _sorted_phi(e):
    return e.download_potential()[e.download_order()]


def _figures(phi, ref_phi, bound, nontie, label):
    err = np.abs(phi.astype(np.float64) - ref_phi)
    rel = err / np.abs(ref_phi)
    r = rel[nontie]
    fig = dict(ratio_max=float((err[nontie] / bound[nontie]).max()) if nontie.any() else 0.0,
               med=float(np.median(r)) if len(r) else 0.0,
               p9999=float(np.quantile(r, 0.9999)) if len(r) else 0.0,
               max=float(r.max()) if len(r) else 0.0,
               tie_max=float(rel[~nontie].max()) if (~nontie).any() else 0.0,
               tie_frac=float((~nontie).mean()))
    print(f"phi check {label}: bodies {len(phi)} ties {fig['tie_frac']:.2%} err/((k+8) u sum|t|) max "
          f"{fig['ratio_max']:.3f}  rel p50 {fig['med']:.2e} p99.99 {fig['p9999']:.2e} max {fig['max']:.2e}  "
          f"ties' rel max {fig['tie_max']:.2e}")
    return err, rel, fig


# ------------------------------------------------------------------ 1. theta = 0: the direct sum
@pytest.mark.parametrize("name,n", [(nm, 777) for nm in EDGE] + [("plummer", 4096), ("plummer", 20_000)])
def test_theta0_potential_is_the_direct_sum(pkg, name, n):
    rng = np.random.default_rng(5)
    ic = pkg.plummer(n, seed=9) if name == "plummer" else special_ics(name, n, rng)
    e = _engine(pkg, ic, theta=0.0)
    st = e.energy()
    phi = e.download_potential()
    assert e.stats().status_flags == 0
    x, y, z, vx, vy, vz, m = ic
    ref, sabs, k = direct_potential_f64(x, y, z, m, e.params.G, e.params.eps2)
    assert np.isfinite(phi).all()
    bound = phi_bound(k, sabs)
    err, rel, fig = _figures(phi, ref, bound, np.ones(n, bool), f"{name} {n} theta 0")
    assert (err <= bound).all(), (name, int((err > bound).sum()), fig)
    assert fig["med"] <= PHI_MED and fig["p9999"] <= (PHI_P9999 if name == "plummer" else EDGE_P9999), fig
    assert st["n"] == n
    e.close()


# ------------------------------------------------------------------ 2. theta > 0: the fp64 walk of the same tree
def _sample(n, every):
    if every <= 1:
        return None
    s = [np.arange(0, n, every), np.arange(0, 64), np.arange(n - 64, n)]
    return np.unique(np.concatenate(s)).astype(np.int32)


def _check_walk(orc, e, label, idx=None):
    rec = e.download_tree()
    xyzm = e.download_sorted_bodies()
    p = e.params
    phi = _sorted_phi(e)
    f = orc.force_f64(rec, xyzm, oparams(orc, p), idx=idx)
    ref = potential_f64(rec, xyzm, p.G, p.theta, p.eps2, idx=f["idx"])
    nontie = f["margin"] >= TIE_MARGIN
    assert (ref["k"][nontie] == f["k"][nontie]).all(), label
    got = phi[f["idx"]]
    assert np.isfinite(got).all(), label
    bound = phi_bound(ref["k"], ref["sabs"])
    err, rel, fig = _figures(got, ref["phi"], bound, nontie, label)
    bad = nontie & (err > bound)
    assert not bad.any(), (label, int(bad.sum()), f["idx"][bad][:8], fig)
    assert fig["tie_frac"] <= 0.05, (label, fig)
    assert fig["tie_max"] <= TIE_PHI_REL, (label, fig)
    assert fig["med"] <= PHI_MED and fig["p9999"] <= PHI_P9999, (label, fig)
    assert e.stats().status_flags == 0
    return fig


@pytest.mark.parametrize("n,every", [(65_536, 8), (300_000, 64), (1_000_000, 256)])
@pytest.mark.parametrize("theta", [0.3, 0.5, 1.0])
def test_potential_vs_f64_walk_plummer(pkg, orc, n, every, theta):
    e = _engine(pkg, pkg.plummer(n, seed=42), theta=theta)
    e.step(2)
    e.energy()
    _check_walk(orc, e, f"plummer {n} theta {theta}", _sample(n, every))
    e.close()


@pytest.mark.parametrize("kw", [dict(key_curve=0), dict(key_curve=1), dict(key_bits=30, max_depth=10),
                                dict(leaf_cap=1, max_depth=3), dict(leaf_cap=4, max_depth=3),
                                dict(leaf_cap=16, max_depth=3)])
def test_potential_vs_f64_walk_tree_shapes(pkg, orc, kw):
    n = 20_000
    e = _engine(pkg, pkg.plummer(n, seed=4), **kw)
    e.energy()
    _check_walk(orc, e, f"plummer {n} {kw}")
    e.close()


# ------------------------------------------------------------------ 3. the walk takes the force walk's records
@pytest.mark.parametrize("n", [777, 20_000, 65_536, 300_000, 1_000_000])
def test_energy_walk_is_the_force_variant_1_walk(pkg, n):
    """bh_energy's accelerations equal bit for bit those of bh_force on a force_variant = 1, force_coop = 1 context at
    the same state (same tree: bh_energy does not move the bodies, and the stages re-sort them stably by the same
    keys); a default context's bh_energy from the same upload gives the same bits, accelerations and potentials"""
    ic = pkg.plummer(n, seed=21)
    e = _engine(pkg, ic, force_variant=1, force_coop=1)
    e.energy()
    a_e = np.stack(e.download_acc(), 1)
    phi = e.download_potential()
    e.tree_stages()
    e.force()
    a_f = np.stack(e.download_acc(), 1)
    assert np.isfinite(a_e).all()
    assert np.array_equal(a_e.view(np.uint32), a_f.view(np.uint32)), int((a_e != a_f).any(1).sum())
    assert e.stats().status_flags == 0
    e.close()
    d = _engine(pkg, ic)
    d.energy()
    assert np.array_equal(np.stack(d.download_acc(), 1).view(np.uint32), a_e.view(np.uint32))
    assert np.array_equal(d.download_potential().view(np.uint32), phi.view(np.uint32))
    d.close()


# ------------------------------------------------------------------ 4. the system sums
def test_energy_totals_against_numpy(pkg):
    n = 65_536
    e = _engine(pkg, pkg.plummer(n, seed=8))
    e.step(3)
    st = e.energy()
    st2 = e.energy()
    assert st == st2  # the same state: the same bits (fixed-order reduction, no float atomics)
    x, y, z, vx, vy, vz = (a.astype(np.float64) for a in e.download())
    m = e.download_mass().astype(np.float64)
    phi = e.download_potential().astype(np.float64)
    K = 0.5 * np.sum(m * (vx * vx + vy * vy + vz * vz))
    W = 0.5 * np.sum(m * phi)
    M = m.sum()
    P = np.array([np.sum(m * vx), np.sum(m * vy), np.sum(m * vz)])
    X = np.stack([x, y, z], 1)
    V = np.stack([vx, vy, vz], 1)
    L = (m[:, None] * np.cross(X, V)).sum(0)
    com = (m[:, None] * X).sum(0) / M
    for got, want in ((st["kinetic"], K), (st["potential"], W), (st["mass"], M)):
        assert abs(got - want) <= 1e-11 * abs(want), (got, want)
    assert st["total"] == st["kinetic"] + st["potential"]
    sv = np.sum(m * np.linalg.norm(V, axis=1))
    sl = np.sum(m * np.linalg.norm(X, axis=1) * np.linalg.norm(V, axis=1))
    assert np.abs(np.array(st["momentum"]) - P).max() <= 1e-12 * sv
    assert np.abs(np.array(st["angular_momentum"]) - L).max() <= 1e-12 * sl
    assert np.abs(np.array(st["com"]) - com).max() <= 1e-12 * np.abs(X).max()
    assert st["n"] == n and e.stats().status_flags == 0
    e.close()


# ------------------------------------------------------------------ 5. physics: an equilibrium Plummer sphere
def test_plummer_sphere_is_virialised(pkg):
    """pkg.plummer(a = 400, G = 0.5) is in equilibrium: 2K = |W|, and W = -3 pi G M^2 / (32 a).  Measured on MI355X
    (seed 42, theta 0.5, eps2 50): 2K / |W| = 0.9904, W / W_plummer = 1.0240 (a finite sample of the sphere); bounds
    0.02 and 0.05 — a missing 1/2 or G, or a dropped self correction, is off by far more"""
    n, a, G = 65_536, 400.0, 0.5
    e = _engine(pkg, pkg.plummer(n, seed=42, a=a, G=G), G=G)
    st = e.energy()
    W0 = -3 * math.pi * G * st["mass"] ** 2 / (32 * a)
    vir = 2 * st["kinetic"] / abs(st["potential"])
    print(f"plummer {n}: 2K/|W| = {vir:.4f}  W / W_plummer = {st['potential'] / W0:.4f}")
    assert abs(vir - 1) <= 0.02, vir
    assert abs(st["potential"] / W0 - 1) <= 0.05, st["potential"] / W0
    e.close()


# ------------------------------------------------------------------ 6. no perturbation
def _run(pkg, ic, kw, timing, energy_after):
    e = _engine(pkg, ic, **kw)
    if timing:
        e.set_timing(timing)
    for s in range(1, 13):
        e.step()
        if s in energy_after:
            e.energy()
    out = [np.stack(e.download(), 1), np.stack(e.download_acc(), 1)]
    steps = e.stats().steps
    assert e.stats().status_flags == 0
    e.close()
    return out, steps


@pytest.mark.parametrize("n,kw,timing", [
    (4_096, dict(), 0),
    (4_096, dict(key_curve=0, step_graph=1), 0),
    (125_000, dict(key_curve=0), 1),
    (125_000, dict(step_graph=1), 0),
    (400_000, dict(), 3),
    (400_000, dict(key_curve=0, step_graph=1), 0),
    (1_000_000, dict(), 0),
    (1_000_000, dict(key_curve=0), 3),
    (1_000_000, dict(step_graph=1), 1),
    (65_536, dict(strict_fp=1), 0),
])
def test_energy_does_not_perturb_the_run(pkg, n, kw, timing):
    ic = pkg.plummer(n, seed=13)
    (s0, a0), k0 = _run(pkg, ic, kw, timing, ())
    for after in (range(1, 12), (3, 6, 9)):
        (s1, a1), k1 = _run(pkg, ic, kw, timing, after)
        assert k1 == k0 == 12
        assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32)), (kw, int((s1 != s0).any(1).sum()))
        assert np.array_equal(a1.view(np.uint32), a0.view(np.uint32)), (kw, int((a1 != a0).any(1).sum()))


# ------------------------------------------------------------------ 7. error paths
def test_energy_error_paths(pkg):
    import torch
    from nbody_barnes_hut_cuda_amd.engine import BhError
    from nbody_barnes_hut_cuda_amd._lib import BhDdSizes, lib
    import ctypes as C
    n = 4_096
    e = _engine(pkg, pkg.plummer(n, seed=1))
    with pytest.raises(BhError) as x:
        e.download_potential()
    assert x.value.status == -6
    assert e.stats().status_flags == 0
    e.energy()
    assert e.download_potential().shape == (n,)
    e.step()
    with pytest.raises(BhError) as x:
        e.download_potential()
    assert x.value.status == -6
    e.energy()
    e.download_potential()
    e.tree_stages(); e.force(); e.integrate()
    with pytest.raises(BhError) as x:
        e.download_potential()
    assert x.value.status == -6
    e.upload(*pkg.plummer(n, seed=2))
    with pytest.raises(BhError) as x:
        e.download_potential()
    assert x.value.status == -6
    assert e.stats().status_flags == 0
    e.close()
    sz = BhDdSizes()
    assert lib.bh_dd_query(50000, 4, 4096, 60000, C.byref(sz)) == 0
    pool = torch.zeros(sz.pool_records * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.Engine(50000) as d:
        d.dd_init(4, 0, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records)
        with pytest.raises(BhError) as x:
            d.energy()
        assert x.value.status == -1
        with pytest.raises(BhError) as x:
            d.download_potential()
        assert x.value.status == -6
        assert d.stats().status_flags == 0


# ------------------------------------------------------------------ 8. bh_bench --energy
LINE = re.compile(r"^energy step (\d+) K (\S+) W (\S+) E (\S+) dE/\|E0\| (\S+)$")


def _bench(*args):
    exe = os.path.join(ROOT, "nbody-barnes-hut-cuda_amd", "bh_bench")
    r = subprocess.run([exe, "--n", "65536", "--steps", "20", "--ic", "plummer", *args], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_bench_energy_lines():
    out = _bench("--energy", "5")
    lines = [LINE.match(l) for l in out if l.startswith("energy")]
    assert len(lines) == 4 and all(lines), out[-10:]
    assert [int(m.group(1)) for m in lines] == [5, 10, 15, 20]
    for m in lines:
        K, W, E, dE = (float(m.group(i)) for i in range(2, 6))
        assert all(math.isfinite(v) for v in (K, W, E, dE))
        assert K > 0 > W and abs(E - (K + W)) <= 1e-6 * abs(W) and abs(dE) < 0.1
    plain = _bench()
    assert not any(l.startswith("energy") for l in plain)
    frames = [l for l in plain if re.match(r"^\d+\s+\| [0-9.]+\s+\| [0-9.]+$", l.rstrip())]
    assert len(frames) == 20
    assert len([l for l in out if re.match(r"^\d+\s+\| [0-9.]+\s+\| [0-9.]+$", l.rstrip())]) == 20
    assert [l for l in out if not l.startswith("energy")][:4] == plain[:4]
    assert any(l.startswith("N=65536 ic=plummer") for l in plain)
