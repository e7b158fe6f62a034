"""Order 2 (bh_set_multipole) on the GPU: the second moments against fp64 sums over every record's bodies, the
quadrupole walk against the fp64 quadrupole walk of the same tree (tests/quadrupole_ref.py) with helpers.check_force_f64,
the gain over monopoles against the direct sum, theta = 0, the potentials and bh_energy, reproducibility, the error
paths and bh_bench --multipole."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import check_force_f64, special_ics
from quadrupole_ref import direct_acc_f64, moments_f64, quadrupole_f64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = ["coincident", "collinear", "outlier", "pairs", "tiny", "grid", "zero_mass"]
MOM_TOL = 1e-5              # |S - S_ref| <= MOM_TOL m s^2 per cell record: a fixed requirement, not a measured limit
                            # (measured 1.4e-8 at most, the far cluster; a prefix-sum build misses it there)
# check_force_f64 limits of the order-2 walk against quadrupole_f64: at most twice the largest MI355X figure over the
# cases of this file (every check prints its figures; DESIGN.md §4 records them).  Measured on the Plummer and theta /
# eps2 cases: err / (sqrt(max(k, 48)) u sum|term|) 1.12 at most (theta 0.3, eps2 0.01; the monopole walks' F64_C = 1.8 is
# kept: below twice the figure), relative error median 9.1e-7, 99.99th percentile 1.38e-5, max 2.04e-5 (all at theta 0.3, the most terms).
QUAD_C = 1.8
QUAD_MED, QUAD_P9999, QUAD_MAX = 1.8e-6, 2.8e-5, 4.1e-5
# edge inputs and the far cluster: median 6.5e-7 (far cluster), 99.99th percentile 6.6e-4 and max 7.1e-4 (the middle of
# the collinear row, where forces cancel to ~0, as for the monopole walks)
EDGE_LIMITS = dict(tie_cap=0.05, med=1.3e-6, p9999=1.3e-3, rmax=1.4e-3)
# potentials against quadrupole_f64's phi (non-tie bodies): median 4.2e-7, 99.99th percentile 3.0e-6
PHI_MED, PHI_P9999 = 8.5e-7, 6.1e-6
# the gain against the fp64 direct sum (200,000 bodies, 2,048 sampled): order-2 / order-1 median 0.36 at theta 0.5 and
# 0.53 at theta 0.7 — at 0.7 the gain stops short of a factor of two (the MAC measures the distance to
# the centre of mass, so a cell's farthest body may lie beyond the body at theta = 0.7 and the series converges slowly)
GAIN = {0.5: 0.5, 0.7: 0.6}


def _engine(pkg, ic, order=2, **kw):
    e = pkg.Engine(len(ic[0]), **kw)
    e.upload(*ic)
    if order != 1:
        e.set_multipole(order)
    return e


def far_cluster(seed=21):
    """4,096 bodies in a unit cube at (1e4, 1e4, 1e4) plus a Plummer sphere of 60,000 (the cluster's small cells are
    where prefix sums of m x x^T about the origin cancel away)"""
    import bhpkg
    pkg = bhpkg.load()
    x, y, z, vx, vy, vz, m = pkg.plummer(60_000, seed=seed)
    rng = np.random.default_rng(seed)
    c = rng.random((4096, 3)).astype(np.float32) + np.float32(1e4)
    f = np.float32
    cat = lambda a, b: np.concatenate([a, b]).astype(f)
    return (cat(x, c[:, 0]), cat(y, c[:, 1]), cat(z, c[:, 2]), cat(vx, np.zeros(4096)), cat(vy, np.zeros(4096)),
            cat(vz, np.zeros(4096)), cat(m, (2 + 5 * rng.random(4096))))


def _sample(n, every):
    if every <= 1:
        return None
    return np.unique(np.concatenate([np.arange(0, n, every), np.arange(0, min(n, 64)), np.arange(max(0, n - 64), n)]))


# ------------------------------------------------------------------ 1. the moments
def _check_moments(e, label, every=1):
    e.tree_stages()
    assert e.multipole == 2
    rec = e.download_tree()
    S = e.download_multipoles()
    xyzm = e.download_sorted_bodies()
    assert S.shape == (len(rec), 6)
    cells = np.flatnonzero(((rec["kind"] == 1) | (rec["kind"] == 2)) & (rec["m"] > 0))
    rows = cells if every <= 1 else cells[::every]
    ref = moments_f64(rec, xyzm, rows=rows)
    scale = rec["m"][rows].astype(np.float64) * rec["s"][rows].astype(np.float64) ** 2
    err = np.abs(S[rows].astype(np.float64) - ref).max(1)
    worst = float((err / scale).max()) if len(rows) else 0.0
    print(f"moments {label}: {len(rows)} cell records, max |S - S_ref| / (m s^2) {worst:.2e}")
    assert worst <= MOM_TOL, (label, worst)
    assert (S[rec["kind"] == 0] == 0).all() and (S[rec["kind"] == 3] == 0).all()
    assert e.stats().status_flags == 0
    return worst


@pytest.mark.parametrize("n,every", [(65536, 1), (1_000_000, 37)])
def test_moments_plummer(pkg, n, every):
    e = _engine(pkg, pkg.plummer(n, seed=41))
    _check_moments(e, f"plummer n={n}", every)
    e.close()


@pytest.mark.parametrize("name", EDGE)
def test_moments_edge_inputs(pkg, name):
    ic = special_ics(name, 5000, np.random.default_rng(5))
    e = _engine(pkg, ic)
    _check_moments(e, f"edge {name}")
    e.close()


def test_moments_far_cluster(pkg):
    e = _engine(pkg, far_cluster())
    _check_moments(e, "far cluster")
    e.close()


@pytest.mark.parametrize("kw", [dict(leaf_cap=1), dict(leaf_cap=8), dict(leaf_cap=16), dict(key_curve=0),
                                dict(key_curve=1), dict(key_bits=30)])
def test_moments_trees(pkg, kw):
    e = _engine(pkg, pkg.plummer(20001, seed=42), **kw)
    _check_moments(e, f"tree {kw}")
    e.close()


# ------------------------------------------------------------------ 2. the walk against the fp64 quadrupole walk
def _acc_sorted(e):
    return np.stack(e.download_acc(), 1)[e.download_order()]


def _check_walk(e, label, idx=None, **kw):
    rec = e.download_tree()
    xyzm = e.download_sorted_bodies()
    p = e.params
    ref = quadrupole_f64(rec, xyzm, p.G, p.theta, p.eps2, idx=idx)
    acc = _acc_sorted(e)[ref["idx"]]
    assert np.isfinite(acc).all(), label
    lim = dict(C=QUAD_C, med=QUAD_MED, p9999=QUAD_P9999, rmax=QUAD_MAX)
    lim.update(kw)
    fig = check_force_f64(acc, ref, label, **lim)
    assert e.stats().status_flags == 0
    return fig, ref, acc


@pytest.mark.parametrize("n,every", [(4096, 1), (65536, 1), (250_000, 61), (1_000_000, 251)])
def test_walk_plummer_vs_f64(pkg, n, every):
    e = _engine(pkg, pkg.plummer(n, seed=43))
    e.tree_stages(); e.force()
    _check_walk(e, f"quad n={n}", _sample(n, every))
    e.close()


@pytest.mark.parametrize("theta", [0.3, 0.5, 0.7, 1.0])
@pytest.mark.parametrize("eps2", [50.0, 0.01])
def test_walk_theta_eps_vs_f64(pkg, theta, eps2):
    n = 20000
    e = _engine(pkg, pkg.plummer(n, seed=44), theta=theta, eps2=eps2)
    e.tree_stages(); e.force()
    _check_walk(e, f"quad theta={theta} eps2={eps2}")
    e.close()


@pytest.mark.parametrize("name", EDGE)
def test_walk_edge_inputs_vs_f64(pkg, name):
    ic = special_ics(name, 5000, np.random.default_rng(5))
    e = _engine(pkg, ic)
    e.tree_stages(); e.force()
    _check_walk(e, f"quad edge {name}", C=QUAD_C, **EDGE_LIMITS)
    e.close()


def test_walk_far_cluster_vs_f64(pkg):
    e = _engine(pkg, far_cluster())
    e.tree_stages(); e.force()
    _check_walk(e, "quad far cluster", _sample(64096, 7), **EDGE_LIMITS)
    e.close()


@pytest.mark.parametrize("n", [4096, 100_000])
def test_fused_step_equals_staged_stages(pkg, n):
    """bh_step's fused force + integrate launch against the stages and bh_integrate, bit for bit, three steps"""
    ic = pkg.plummer(n, seed=45)
    a = _engine(pkg, ic)
    b = _engine(pkg, ic)
    for _ in range(3):
        a.step()
        b.tree_stages(); b.force(); b.integrate()
    sa, sb = a.download(), b.download()
    for u, v in zip(sa, sb):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    a.close(); b.close()


def test_theta0_is_the_direct_sum(pkg, orc):
    n = 2048
    e = _engine(pkg, pkg.plummer(n, seed=39), theta=0.0)
    e.tree_stages(); e.force()
    _, ref, _ = _check_walk(e, f"quad theta=0 n={n}", tie_cap=0.0)
    d = orc.direct_f64(e.download_sorted_bodies(), e.params.G, e.params.eps2)
    assert np.all(ref["k"] == n)
    assert np.all(np.linalg.norm(ref["acc"] - d, axis=1) <= 1e-13 * ref["sabs"])
    e.close()


# ------------------------------------------------------------------ 3. it helps
def test_quadrupoles_halve_the_median_error(pkg):
    n = 200_000
    ic = pkg.plummer(n, seed=46)
    rows = np.random.default_rng(0).choice(n, 2048, replace=False)
    xyzm = np.stack([ic[0], ic[1], ic[2], ic[6]], 1).astype(np.float32)
    gp = pkg.default_params()
    exact = direct_acc_f64(xyzm, gp.G, gp.eps2, rows, block=16)  # the engines below run with these G and eps2
    for theta in (0.5, 0.7):
        med = {}
        for order in (1, 2):
            e = _engine(pkg, ic, order=order, theta=theta)
            assert (e.params.G, e.params.eps2) == (gp.G, gp.eps2)
            e.tree_stages(); e.force()
            a = np.stack(e.download_acc(), 1)[rows].astype(np.float64)
            med[order] = float(np.median(np.linalg.norm(a - exact, axis=1) / np.linalg.norm(exact, axis=1)))
            e.close()
        print(f"theta {theta}: median rel err vs direct sum, order 1 {med[1]:.3e}, order 2 {med[2]:.3e} "
              f"(ratio {med[2] / med[1]:.3f})")
        assert med[2] <= GAIN[theta] * med[1], (theta, med)


# ------------------------------------------------------------------ 4. energy
def test_potential_and_energy_walk(pkg):
    n = 20000
    e = _engine(pkg, pkg.plummer(n, seed=47))
    e.tree_stages(); e.force()
    f = _acc_sorted(e)
    e.energy()
    g = _acc_sorted(e)
    assert np.array_equal(f.view(np.uint32), g.view(np.uint32))  # bh_energy's walk is the force launch's, bit for bit
    phi = e.download_potential()[e.download_order()]
    rec = e.download_tree()
    ref = quadrupole_f64(rec, e.download_sorted_bodies(), e.params.G, e.params.theta, e.params.eps2)
    nontie = ref["margin"] >= 1e-5
    rel = np.abs(phi.astype(np.float64) - ref["phi"]) / np.abs(ref["phi"])
    med, p9999 = float(np.median(rel[nontie])), float(np.quantile(rel[nontie], 0.9999))
    print(f"quad phi: rel p50 {med:.2e} p99.99 {p9999:.2e} max {rel[nontie].max():.2e}")
    assert med <= PHI_MED and p9999 <= PHI_P9999
    e.close()


def test_energy_does_not_perturb_the_run(pkg):
    ic = pkg.plummer(30000, seed=48)
    a = _engine(pkg, ic)
    b = _engine(pkg, ic)
    for s in range(6):
        a.step()
        b.step()
        if s % 2 == 0:
            b.energy()
    for u, v in zip(a.download(), b.download()):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    a.close(); b.close()


# ------------------------------------------------------------------ 5. reproducibility
def test_twenty_steps_are_reproducible(pkg):
    ic = pkg.plummer(65536, seed=49)
    out = []
    for _ in range(2):
        e = _engine(pkg, ic)
        e.step(20)
        out.append(e.download())
        assert e.stats().status_flags == 0
        e.close()
    for u, v in zip(*out):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_switching_back_changes_nothing(pkg):
    ic = pkg.plummer(30000, seed=50)
    a = _engine(pkg, ic, order=1)
    b = _engine(pkg, ic, order=1)
    for _ in range(2):
        a.step(); b.step()
    b.set_multipole(2)
    b.set_multipole(1)
    assert b.multipole == 1
    for _ in range(3):
        a.step(); b.step()
    for u, v in zip(a.download(), b.download()):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    a.close(); b.close()


def test_order_two_differs_from_order_one(pkg):
    ic = pkg.plummer(4096, seed=51)
    a = _engine(pkg, ic, order=1)
    b = _engine(pkg, ic)
    a.tree_stages(); a.force()
    b.tree_stages(); b.force()
    fa, fb = _acc_sorted(a), _acc_sorted(b)
    assert not np.array_equal(fa, fb)
    assert np.abs(fa - fb).max() < 0.05 * np.abs(fa).max()
    a.close(); b.close()


# ------------------------------------------------------------------ 6. error paths
def test_error_paths(pkg):
    lib = pkg._lib.lib
    import ctypes as C
    ic = pkg.plummer(4096, seed=52)
    e = _engine(pkg, ic, order=1)
    assert e.multipole == 1
    for bad in (0, 3, -1):
        assert lib.bh_set_multipole(e._h, bad) == -1
    # ORDER: no COM stage with order 2 yet
    e.tree_stages()
    assert lib.bh_download_multipoles(e._h, None, 0, None) == -6
    e.set_multipole(2)
    assert lib.bh_force(e._h) == -6                        # the switch invalidated the COM stage
    assert lib.bh_download_multipoles(e._h, None, 0, None) == -6
    e.com()
    assert lib.bh_force(e._h) == 0
    cnt = C.c_int(0)
    assert lib.bh_download_multipoles(e._h, None, 0, C.byref(cnt)) == 0 and cnt.value > 0
    buf = np.zeros((cnt.value - 1, 6), np.float32)
    assert lib.bh_download_multipoles(e._h, buf.ctypes.data_as(C.POINTER(C.c_float)), cnt.value - 1,
                                      C.byref(cnt)) == -7
    # no fall-back to monopoles
    assert lib.bh_force_range(e._h, 0, 64) == -1
    assert lib.bh_force_count(e._h) == -1
    st = pkg._lib.BhWalkStats()
    assert lib.bh_force_walk_stats(e._h, C.byref(st)) == -1
    rows = np.zeros(4 * 4096, np.uint32)
    nr = C.c_int(0)
    assert lib.bh_force_launch_trace(e._h, rows.ctypes.data_as(C.POINTER(C.c_uint32)), 4096, C.byref(nr)) == -1
    # a new tree: its COM stage decides
    e.bbox(); e.morton(); e.sort(); e.build()
    assert lib.bh_download_multipoles(e._h, None, 0, None) == -6
    e.com()
    assert lib.bh_download_multipoles(e._h, None, 0, None) == 0
    # the decomposed step refuses order 2 (and order 2 refuses a decomposed context)
    import torch
    sz = pkg.Engine.dd_query(4096, 2, 1024, 8192)
    pool = torch.zeros(sz.pool_records * 32, dtype=torch.uint8, device="cuda:0")  # a real pool of the queried size
    torch.cuda.synchronize()
    assert lib.bh_dd_init(e._h, 2, 0, 8192, 1024, 8192, C.c_void_p(pool.data_ptr()), sz.pool_records) == -1
    e.close()
    d = pkg.Engine(4096)
    assert lib.bh_dd_init(d._h, 2, 0, 8192, 1024, 8192, C.c_void_p(pool.data_ptr()), sz.pool_records) == 0
    assert lib.bh_set_multipole(d._h, 2) == -1 and d.multipole == 1
    d.close()
    del pool
    # a switch of order invalidates the potentials of the last bh_energy (they were walked with the other order)
    p = _engine(pkg, ic, order=1)
    p.energy()
    p.download_potential()
    p.set_multipole(2)
    assert lib.bh_download_potential(p._h, np.zeros(4096, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == -6
    p.energy()
    p.download_potential()
    p.close()
    for kw in (dict(strict_fp=1), dict(literal_force=1)):
        s = pkg.Engine(4096, **kw)
        assert lib.bh_set_multipole(s._h, 2) == -1 and s.multipole == 1
        s.close()


# ------------------------------------------------------------------ 7. bh_bench --multipole 2
ELINE = re.compile(r"^energy step (\d+) K (\S+) W (\S+) E (\S+) dE/\|E0\| (\S+)$")
FRAME = re.compile(r"^\d+\s+\| [0-9.]+\s+\| [0-9.]+$")


def _bench(*args, ok=True):
    exe = os.path.join(ROOT, "nbody-barnes-hut-cuda_amd", "bh_bench")
    r = subprocess.run([exe, "--n", "65536", "--steps", "20", "--ic", "plummer", *args], capture_output=True,
                       text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_bench_multipole_lines():
    out = _bench("--multipole", "2").stdout.splitlines()
    assert "multipole order 2: quadrupole moments, compiler-scheduled walk" in out
    assert len([l for l in out if FRAME.match(l.rstrip())]) == 20
    assert any(l.startswith("N=65536 ic=plummer") for l in out)
    en = _bench("--multipole", "2", "--energy", "5").stdout.splitlines()
    lines = [ELINE.match(l) for l in en if l.startswith("energy")]
    assert len(lines) == 4 and all(lines)
    assert [int(m.group(1)) for m in lines] == [5, 10, 15, 20]
    for m in lines:
        K, W, E, dE = (float(m.group(i)) for i in range(2, 6))
        assert K > 0 > W and abs(E - (K + W)) <= 1e-6 * abs(W) and abs(dE) < 0.1
    plain = _bench().stdout.splitlines()
    assert not any(l.startswith("multipole") for l in plain)
    r = _bench("--multipole", "2", "--gpus", "2", ok=False)
    assert r.returncode != 0 and "--multipole" in r.stderr
