"""Order 2 (bh_set_multipole) without a GPU: the library exports and binds the interface, and the fp64 reference of
tests/quadrupole_ref.py is right — the two-mass example of the definition, the order of the truncation error of one
isolated cell, a better walk than monopoles on an oracle-built tree, and an error bound that catches the traceless
(unsoftened) form of the t term at eps2 = 50."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import force_f64_flags, oparams, oracle_pipeline
from quadrupole_ref import S6, direct_acc_f64, expansion_terms, moments_f64, quadrupole_f64, record_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD_C = 1.8  # tests/test_gpu_quadrupole.py: the per-body constant of check_force_f64 for the order-2 walk


def test_library_exports_and_binds_the_multipole_interface(pkg):
    lib = C.CDLL(os.path.join(ROOT, "nbody-barnes-hut-cuda_amd", "libbh.so"))
    for name in ("bh_set_multipole", "bh_get_multipole", "bh_download_multipoles"):
        assert hasattr(lib, name), name
    bound = {s[0] for s in pkg._lib.SYMBOLS}
    assert {"bh_set_multipole", "bh_get_multipole", "bh_download_multipoles"} <= bound
    for attr in ("set_multipole", "multipole", "download_multipoles"):
        assert hasattr(pkg.Engine, attr), attr
    # null contexts are refused, not dereferenced
    assert pkg._lib.lib.bh_set_multipole(None, 2) == -1
    assert pkg._lib.lib.bh_get_multipole(None) == -1
    assert pkg._lib.lib.bh_download_multipoles(None, None, 0, None) == -1


def _one_record(m, c, S, kind=2, s=1.0):
    rec = np.zeros(1, [("x", "f4"), ("y", "f4"), ("z", "f4"), ("m", "f4"), ("s", "f4"), ("first", "i4"),
                       ("count", "i4"), ("kind", "i4")])
    rec["x"], rec["y"], rec["z"] = c
    rec["m"], rec["s"], rec["kind"] = m, s, kind
    return rec


def test_two_masses_on_the_axis():
    """two masses m/2 at +-a on the x axis seen from D on that axis, eps = 0: G m / D^2 + 3 G m a^2 / D^4"""
    G, m, a, D = 0.5, 2.0, 1.0, 10.0
    S = np.array([[m * a * a, 0, 0, 0, 0, 0]], float)
    ax, ay, az, phi, _ = expansion_terms(np.array([-D]), np.zeros(1), np.zeros(1), np.array([m]), S, G, 0.0)
    assert ax[0] == pytest.approx(-(G * m / D ** 2 + 3 * G * m * a * a / D ** 4), rel=1e-14)
    assert ay[0] == 0 and az[0] == 0
    # potential: -G m / D - G m a^2 / D^3 (the same expansion of -G m/2 (1/(D-a) + 1/(D+a)))
    assert phi[0] == pytest.approx(-(G * m / D + G * m * a * a / D ** 3), rel=1e-14)
    # and through the walk and the moments of the record's bodies
    xyzm = np.array([[-a, 0, 0, m / 2], [a, 0, 0, m / 2], [D, 0, 0, 1e-30]], np.float32)
    rec = _one_record(m, (0, 0, 0), None)
    rec["first"], rec["count"] = 0, 2
    assert np.allclose(moments_f64(rec, xyzm[:2]), S)


def _cell(rng, nb=64, s=1.0):
    p = rng.uniform(-s / 2, s / 2, (nb, 3))
    m = rng.uniform(1, 3, nb)
    c = (m[:, None] * p).sum(0) / m.sum()
    return p, m, c


def test_isolated_cell_error_order():
    """relative error against the exact sum: (s/D)^3 with quadrupoles (the dipole vanishes about the COM), (s/D)^2
    without — the error ratio of D and 2D is ~8 and ~4"""
    rng = np.random.default_rng(3)
    p, m, c = _cell(rng)
    d = p - c
    S = np.array([[(m * d[:, i] * d[:, j]).sum() for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]])
    G, eps2 = 1.0, 1e-9
    u = np.array([0.6, -0.48, 0.64])  # a unit direction off every axis
    errs = {1: [], 2: []}
    Ds = [8.0, 16.0, 32.0, 64.0]
    for D in Ds:
        x = c + D * u
        dd = p - x
        exact = (G * m[:, None] * dd / (((dd * dd).sum(1) + eps2) ** 1.5)[:, None]).sum(0)
        dc = (c - x)[None, :]
        for order in (1, 2):
            ax, ay, az, _, _ = expansion_terms(dc[:, 0], dc[:, 1], dc[:, 2], np.array([m.sum()]), S, G, eps2, order)
            a = np.array([ax[0], ay[0], az[0]])
            errs[order].append(np.linalg.norm(a - exact) / np.linalg.norm(exact))
    r1 = [errs[1][i] / errs[1][i + 1] for i in range(3)]
    r2 = [errs[2][i] / errs[2][i + 1] for i in range(3)]
    print("monopole", errs[1], r1, "quadrupole", errs[2], r2)
    assert all(3.5 < r < 4.5 for r in r1), r1
    assert all(7.0 < r < 9.0 for r in r2), r2
    assert all(e2 < 0.2 * e1 for e1, e2 in zip(errs[1], errs[2]))


def _oracle_tree(O, pkg, n, seed=7, **kw):
    p = pkg.default_params(**kw)
    ic = pkg.plummer(n, seed=seed)
    t = oracle_pipeline(O, ic, oparams(O, p))
    return p, t


def test_record_ranges_and_moments_match_a_direct_sum(pkg, orc):
    p, t = _oracle_tree(orc, pkg, 3000)
    rec, xyzm = t["rec"], t["xyzm"]
    lo, hi = record_ranges(rec)
    live = rec["kind"] != 3
    assert np.array_equal(lo[live], t["er_lo"][: len(rec)][live]) and np.array_equal(hi[live], t["er_hi"][: len(rec)][live])
    S = moments_f64(rec, xyzm)
    for e in np.flatnonzero(rec["kind"] == 1)[:50]:
        b = xyzm[lo[e]:hi[e]].astype(np.float64)
        d = b[:, :3] - np.array([rec["x"][e], rec["y"][e], rec["z"][e]], np.float64)
        want = [(b[:, 3] * d[:, i] * d[:, j]).sum() for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
        assert np.allclose(S[e], want, rtol=1e-12, atol=0), (e, S6)
    assert (S[rec["kind"] == 0] == 0).all()


def test_quadrupole_walk_beats_the_monopole_walk(pkg, orc):
    """oracle-built tree, theta 0.5: the order-2 walk's median error against the direct sum is far below order 1's"""
    p, t = _oracle_tree(orc, pkg, 4000, seed=11)
    rec, xyzm = t["rec"], t["xyzm"]
    idx = np.arange(0, 4000, 7)
    exact = direct_acc_f64(xyzm, p.G, p.eps2, idx)
    S = moments_f64(rec, xyzm)
    med = {}
    for order in (1, 2):
        r = quadrupole_f64(rec, xyzm, p.G, p.theta, p.eps2, S=S, idx=idx, order=order)
        rel = np.linalg.norm(r["acc"] - exact, axis=1) / np.linalg.norm(exact, axis=1)
        med[order] = float(np.median(rel))
    print("median rel err vs direct sum: order 1 %.3e, order 2 %.3e" % (med[1], med[2]))
    assert med[2] < 0.5 * med[1]
    # order 1 is the monopole walk of oracle.force_f64 on the same tree
    f = orc.force_f64(rec, xyzm, oparams(orc, p), idx=idx.astype(np.int32))
    r1 = quadrupole_f64(rec, xyzm, p.G, p.theta, p.eps2, idx=idx, order=1)
    assert np.allclose(r1["acc"], f["acc"], rtol=1e-12, atol=1e-300)
    assert np.array_equal(r1["k"], f["k"].astype(np.int64))


def test_error_bound_catches_the_traceless_t_term(pkg, orc):
    """at eps2 = 50 the walk with the unsoftened traceless t term differs from the exact expansion by far more than the
    per-body bound the GPU tests use (QUAD_C): the check is sharp enough to see the eps2 part"""
    p, t = _oracle_tree(orc, pkg, 4000, seed=13)
    assert p.eps2 == 50.0
    rec, xyzm = t["rec"], t["xyzm"]
    S = moments_f64(rec, xyzm)
    ref = quadrupole_f64(rec, xyzm, p.G, p.theta, p.eps2, S=S)
    wrong = quadrupole_f64(rec, xyzm, p.G, p.theta, p.eps2, S=S, traceless=True)
    bad = force_f64_flags(wrong["acc"], ref, QUAD_C)
    print(f"traceless t term flagged on {bad.mean():.1%} of the bodies")
    assert bad.mean() > 0.5
    assert not force_f64_flags(ref["acc"], ref, QUAD_C).any()
