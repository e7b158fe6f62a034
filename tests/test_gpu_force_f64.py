"""Every force walk the planner (plan_force, csrc/bh_force.hip) can choose for a single context, against the fp64 walk
of the SAME tree (oracle.force_f64 on Engine.download_tree() and download_sorted_bodies(): centre-of-mass rounding
does not enter) with the per-body error model of helpers.check_force_f64.  A tie body (a cell within 1e-5 of the MAC
boundary) keeps the old relative 5e-4; every other body must have exactly the reference's interactions, summed to
within F64_C sqrt(max(k, 48)) u sum|term| — a dropped, repeated or misweighted interaction shows there where the old
max of 5e-4 let it through.

The sizes sit where the planner changes its mind, derived from its rules for the MI355X's 256 CUs (as
test_force_launch_trace_is_the_product_launch does), and every case asserts that the intended walk ran: the rows of
the traced launch (one per wave), the group size and the waves per group."""
import numpy as np
import pytest

from helpers import check_force_f64, oparams, special_ics

pytestmark = pytest.mark.gpu

CUS = 256
T = CUS * 4 * 7 // 3          # groups of the cooperative tail of a mixed launch (kTailWaves = 7): 2,389
PF_MAX = 200_000              # kPrefetchMaxBodies: the one-wave walk with the scalar-cache prefetch up to here


def default_plan(n):
    """(walk, K, bulk, trace rows) of the default engine's launch over n bodies (force_coop = 0, 64-body groups):
    cooperative throughout up to 2T groups — 8 waves per group while 8 per group fit the GPU (groups * 8 <= 256 CUs *
    4 SIMDs * 8 waves), else 4 — then mixed: the first gb groups one wave each, the last T to T + 3 by four."""
    G = (n + 63) // 64
    if G > 2 * T:
        gb = (G - T) // 4 * 4
        return "mixed", 4, gb * 64, gb + 4 * (G - gb)
    K = 8 if G * 8 <= CUS * 4 * 8 else 4
    return "coop", K, 0, G * K


def one_wave_group(n):
    """bodies per wave of the one-wave walk (force_coop = 1, force_group automatic)"""
    return 16 if n <= 20 * 1024 else (32 if n <= 56 * 1024 else 64)


def sample(n, bulk=0, every=8):
    """sorted body indices: every `every`-th, plus all bodies of the first group, of the last two and of the groups
    on either side of the bulk / tail boundary"""
    if n <= 70_000:
        return None
    s = [np.arange(0, n, every), np.arange(0, 64), np.arange(max(0, (n - 1) // 64 * 64 - 64), n)]
    if 0 < bulk < n:
        s.append(np.arange(bulk - 64, min(n, bulk + 64)))
    return np.unique(np.concatenate(s)).astype(np.int32)


def _engine(pkg, ic, **kw):
    e = pkg.Engine(len(ic[0]), **kw)
    e.upload(*ic)
    return e


def _reference(orc, e, idx=None):
    """the fp64 walk of e's current tree over e's sorted bodies (rows: idx, or all bodies)"""
    return orc.force_f64(e.download_tree(), e.download_sorted_bodies(), oparams(orc, e.params), idx=idx)


def _acc_sorted(e, order=None):
    """e's accelerations in sorted order (download_acc is in upload order; slot i holds body order[i])"""
    a = np.stack(e.download_acc(), 1)
    return a[e.download_order() if order is None else order]


def _check(orc, e, label, idx=None, **kw):
    ref = _reference(orc, e, idx)
    acc = _acc_sorted(e)[ref["idx"]]
    assert np.isfinite(acc).all(), label
    fig = check_force_f64(acc, ref, label, **kw)
    assert e.stats().status_flags == 0
    return fig, ref, acc


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 4097, 65536, 65537, 305_792, 305_856, 500_000,
                               1_000_000])
def test_default_engine_walk_vs_f64(pkg, orc, n):
    """the walk bh_step makes, at the planner's boundaries: K 8 -> 4 between 65,536 and 65,537 bodies (1,024 ->
    1,025 groups), cooperative -> mixed between 305,792 and 305,856 (2T = 4,778 -> 4,779 groups), a mixed launch with
    a partial last group at 500,000, and 1M sampled"""
    walk, K, bulk, rows = default_plan(n)
    ic = pkg.plummer(n, seed=31)
    e = _engine(pkg, ic)
    e.tree_stages(); e.force()
    tr = e.force_launch_trace()
    assert tr.shape[0] == rows, (walk, K, tr.shape, rows)
    _check(orc, e, f"default n={n} ({walk}, K={K}, bulk={bulk})", sample(n, bulk))
    e.close()


@pytest.mark.parametrize("n", [20_480, 20_481, 57_344, 57_345, 200_000, 200_001])
def test_one_wave_walk_vs_f64(pkg, orc, n):
    """force_coop = 1: the depth-first walk, 16 / 32 / 64 bodies per wave (switches after 20,480 and 57,344), with the
    scalar-cache prefetch up to 200,000 bodies (fast_pf) and without it above (fast)"""
    group = one_wave_group(n)
    ic = pkg.plummer(n, seed=32)
    e = _engine(pkg, ic, force_coop=1)
    e.tree_stages(); e.force()
    assert e.force_launch_trace().shape[0] == (n + group - 1) // group
    walk = "fast_pf" if n <= PF_MAX else "fast"
    _check(orc, e, f"one-wave n={n} ({walk}, group {group})", sample(n))
    e.close()


@pytest.mark.parametrize("n", [4096, 65536])
def test_compiler_scheduled_walk_vs_f64(pkg, orc, n):
    """force_variant = 1 (fast_v1: no traced instance)"""
    ic = pkg.plummer(n, seed=33)
    e = _engine(pkg, ic, force_variant=1)
    e.tree_stages(); e.force()
    assert len(e.force_launch_trace()) == 0
    _check(orc, e, f"variant 1 n={n}")
    e.close()


@pytest.mark.parametrize("kw", [dict(force_coop=K) for K in range(2, 9)] + [dict(force_group=16), dict(force_group=32)])
def test_coop_walk_by_hand_vs_f64(pkg, orc, kw):
    """force_coop 2..8 at 65,536 bodies (1,024 groups of 64), and 16- / 32-body groups of the automatic cooperative
    walk (4,096 / 2,048 groups: four waves each)"""
    n = 65536
    group = kw.get("force_group", 64)
    G = n // group
    K = kw.get("force_coop", 8 if G * 8 <= CUS * 4 * 8 else 4)
    ic = pkg.plummer(n, seed=34)
    e = _engine(pkg, ic, **kw)
    e.tree_stages(); e.force()
    if G * K <= (n + 63) // 64 * 8 + 64:   # (force_launch_trace's rows are sized for 64-body groups)
        assert e.force_launch_trace().shape[0] == G * K
    _check(orc, e, f"coop {kw} n={n}")
    assert e.stats().force_redo_waves == 0
    e.close()


def test_generic_counting_walk_vs_f64(pkg, orc):
    """bh_force_count (force_kernel, fast arithmetic on the canonical records): accelerations, and V / O / P per body
    equal to the reference's on every non-tie body"""
    n = 65536
    ic = pkg.plummer(n, seed=35)
    e = _engine(pkg, ic)
    e.tree_stages(); e.force_count()
    _, ref, _ = _check(orc, e, f"generic (counting) n={n}")
    order = e.download_order()
    nt = ref["margin"] >= 1e-5
    for name, c in zip("VOP", e.download_counters()):
        assert np.array_equal(c[order][nt], ref[name][nt]), name
    e.close()


@pytest.mark.parametrize("n", [65536, 500_000])
def test_force_range_vs_f64(pkg, orc, n):
    """bh_force_range: slabs on 256-body boundaries, and at 500,000 (mixed) one slab that straddles `bulk` — two
    launches, the one-wave part and the cooperative part"""
    _, _, bulk, _ = default_plan(n)
    if bulk:
        cuts = [0, bulk - 6400, bulk + 6400, n]
        assert cuts[1] % 256 == 0 and (cuts[2] - bulk) % 64 == 0
    else:
        q = n // 4 // 256 * 256
        cuts = [0, q, 3 * q, n]
    ic = pkg.plummer(n, seed=36)
    e = _engine(pkg, ic)
    e.tree_stages()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e.force(lo, hi)
    _check(orc, e, f"range n={n} cuts {cuts}", sample(n, bulk))
    e.close()


@pytest.mark.parametrize("n", [65536, 500_000])
def test_fused_step_vs_f64(pkg, orc, n):
    """the accelerations of one bh_step (the FUSE instance of the walk, which also integrates), against the fp64 walk
    of the tree a second engine builds from the same input through the stage calls — bit for bit the step's tree"""
    _, _, bulk, _ = default_plan(n)
    ic = pkg.plummer(n, seed=37)
    e = _engine(pkg, ic)
    e.step(1)
    a = np.stack(e.download_acc(), 1)
    assert e.stats().status_flags == 0
    e.close()
    t = _engine(pkg, ic)
    t.tree_stages()
    order = t.download_order()
    ref = _reference(orc, t, sample(n, bulk))
    check_force_f64(a[order][ref["idx"]], ref, f"fused step n={n}")
    t.close()


@pytest.mark.parametrize("theta", [0.3, 1.0])
def test_theta_vs_f64(pkg, orc, theta):
    """theta 0.3 and 1.0 on the default engine (0.5 is the default of every other case)"""
    n = 65536
    ic = pkg.plummer(n, seed=38)
    e = _engine(pkg, ic, theta=theta)
    e.tree_stages(); e.force()
    _check(orc, e, f"theta={theta} n={n}")
    e.close()


def test_theta0_vs_direct_sum(pkg, orc):
    """theta = 0 opens every cell: the fp64 walk is the fp64 direct sum, and the walk is held to its bound"""
    n = 2048
    ic = pkg.plummer(n, seed=39)
    e = _engine(pkg, ic, theta=0.0)
    e.tree_stages(); e.force()
    _, ref, _ = _check(orc, e, f"theta=0 n={n}", tie_cap=0.0)
    d = orc.direct_f64(e.download_sorted_bodies(), e.params.G, e.params.eps2)
    assert np.all(ref["k"] == n)
    assert np.all(np.linalg.norm(ref["acc"] - d, axis=1) <= 1e-13 * ref["sabs"])
    e.close()


@pytest.mark.parametrize("kw", [dict(key_curve=0), dict(key_curve=1), dict(leaf_cap=1), dict(leaf_cap=3),
                                dict(leaf_cap=4), dict(leaf_cap=8), dict(leaf_cap=16)])
def test_trees_vs_f64(pkg, orc, kw):
    """both key curves; unsplit cells of up to 1, 3, 4, 8 and 16 bodies (odd cells, and the NULL record that pads an
    odd child block) at an odd body count"""
    n = 20001
    ic = pkg.plummer(n, seed=40)
    e = _engine(pkg, ic, **kw)
    e.tree_stages(); e.force()
    if kw.get("leaf_cap", 1) > 1:
        assert (e.download_tree()["kind"] == orc.KIND_MULTI).sum() > 0
    _check(orc, e, f"tree {kw} n={n}")
    e.close()


# edge inputs: the per-body bound, the tie cap and TIE_REL_MAX as everywhere; the population limits of the relative
# error are their own (twice what was measured) where forces cancel to ~0: the middle of the collinear row, p99.99
# 5.0e-4 and max 7.1e-4 (the oracle's own fp32 walk: 6.3e-4 / 7.5e-4); median 3.5e-7
EDGE_LIMITS = dict(tie_cap=0.05, med=7e-7, p9999=1e-3, rmax=1.5e-3)


@pytest.mark.parametrize("name", ["coincident", "collinear", "outlier", "pairs", "tiny", "grid", "zero_mass"])
def test_edge_inputs_vs_f64(pkg, orc, name):
    n = 5000
    ic = special_ics(name, n, np.random.default_rng(5))
    e = _engine(pkg, ic)
    e.tree_stages(); e.force()
    _check(orc, e, f"edge {name} n={n}", **EDGE_LIMITS)
    e.close()
