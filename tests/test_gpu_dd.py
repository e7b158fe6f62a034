"""Domain-decomposed multi-GPU stepping (bh_rank / bh_dd_* of include/bh.h, dist.DomainStepper) on ONE GPU:
P ranks run as P threads of this process (dist.LocalComm = the library's in-process transport bh_hub: the
exchanges are device copies), each with its own context, owning one interval of the key curve.  The stitched tree (local octree + top tree +
imported LET segments) must reproduce the single-context run: same canonical octree, so forces
agree up to summation order / the last bit of cell sums."""
import threading
import time

import numpy as np
import pytest

import bhpkg

pytestmark = pytest.mark.gpu


def run_ranks(world, ic, steps, comm=None, before_last=None, **kw):
    """comm(group, rank): the rank's transport (default dist.LocalComm).  before_last: a list that receives every
    rank's local_state() + (let_retries,) after steps - 1 steps; the last step is then taken by a call of its own."""
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    order = bhdist.global_morton_order(pkg, ic, 0)
    group = bhdist.LocalGroup(world)
    group.slots = [None] * world
    stream = torch.cuda.Stream(0)
    out, errs = [None] * world, []
    if before_last is not None:
        before_last[:] = [None] * world

    def work(r):
        try:
            torch.cuda.set_device(0)
            st = bhdist.DomainStepper(pkg, ic, (comm or bhdist.LocalComm)(group, r), 0, stream=stream, order=order,
                                      mig_log=True, **kw)
            group.barrier.wait()
            if before_last is not None:
                st.step(steps - 1)
                before_last[r] = st.local_state() + (st.let_retries,)   # (bh_dd_download only reads)
                st.step(1)
            else:
                st.step(steps)
            assert st.e.stats().status_flags == 0
            out[r] = st.local_state() + (st.let_counts.copy(), st.let_retries, st.e.dd_info(), st.mig_log, st.n_loc)
            group.barrier.wait()
            st.close()
        except BaseException as ex:  # noqa: BLE001 - report from the main thread
            errs.append((r, ex))
            group.abort()            # releases ranks waiting inside an exchange (BH_ERR_COMM)
            group.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0][1]
    return out


def merge(out, n):
    pos = np.zeros((n, 3), np.float32)
    vel = np.zeros((n, 3), np.float32)
    acc = np.zeros((n, 3), np.float32)
    seen = np.zeros(n, np.int32)
    for ids, posm, v, a, *_ in out:
        pos[ids] = posm[:, :3]
        vel[ids] = v
        acc[ids] = a
        seen[ids] += 1
    assert (seen == 1).all(), "every body must be owned by exactly one rank"
    return pos, vel, acc


def single(ic, steps, **kw):
    pkg = bhpkg.load()
    n = len(ic[0])
    with pkg.Engine(n, **kw) as e:
        e.upload(*ic)
        e.step(steps)
        x, y, z, vx, vy, vz = e.download()
        ax, ay, az = e.download_acc()
        assert e.stats().status_flags == 0
    return np.stack([x, y, z], 1), np.stack([vx, vy, vz], 1), np.stack([ax, ay, az], 1)


def rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)


def state_of(parts, n):
    """the merged state of every rank's (ids, posm, vel, ...) as initial conditions in id order: x, y, z, vx, vy, vz, m"""
    posm = np.zeros((n, 4), np.float32)
    vel = np.zeros((n, 3), np.float32)
    seen = np.zeros(n, np.int32)
    for ids, pm, v, *_ in parts:
        posm[ids] = pm
        vel[ids] = v
        seen[ids] += 1
    assert (seen == 1).all(), "every body must be owned by exactly one rank"
    return tuple(np.ascontiguousarray(c) for c in (*posm[:, :3].T, *vel.T, posm[:, 3]))


def single_from(state, steps=1, **kw):
    """a fresh single context from a merged state (state_of), `steps` steps: positions, velocities, accelerations"""
    return single(state, steps, **kw)


# |dvel| after ONE decomposed step against one single-context step from the same state.  Measured on MI355X over every
# case that applies the check (check_last_step; tests/test_gpu_dist.py for the multi-process workers): at most 1.9e-6
# in-process at theta = 0.5, 7.6e-6 for the 2 x 500,000-body workers, 1.53e-5 at theta = 0.2 (2,000,000 bodies).  The
# bound is about 3x the largest of them; a body whose velocity is off by one step's worth of a wrong acceleration, or
# 1e-3 added on migration, lies far above it.
DVEL_MAX = 5e-5


def check_last_step(out, before, ic, acc=(2e-6, 1e-4, 2e-3), **kw):
    """The same-state check of a K-step decomposed run: its LAST step against one single-context step from the merged
    state after K - 1 steps (before: run_ranks(before_last=...)).  The decomposed walk reproduces the single context's
    canonical tree, so the first-step bounds hold for that step: accelerations (relative error median, p99.99, max),
    |dpos| after the step and a |dvel| bound.  Masses after K steps are the initial masses bit for bit.
    -> the measured figures"""
    n = len(ic[0])
    p, v, a = merge(out, n)
    m = np.zeros(n, np.float32)
    for ids, posm, *_ in out:
        m[ids] = posm[:, 3]
    m0 = np.ascontiguousarray(ic[6], np.float32)
    assert np.array_equal(m.view(np.uint32), m0.view(np.uint32)), \
        f"{int((m.view(np.uint32) != m0.view(np.uint32)).sum())} bodies changed mass"
    p1, v1, a1 = single_from(state_of(before, n), 1, **kw)
    e = rel(a, a1)
    f = dict(acc_median=float(np.median(e)), acc_p9999=float(np.quantile(e, 0.9999)), acc_max=float(e.max()),
             dpos=float(np.abs(p - p1).max()), dvel=float(np.abs(v - v1).max()))
    print("last step vs one single-context step from the same state: acc rel median {acc_median:.2e} p99.99 "
          "{acc_p9999:.2e} max {acc_max:.2e}; |dpos| max {dpos:.2e}; |dvel| max {dvel:.2e}".format(**f))
    assert f["acc_median"] < acc[0], f
    assert f["acc_p9999"] < acc[1], f
    assert f["acc_max"] < acc[2], f
    assert f["dpos"] < 1e-3, f
    assert f["dvel"] < DVEL_MAX, f
    return f


@pytest.mark.parametrize("split", [False, True, 100])
@pytest.mark.parametrize("let_mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_dd_first_step_matches_single_context(world, let_mode, split):
    """let_mode 0: X4 = all-gather of the union of what any rank may open; 1 (default): per-destination segments
    exchanged with an all-to-all — a receiver holds only what its own boxes can open, the rest arrives closed.
    split: False = one force pass after X4; True = the default two-pass form (the first 30 % of a rank's bodies: own
    pieces on a side stream while X4 travels, then the remote pass; the rest in one pass after X4); 100 = every body in
    two passes"""
    kw = dict(split_pct=100) if split == 100 and split is not True else {}
    split = bool(split)
    pkg = bhpkg.load()
    n = 60000
    ic = pkg.plummer(n, seed=7)
    p1, v1, a1 = single(ic, 1)
    out = run_ranks(world, ic, 1, let_mode=let_mode, split=split, **kw)
    p, v, a = merge(out, n)
    e = rel(a, a1)
    # same accepted sets; fp32 summation order differs (top tree first, segments interleaved)
    assert np.median(e) < 2e-6, np.median(e)
    assert np.quantile(e, 0.9999) < 1e-4, np.quantile(e, 0.9999)
    assert e.max() < 2e-3, e.max()
    assert np.abs(p - p1).max() < 1e-3


@pytest.mark.parametrize("world,split,let_mode", [(2, True, 1), (4, True, 1), (4, 100, 1), (4, False, 1), (4, True, 0), (3, False, 0)])
def test_dd_many_steps_conserve_and_track(world, split, let_mode):
    """split: two-pass force (own pieces on a side stream while X4 is in flight + remote pieces; 100: for every body)"""
    kw = dict(split_pct=100) if split == 100 else {}
    split = bool(split)
    pkg = bhpkg.load()
    n = 40000
    ic = pkg.plummer(n, seed=11)
    steps = 12
    p1, v1, a1 = single(ic, steps)
    before = []
    out = run_ranks(world, ic, steps, before_last=before, split=split, let_mode=let_mode, **kw)
    p, v, a = merge(out, n)     # also checks that migration lost / duplicated nobody
    assert sum(o[-1] for o in out) == n
    assert np.abs(p - p1).max() < 5e-2, np.abs(p - p1).max()
    e = rel(a, a1)
    assert np.median(e) < 1e-4, np.median(e)
    check_last_step(out, before, ic)


@pytest.mark.parametrize("world,pct,n,steps", [(3, 25, 60000, 1), (8, 25, 60000, 1), (8, 60, 160000, 5), (2, 10, 40000, 12),
                                                 (4, 25, 6000, 3)])
def test_dd_partial_two_pass_step(world, pct, n, steps):
    """split_pct < 100: only the first pct per cent of a rank's bodies are walked in two passes (their own pass hides
    the LET export and X4), the others in ONE pass after X4 — the remote pass of the first part on the side stream at
    the same time, both launches integrating their bodies and sharing one min / max fold.  Same canonical tree, same
    accepted sets: forces to summation order, as the other two forms (the last case: ranks so small that the split
    part rounds to nothing or to everything)."""
    pkg = bhpkg.load()
    ic = pkg.plummer(n, seed=13)
    p1, v1, a1 = single(ic, steps)
    before = [] if steps > 1 else None
    out = run_ranks(world, ic, steps, before_last=before, split=True, split_pct=pct)
    p, v, a = merge(out, n)
    assert sum(o[-1] for o in out) == n
    e = rel(a, a1)
    if steps == 1:
        assert np.median(e) < 2e-6 and np.quantile(e, 0.9999) < 1e-4 and e.max() < 2e-3, (np.median(e), e.max())
        assert np.abs(p - p1).max() < 1e-3
    else:
        assert np.median(e) < 1e-4, np.median(e)
        assert np.abs(p - p1).max() < 5e-2, np.abs(p - p1).max()
        check_last_step(out, before, ic)
    # and against the full two-pass form: the bodies of the split part get the same bits (same two launches' order)
    out2 = run_ranks(world, ic, steps, split=True, split_pct=100)
    p2, v2, a2 = merge(out2, n)
    assert np.abs(p - p2).max() < (1e-3 if steps == 1 else 5e-2)


def test_dd_per_destination_let_is_smaller_and_equivalent():
    """the per-destination X4 (all-to-all) against the union X4 (all-gather) on the same system, 8 ranks x 5 steps:
    the same canonical tree is walked (the closed copies are exactly the cells the receiver cannot open), so the
    states agree to the last bit of the summation order; and the largest segment any pair of ranks exchanges is
    well below the union every rank used to receive from every other"""
    pkg = bhpkg.load()
    n = 160000
    ic = pkg.plummer(n, seed=19)
    o0 = run_ranks(8, ic, 5, let_mode=0)
    o1 = run_ranks(8, ic, 5, let_mode=1)
    p0, v0, a0 = merge(o0, n)
    p1, v1, a1 = merge(o1, n)
    e = rel(a1, a0)
    assert np.median(e) < 1e-6 and e.max() < 2e-3, (np.median(e), e.max())
    assert np.abs(p1 - p0).max() < 1e-3
    need0 = max(int(o[4].max()) for o in o0)     # records of the largest union segment
    need1 = max(int(o[4].max()) for o in o1)     # records of the largest per-destination segment
    print(f"largest X4 segment: union {need0} records, per destination {need1}")
    assert need1 < 0.75 * need0, (need0, need1)


def test_dd_migration_across_ranks():
    """a fast cold stream crossing the domain boundaries: bodies must change owner"""
    pkg = bhpkg.load()
    n = 32768
    x, y, z, vx, vy, vz, m = [a.copy() for a in pkg.plummer(n, seed=3)]
    vx += 400.0  # everything drifts 8 units per step in +x while the slabs' splitters follow
    vx[: n // 2] -= 800.0
    ic = (x, y, z, vx, vy, vz, m)
    steps = 10
    p1, v1, a1 = single(ic, steps)
    before = []
    out = run_ranks(4, ic, steps, before_last=before)
    p, v, a = merge(out, n)
    assert np.abs(p - p1).max() < 5e-2
    e = rel(a, a1)
    assert np.median(e) < 1e-4
    # the bodies that changed owner in the last step came with their velocities and masses
    check_last_step(out, before, ic)


def test_dd_boundaries_persist_and_rebalance():
    """The domain boundaries (splitter keys) persist from step to step and move only when a rank's body count leaves
    n / P by more than 1.5 %: 200 steps of a system whose two halves
    stream through each other at first (so the counts drift and the boundaries HAVE to move several times) and then
    settles.  Checked: nobody lost or duplicated; the boundaries moved more than once but in at most a fifth of the
    steps (measured on MI355X, round 5: see the printed line; the bound was loosened to a third in round 4 to pass a
    run with 42 moves — restored); in the steps that kept them the emigrants are what physically crossed a boundary — per step well under
    1 % of a rank (round 3 re-drew the boundaries from samples every step: 2-5 % of every rank per step); every rank
    ends within 3 % of its fair share; forces of the final state against a single context."""
    pkg = bhpkg.load()
    n = 48000
    x, y, z, vx, vy, vz, m = [a.copy() for a in pkg.plummer(n, seed=21)]
    vx += 30.0
    vx[: n // 2] -= 60.0         # two halves drifting apart at first, 0.6 units per step each way
    ic = (x, y, z, vx, vy, vz, m)
    steps, world = 200, 4
    before = []
    out = run_ranks(world, ic, steps, before_last=before)
    p, v, a = merge(out, n)
    counts = np.array([o[-1] for o in out])
    assert counts.sum() == n
    info = out[0][6]
    moved = info[2]
    log = np.array(out[0][7])            # per step: (most emigrants found on any rank, what the boundaries did)
    kept = log[:, 1] == 0
    print(f"boundaries moved in {moved} of {steps} steps; emigrants per step (max over ranks): kept steps median "
          f"{np.median(log[kept, 0]):.0f} max {log[kept, 0].max()}, moved steps max {log[~kept, 0].max()}; "
          f"final counts {counts.tolist()}")
    assert 2 <= moved <= steps // 5, moved
    assert (log[:, 1] != 0).sum() == moved
    assert np.median(log[kept, 0]) < 0.01 * n / world
    assert np.abs(counts - n / world).max() <= 0.03 * n / world, counts
    p1, v1, a1 = single(ic, steps)
    # 200 chaotic steps: the trajectories of close pairs part; compare the bulk
    assert np.median(np.abs(p - p1).max(axis=1)) < 1e-2
    e = rel(a, a1)
    assert np.median(e) < 1e-3, np.median(e)
    check_last_step(out, before, ic)


def _check(ic, world, steps, tol_pos=5e-2, tol_med=1e-4, **kw):
    n = len(ic[0])
    p1, v1, a1 = single(ic, steps, **kw)
    out = run_ranks(world, ic, steps, **kw)
    p, v, a = merge(out, n)
    assert np.abs(p - p1).max() < tol_pos, np.abs(p - p1).max()
    e = rel(a, a1)
    assert np.median(e) < tol_med, np.median(e)
    return e


def test_dd_eight_ranks_vs_the_oracle_itself():
    """the domain-decomposed step against the CPU ORACLE (not against a single HIP context): 8 ranks in-process,
    65,536 Plummer bodies (BASELINE configs[0] size), K = 5 whole steps vs oracle.Oracle.step from identical
    inputs.  Same distribution form as tests/test_gpu_fullsize.py; the stitched tree accepts the same cells, the
    fp32 summation order differs (top tree first, LET segments interleaved).  Stated tolerance after 5 steps:
        |dx| median and p99.99 <= 3.1e-5 (one ulp of a position below 512), max <= 6.2e-5;
        |dv| median <= 1e-7, p99.99 <= 4e-6, max <= 5e-6;  last step's accelerations: relative median <= 1e-6, max <= 1e-4
    (<= 2x measured on MI355X, round 3: |dx| 0 / 5.5e-6 / 3.1e-5, |dv| 0 / 1.9e-6 / 2.4e-6, acc 5.1e-7 / max 4.1e-5)"""
    import oracle as O
    pkg = bhpkg.load()
    n, K, world = 65536, 5, 8
    ic = pkg.plummer(n, seed=42)
    out = run_ranks(world, ic, K)
    p, v, a = merge(out, n)
    o = O.Oracle(n, O.params(key_curve=pkg.default_params().key_curve))
    o.upload(*ic)
    o.step(K, order=O.ORDER_BATCHED)
    w = np.stack(o.download(), 1).astype(np.float64)
    oa = np.stack(o.download_acc(), 1)
    o.close()
    dx = np.abs(p.astype(np.float64) - w[:, :3]).max(axis=1)
    dv = np.abs(v.astype(np.float64) - w[:, 3:]).max(axis=1)
    e = rel(a, oa)
    print(f"DD x8 vs oracle, n={n} K={K}: |dx| p50 {np.median(dx):.3e} p99.99 {np.percentile(dx, 99.99):.3e} max {dx.max():.3e}; "
          f"|dv| p50 {np.median(dv):.3e} p99.99 {np.percentile(dv, 99.99):.3e} max {dv.max():.3e}; "
          f"acc rel p50 {np.median(e):.3e} max {e.max():.3e}")
    assert np.median(dx) <= 3.1e-5 and np.percentile(dx, 99.99) <= 3.1e-5 and dx.max() <= 6.2e-5
    assert np.median(dv) <= 1e-7 and np.percentile(dv, 99.99) <= 4e-6 and dv.max() <= 5e-6
    assert np.median(e) <= 1e-6 and e.max() <= 1e-4


def test_group_step_from_c_vs_oracle_and_python_binding():
    """the multi-GPU step driven from C only (ctypes on bh_create_group / bh_group_upload / bh_step_group /
    bh_group_download: no Python protocol code, one library thread per rank): 8 ranks on this GPU through the
    in-process transport, 65,536 bodies, 5 steps — within test_dd_eight_ranks_vs_the_oracle_itself's bounds of the
    ORACLE, and bit-identical to the DomainStepper-driven run (the same bh_rank_step under both)."""
    import ctypes as C
    import oracle as O
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    n, K, world = 65536, 5, 8
    ic = pkg.plummer(n, seed=42)
    g = C.c_void_p()
    dev = (C.c_int * world)(*([0] * world))
    assert L.lib.bh_create_group(C.byref(g), world, dev, n, None, None, 0) == 0
    try:
        F = L._F
        assert L.lib.bh_group_size(g) == world
        assert L.lib.bh_group_upload(g, *[np.ascontiguousarray(a).ctypes.data_as(F) for a in ic]) == 0
        assert L.lib.bh_step_group(g, K) == 0
        assert L.lib.bh_group_sync(g) == 0
        st6 = [np.full(n, np.nan, np.float32) for _ in range(6)]
        assert L.lib.bh_group_download(g, *[a.ctypes.data_as(F) for a in st6]) == 0
        acc = [np.full(n, np.nan, np.float32) for _ in range(3)]
        assert L.lib.bh_group_download_acc(g, *[a.ctypes.data_as(F) for a in acc]) == 0
        info = L.BhRankInfo()
        held = 0
        for q in range(world):
            assert L.lib.bh_rank_get_info(L.lib.bh_group_rank(g, q), C.byref(info)) == 0
            assert info.steps == K
            held += info.n_loc
        assert held == n
    finally:
        L.lib.bh_destroy_group(g)
    p, v, a = np.stack(st6[:3], 1), np.stack(st6[3:], 1), np.stack(acc, 1)
    assert np.isfinite(p).all() and np.isfinite(a).all()          # every body came back exactly once
    o = O.Oracle(n, O.params(key_curve=pkg.default_params().key_curve))
    o.upload(*ic)
    o.step(K, order=O.ORDER_BATCHED)
    w = np.stack(o.download(), 1).astype(np.float64)
    oa = np.stack(o.download_acc(), 1)
    o.close()
    dx = np.abs(p.astype(np.float64) - w[:, :3]).max(axis=1)
    dv = np.abs(v.astype(np.float64) - w[:, 3:]).max(axis=1)
    e = rel(a, oa)
    print(f"bh_step_group x8 vs oracle, n={n} K={K}: |dx| p50 {np.median(dx):.3e} p99.99 {np.percentile(dx, 99.99):.3e} "
          f"max {dx.max():.3e}; |dv| max {dv.max():.3e}; acc rel p50 {np.median(e):.3e} max {e.max():.3e}")
    assert np.median(dx) <= 3.1e-5 and np.percentile(dx, 99.99) <= 3.1e-5 and dx.max() <= 6.2e-5
    assert np.median(dv) <= 1e-7 and np.percentile(dv, 99.99) <= 4e-6 and dv.max() <= 5e-6
    assert np.median(e) <= 1e-6 and e.max() <= 1e-4
    out = run_ranks(world, ic, K)
    p2, v2, a2 = merge(out, n)
    assert np.array_equal(p, p2) and np.array_equal(v, v2) and np.array_equal(a, a2)


def test_ranks_given_arbitrary_subsets_of_the_bodies():
    """distributed input (bh_rank_upload takes ANY subset with its global ids: INTEGRATION.md §4b): every rank starts
    with a RANDOM quarter of the system — nothing sorted, nothing near its own domain — the first step draws sample
    quantiles and three quarters of every rank's bodies change owner over several X2 rounds; from then on the run
    must be the run that started from slabs of the curve: same canonical tree, forces to summation order."""
    import ctypes as C
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    n, world, K = 100_000, 4, 3
    ic = pkg.plummer(n, seed=31)
    rng = np.random.default_rng(5)
    owner = rng.permutation(n) % world
    g = C.c_void_p()
    dev = (C.c_int * world)(*([0] * world))
    assert L.lib.bh_create_group(C.byref(g), world, dev, n, None, None, 0) == 0
    try:
        F = L._F
        for q in range(world):
            ids = np.nonzero(owner == q)[0].astype(np.int32)
            arrs = [np.ascontiguousarray(a[ids]) for a in ic]
            assert L.lib.bh_rank_upload(L.lib.bh_group_rank(g, q), len(ids), *[a.ctypes.data_as(F) for a in arrs],
                                        ids.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        assert L.lib.bh_step_group(g, K) == 0 and L.lib.bh_group_sync(g) == 0
        st6 = [np.full(n, np.nan, np.float32) for _ in range(6)]
        assert L.lib.bh_group_download(g, *[a.ctypes.data_as(F) for a in st6]) == 0
        acc = [np.full(n, np.nan, np.float32) for _ in range(3)]
        assert L.lib.bh_group_download_acc(g, *[a.ctypes.data_as(F) for a in acc]) == 0
        info = L.BhRankInfo()
        counts = []
        for q in range(world):
            L.lib.bh_rank_get_info(L.lib.bh_group_rank(g, q), C.byref(info))
            counts.append(info.n_loc)
        assert info.mig_rounds >= 1                       # the first step's wave did not fit one X2 round
    finally:
        L.lib.bh_destroy_group(g)
    p, a = np.stack(st6[:3], 1), np.stack(acc, 1)
    assert np.isfinite(p).all() and sum(counts) == n
    assert np.abs(np.array(counts) - n / world).max() < 0.05 * n / world, counts
    p1, v1, a1 = single(ic, K)
    assert np.abs(p - p1).max() < 1e-3
    e = rel(a, a1)
    assert np.median(e) < 2e-6 and e.max() < 2e-3, (np.median(e), e.max())


def test_group_reupload_starts_from_scratch():
    """bh_group_upload / bh_dd_upload a second time: the boundaries, counts and drift estimate of the first run mean
    nothing for the new bodies (round-4 advisor finding: the splitter keys of the old run survived and classified the
    new bodies under a new cube) — the second run must be bit-identical to the same run in a fresh group."""
    import ctypes as C
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    n, world, K = 80_000, 4, 4
    ic1 = pkg.plummer(n, seed=2)
    ic2 = pkg.disc(n, seed=9)          # another distribution under another cube
    F = L._F

    def run(g, ic):
        assert L.lib.bh_group_upload(g, *[np.ascontiguousarray(a).ctypes.data_as(F) for a in ic]) == 0
        assert L.lib.bh_step_group(g, K) == 0 and L.lib.bh_group_sync(g) == 0
        out = [np.full(n, np.nan, np.float32) for _ in range(6)]
        assert L.lib.bh_group_download(g, *[a.ctypes.data_as(F) for a in out]) == 0
        return np.stack(out, 1)

    dev = (C.c_int * world)(*([0] * world))
    g = C.c_void_p()
    assert L.lib.bh_create_group(C.byref(g), world, dev, n, None, None, 0) == 0
    try:
        run(g, ic1)
        second = run(g, ic2)
        info = np.zeros(8, np.int32)
        L.lib.bh_dd_get_info(L.lib.bh_rank_ctx(L.lib.bh_group_rank(g, 0)), info.ctypes.data_as(C.POINTER(C.c_int32)))
    finally:
        L.lib.bh_destroy_group(g)
    g2 = C.c_void_p()
    assert L.lib.bh_create_group(C.byref(g2), world, dev, n, None, None, 0) == 0
    try:
        fresh = run(g2, ic2)
        info2 = np.zeros(8, np.int32)
        L.lib.bh_dd_get_info(L.lib.bh_rank_ctx(L.lib.bh_group_rank(g2, 0)), info2.ctypes.data_as(C.POINTER(C.c_int32)))
    finally:
        L.lib.bh_destroy_group(g2)
    assert np.isfinite(second).all()
    assert np.array_equal(second, fresh)
    assert info[2] == info2[2]          # steps in which the boundaries moved: counted from the second upload


def test_group_rank_local_failure_releases_the_other_ranks():
    """a rank that fails on its own AFTER the last exchange of a step (here: bh_group_upload never ran, so phase 1
    fails everywhere — and a group whose rank 1 alone was never given bodies) must not leave the other library
    threads waiting in an exchange: bh_step_group returns an error and the group reports BH_ERR_COMM afterwards"""
    import ctypes as C
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    n, world = 40000, 3
    ic = pkg.plummer(n, seed=1)
    g = C.c_void_p()
    dev = (C.c_int * world)(0, 0, 0)
    assert L.lib.bh_create_group(C.byref(g), world, dev, n, None, None, 2) == 0
    try:
        F = L._F
        ids = np.arange(n, dtype=np.int32)
        for q in (0, 2):     # rank 1 gets nothing: its first call fails with BH_ERR_ORDER, before any exchange
            lo, hi = q * n // world, (q + 1) * n // world
            arrs = [np.ascontiguousarray(a[lo:hi]) for a in ic]
            assert L.lib.bh_rank_upload(L.lib.bh_group_rank(g, q), hi - lo, *[a.ctypes.data_as(F) for a in arrs],
                                        ids[lo:hi].ctypes.data_as(C.POINTER(C.c_int32))) == 0
        st = L.lib.bh_step_group(g, 2)
        assert st not in (0, L.BH_ERR_DOMAIN_LEFT), st
        assert L.lib.bh_step_group(g, 1) == L.BH_ERR_COMM
    finally:
        L.lib.bh_destroy_group(g)


def test_dd_disc_initial_conditions():
    """the reference's thin rotating disc (ref:297-307): strongly anisotropic domains"""
    pkg = bhpkg.load()
    _check(pkg.disc(50000, seed=5), 4, 5)


def test_dd_coincident_bodies_and_zero_masses():
    """bodies at identical positions form unsplit multi-body cells (exported as blocks of body
    records), zero-mass bodies form records every traversal skips; both must survive the LET path"""
    pkg = bhpkg.load()
    n = 30000
    x, y, z, vx, vy, vz, m = [a.copy() for a in pkg.plummer(n, seed=9)]
    for lo, cnt in ((1000, 40), (17000, 150)):       # two clumps of identical positions
        x[lo:lo + cnt] = x[lo]
        y[lo:lo + cnt] = y[lo]
        z[lo:lo + cnt] = z[lo]
        vx[lo:lo + cnt] = vy[lo:lo + cnt] = vz[lo:lo + cnt] = 0.0
    m[5000:5200] = 0.0
    e = _check((x, y, z, vx, vy, vz, m), 3, 3)
    assert e.max() < 5e-3, e.max()


def test_dd_small_system_many_ranks():
    pkg = bhpkg.load()
    _check(pkg.plummer(8 * 1500, seed=2), 8, 4)


def test_dd_rank_failure_is_collective():
    """a rank whose context cannot hold its bodies after migration must not strand the other ranks in
    an all-gather: it keeps exchanging empty payloads, marks its LET segment, and every rank raises"""
    pkg = bhpkg.load()
    n = 200000
    ic = pkg.plummer(n, seed=4)
    with pytest.raises(Exception) as ei:
        run_ranks(4, ic, 6, slack=0.92)   # capacity 50,096 bodies per rank for ~50,000 +- 1 %
    assert "left the domain-decomposed step" in str(ei.value) or "overflow" in str(ei.value)


def test_dd_config4_full_size_8_ranks_x_1M(orc):
    """BASELINE config 4 (8,000,000 bodies on 8 GPUs) rehearsed on this one GPU: 8 ranks x 1M bodies in
    one process, 2 steps, against (a) the CPU oracle's step loop on the 8M bodies (ref:255-283 stage order; the
    bounds of test_fullsize_k_steps_vs_oracle's 8M case: |dx| max <= 4.9e-4, |dv| p99.99 <= 6.1e-5, max <= 4.3e-4)
    and (b) a single 8M-body context: same canonical octree, so the forces agree to summation order (the two-pass
    force adds the own and the remote part separately)."""
    pkg = bhpkg.load()
    n = 8_000_000
    ic = pkg.plummer(n, seed=42)
    p1, v1, a1 = single(ic, 2)
    out = run_ranks(8, ic, 2)
    p, v, a = merge(out, n)
    o = orc.Oracle(n)
    o.upload(*ic)
    o.step(2, order=orc.ORDER_BATCHED)
    w = np.stack(o.download(), 1)
    o.close()
    dx = np.abs(p.astype(np.float64) - w[:, :3]).max(axis=1)
    dv = np.abs(v.astype(np.float64) - w[:, 3:]).max(axis=1)
    print(f"8 ranks x 1M vs oracle, K=2: |dx| p50 {np.median(dx):.3e} p99.99 {np.percentile(dx, 99.99):.3e} "
          f"max {dx.max():.3e}; |dv| p50 {np.median(dv):.3e} p99.99 {np.percentile(dv, 99.99):.3e} max {dv.max():.3e}")
    assert np.median(dx) <= 3.1e-5 and np.percentile(dx, 99.99) <= 1.3e-4 and dx.max() <= 4.9e-4
    assert np.median(dv) <= 1e-6 and np.percentile(dv, 99.99) <= 6.1e-5 and dv.max() <= 4.3e-4
    del w, dx, dv
    assert sum(o[-1] for o in out) == n
    e = rel(a, a1)
    assert np.median(e) < 2e-6, np.median(e)
    assert np.quantile(e, 0.9999) < 1e-4, np.quantile(e, 0.9999)
    assert e.max() < 2e-3, e.max()
    assert np.abs(p - p1).max() < 1e-3
    # every rank ends within 2 % of its fair share and exports well under a third of its tree
    counts = np.array([o[-1] for o in out])
    assert np.abs(counts - n / 8).max() < 0.02 * n / 8, counts
    let = out[0][4]
    assert let.max() < 0.35 * 2 * n / 8, let


def test_dd_abi_argument_and_order_checks():
    """error behaviour of the bh_dd_* entry points: bad sizes, unsupported parameters, calls out of order"""
    import ctypes as C
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd._lib import lib, BhDdSizes
    from nbody_barnes_hut_cuda_amd.engine import BhError
    sz = BhDdSizes()
    assert lib.bh_dd_query(50000, 4, 4096, 100, C.byref(sz)) == -1          # let_cap below header + piece slots
    assert lib.bh_dd_query(50000, 65, 4096, 60000, C.byref(sz)) == -1       # more than 64 ranks
    assert lib.bh_dd_query(50000, 4, 4096, 60000, C.byref(sz)) == 0
    assert sz.seg_base > sz.top_base > 2 * 50000 and sz.pool_records > sz.seg_base + 4 * 60000
    pool = torch.zeros(sz.pool_records * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for bad in (dict(leaf_cap=4), dict(key_bits=30, max_depth=10), dict(strict_fp=1), dict(max_depth=6)):
        with pkg.Engine(50000, **bad) as e:                                 # needs 63-bit keys, leaf_cap 1, fast kernel
            with pytest.raises(BhError):
                e.dd_init(4, 0, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records)
    with pkg.Engine(50000) as e:
        with pytest.raises(BhError):
            e.dd_init(4, 4, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records)      # rank out of range
        with pytest.raises(BhError):
            e.dd_init(4, 0, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records - 1)  # pool too small
        e.dd_init(4, 0, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records)
        with pytest.raises(BhError):
            e.dd_init(4, 0, 200000, 4096, 60000, pool.data_ptr(), sz.pool_records)      # already initialised
        buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(BhError):
            e.dd_cube_pack(buf.data_ptr())                                  # nothing uploaded yet
        ic = pkg.plummer(40000, seed=1)
        e.dd_upload(*ic, np.arange(40000, dtype=np.int32))
        with pytest.raises(BhError):
            e.dd_migrate_pack(buf.data_ptr(), 1024)                         # before the cube exchange
        with pytest.raises(BhError):
            e.dd_let_pack(buf.data_ptr(), buf.data_ptr(), 1024)             # before the local tree
        with pytest.raises(BhError):
            e.dd_force()
        with pytest.raises(BhError):
            e.dd_upload(*pkg.plummer(60000, seed=1), np.arange(60000, dtype=np.int32))  # above the capacity


@pytest.mark.parametrize("how", ["pointer", "nan_threshold"])
def test_dd_malformed_let_record_is_closed_and_reported(how):
    """(how = nan_threshold: the record's opening threshold is NaN as well — the walk's `d2 > thr2` is then never
    true, so the record is ALWAYS opened; the validation must not mistake it for a closed one.)
    hang/fault safety of the first unattended multi-GPU run: a gathered LET record whose child block
    points outside its own segment is closed by the validation pass of bh_dd_top (never opened), the sticky
    flag BH_FLAG_DD_LET_INVALID is raised, bh_sync returns BH_ERR_DEVICE_FLAG, and the next step's
    bh_dd_migrate_apply refuses to go on.  (The corrupted pointer stays inside the pool, so even a missing
    check could not fault the box.)"""
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    n, world = 60000, 2
    ic = pkg.plummer(n, seed=7)
    order = bhdist.global_morton_order(pkg, ic, 0)
    group = bhdist.LocalGroup(world)
    stream = torch.cuda.Stream(0)
    res, errs = [None] * world, []

    group.slots = [None] * world

    class CorruptingComm(bhdist.TensorComm):   # the caller-callback transport: device copies done here, in Python
        hits = 0

        def __init__(self, group, rank):
            super().__init__(group.world, rank)
            self.g = group

        def all_gather(self, out, send):
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel()
            o = out.view(-1)
            for q in range(self.world):
                o[q * k:(q + 1) * k].copy_(g.slots[q].view(-1))
            if self.rank == 0 and k % 64 == 0:      # X4 (the only payload that is whole 64-byte digest pairs)
                self._corrupt(o[k:2 * k])
            g.barrier.wait()

        def all_to_all(self, out, send):             # X4 of the per-destination flavour
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel() // self.world
            o = out.view(-1)
            for q in range(self.world):
                o[q * k:(q + 1) * k].copy_(g.slots[q].view(-1)[self.rank * k:(self.rank + 1) * k])
            if self.rank == 0:
                self._corrupt(o[k:2 * k])
            g.barrier.wait()

        def _corrupt(self, segbytes):
            if True:
                seg = segbytes.view(torch.int32).view(-1, 16)             # rank 1's segment as rank 0 holds it, a row per pair
                thr = seg.view(torch.float32)[:, 8]
                cand = torch.nonzero((thr[300:] >= 0) & (seg[300:, 12] > 0))  # an openable record of the block area
                if len(cand) > 0:   # (a segment sent closed because it did not fit carries no blocks: wait for the retry)
                    seg[300 + int(cand[0]), 10] = 2                       # child block -> the local tree's first block
                    if how == "nan_threshold":
                        seg.view(torch.float32)[300 + int(cand[0]), 8] = float("nan")
                    CorruptingComm.hits += 1

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = CorruptingComm(group, r)
            st = bhdist.DomainStepper(pkg, ic, comm, 0, stream=stream, order=order)
            group.barrier.wait()
            st.step(1)
            status = 0
            try:
                st.e.sync()
            except pkg.BhError as ex:
                status = ex.status
            flags = st.e.stats().status_flags
            nxt = None
            if r == 0:
                try:
                    # the next step would stop at the migration phase: drive that entry point alone
                    st.e.dd_cube_pack(st.x1s.data_ptr())
                except pkg.BhError as ex:  # pragma: no cover - cube_pack itself does not check flags
                    nxt = ex.status
            res[r] = (status, flags, nxt)
            group.barrier.wait()
            st.close()
        except BaseException as ex:  # noqa: BLE001
            errs.append((r, ex))
            group.abort()
            group.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0][1]
    assert CorruptingComm.hits >= 1
    assert res[0][0] == -8 and res[0][1] & 64, res        # BH_ERR_DEVICE_FLAG, BH_FLAG_DD_LET_INVALID
    assert res[1] [0] == 0 and res[1][1] == 0, res        # the other rank saw well-formed segments


def test_transport_self_check_passes_on_the_hub_and_catches_a_misdelivering_transport():
    """bh_comm_check (what bench.py / bh_create_group run before the first step over RCCL): known words through
    one all-gather and one all-to-all.  The in-process hub with 3 ranks passes; a caller-callback transport whose
    all-to-all delivers chunk `rank + 1` instead of chunk `rank` returns BH_ERR_COMM (-9) on every rank."""
    import ctypes as C
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    L = pkg._lib
    world = 3
    group = bhdist.LocalGroup(world)
    res = {}

    def hub_rank(r):
        torch.cuda.set_device(0)
        c = bhdist.LocalComm(group, r).bh_comm()
        res["hub", r] = L.lib.bh_comm_check(C.byref(c))
        c.release(c.user)

    th = [threading.Thread(target=hub_rank, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert [res["hub", r] for r in range(world)] == [0] * world

    # a transport built from plain callbacks on raw pointers (no tensor registry): copies by hipMemcpy through torch
    slots, bar = [None] * world, threading.Barrier(world)

    def view(ptr, nbytes):
        return torch.as_tensor(_DevBytes(ptr, nbytes), device="cuda:0")

    def make(r, shift):
        def ag(user, recv, send, nb, st):
            torch.cuda.synchronize()   # (the check's own stream does not order with torch's)
            slots[r] = view(send, nb * world)
            bar.wait()
            out = view(recv, nb * world)
            for q in range(world):
                out[q * nb:(q + 1) * nb].copy_(slots[q][:nb])
            torch.cuda.synchronize()
            bar.wait()
            return 0

        def a2a(user, recv, send, nb, st):
            torch.cuda.synchronize()
            slots[r] = view(send, nb * world)
            bar.wait()
            out = view(recv, nb * world)
            me = (r + shift) % world
            for q in range(world):
                out[q * nb:(q + 1) * nb].copy_(slots[q][me * nb:(me + 1) * nb])
            torch.cuda.synchronize()
            bar.wait()
            return 0
        fa, fb = L.COMM_FN(ag), L.COMM_FN(a2a)
        return L.BhComm(world, r, None, fa, fb, L.COMM_RELEASE_FN()), (fa, fb)

    for shift, want in ((0, 0), (1, -9)):
        def cb_rank(r, shift=shift):
            torch.cuda.set_device(0)
            c, keep = make(r, shift)
            res[shift, r] = L.lib.bh_comm_check(C.byref(c))
        th = [threading.Thread(target=cb_rank, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert [res[shift, r] for r in range(world)] == [want] * world


class _DevBytes:
    """a raw device range as something torch.as_tensor accepts (__cuda_array_interface__)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2}


def test_replayed_force_phase_leaves_the_run_as_it_was():
    """bh_rank_replay_force_phase (measurement: the last step's LET kernels, an idle wave for X4, validation, top
    trees and force passes run again on the rank's own two streams, without integration) returns a positive time for
    every form — also the two-pass forms on ranks that step with one pass — and the run continues bit for bit as if
    it had not been called: 3 ranks x 20,000 bodies, 3 steps, replays, 2 steps == 5 steps."""
    import ctypes as C
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    n, world = 60000, 3
    ic = pkg.plummer(n, seed=5)
    F = L._F

    def run(replay):
        g = C.c_void_p()
        dev = (C.c_int * world)(*([0] * world))
        assert L.lib.bh_create_group(C.byref(g), world, dev, n, None, None, 0) == 0
        try:
            assert L.lib.bh_group_upload(g, *[np.ascontiguousarray(a).ctypes.data_as(F) for a in ic]) == 0
            ms = C.c_float()
            # before any step there is nothing to replay
            assert L.lib.bh_rank_replay_force_phase(L.lib.bh_group_rank(g, 0), 0, 0, 0, 1, C.byref(ms)) == -6  # BH_ERR_ORDER
            assert L.lib.bh_step_group(g, 3) == 0 and L.lib.bh_group_sync(g) == 0
            times = []
            if replay:
                for q in range(world):
                    for split, pct, us in ((0, 0, 0), (1, 20, 0), (1, 100, 50), (0, 0, 100)):
                        assert L.lib.bh_rank_replay_force_phase(L.lib.bh_group_rank(g, q), split, pct, us, 2, C.byref(ms)) == 0
                        times.append((split, pct, us, ms.value))
                assert L.lib.bh_rank_replay_force_phase(L.lib.bh_group_rank(g, 0), 1, 0, 0, 1, C.byref(ms)) == -1  # bad pct
            assert L.lib.bh_step_group(g, 2) == 0 and L.lib.bh_group_sync(g) == 0
            st6 = [np.full(n, np.nan, np.float32) for _ in range(6)]
            assert L.lib.bh_group_download(g, *[a.ctypes.data_as(F) for a in st6]) == 0
            acc = [np.full(n, np.nan, np.float32) for _ in range(3)]
            assert L.lib.bh_group_download_acc(g, *[a.ctypes.data_as(F) for a in acc]) == 0
            return st6 + acc, times
        finally:
            L.lib.bh_destroy_group(g)

    a, times = run(True)
    b, _ = run(False)
    assert all(t[3] > 0.0 for t in times)
    # an idle wave of 100 us in the place of X4 shows in the one-pass form
    one = [t[3] for t in times if t[0] == 0]
    assert all(one[2 * q + 1] > one[2 * q] + 0.05 for q in range(world))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("split", [False, True])
def test_let_that_outgrows_its_stride_is_exchanged_again_and_the_held_back_launches_do_no_harm(split):
    """The force launches of a step are enqueued BEFORE the host has read the X4 headers; the validation kernel takes
    the fit decision on the device (bh_devinfo.dd_hold) and a launch behind an exchange that does not fit returns at
    once.  theta = 0.2 with 2 ranks x 30,000 bodies needs several times the first stride (516 + capacity / 8): the
    first step must repeat X4 (let_retries >= 1 on every rank, the same number) — one pass and the two-pass form, whose
    own pass runs once — and still give the single-context step's forces and positions."""
    pkg = bhpkg.load()
    n, world = 60000, 2
    ic = pkg.plummer(n, seed=11)
    p1, v1, a1 = single(ic, 2, theta=0.2)
    out = run_ranks(world, ic, 2, split=split, theta=0.2)
    retries = [o[5] for o in out]
    assert retries[0] >= 1 and len(set(retries)) == 1, retries
    p, v, a = merge(out, n)
    e = rel(a, a1)
    assert np.median(e) < 5e-6, np.median(e)
    assert np.quantile(e, 0.9999) < 2e-4, np.quantile(e, 0.9999)
    assert np.abs(p - p1).max() < 2e-3


def stream_comm(group, rank, repeat_delay=0.05):
    """a caller-callback transport (dist.TensorComm) for in-process ranks: the copies are enqueued on the ranks' stream
    (TensorComm._call) and nothing waits for the device, so the ranks run NOT serial — the own-pieces passes go to the
    device's side stream — and the kernels of the step are still running while an exchange is made.  A repeated X4 (a
    second all-to-all before the next step's all-gathers) first waits `repeat_delay` seconds on the host: a larger
    exchange over a slow link."""
    from nbody_barnes_hut_cuda_amd import dist as bhdist

    class StreamComm(bhdist.TensorComm):
        def __init__(self):
            super().__init__(group.world, rank)
            self.g = group
            self.x4_this_step = 0

        def all_gather(self, out, send):
            self.x4_this_step = 0      # X1 .. X3: a new step has begun
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel()
            o = out.view(-1)
            for q in range(self.world):
                o[q * k:(q + 1) * k].copy_(g.slots[q].view(-1))
            g.barrier.wait()

        def all_to_all(self, out, send):   # X4 (per-destination segments)
            if self.x4_this_step > 0:
                time.sleep(repeat_delay)
            self.x4_this_step += 1
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel() // self.world
            o = out.view(-1)
            for q in range(self.world):
                o[q * k:(q + 1) * k].copy_(g.slots[q].view(-1)[self.rank * k:(self.rank + 1) * k])
            g.barrier.wait()

    return StreamComm()


@pytest.mark.parametrize("pct", [100, 30])
def test_x4_repeated_while_the_own_pass_runs_on_the_side_stream(pct):
    """The own-pieces pass of a two-pass step is launched on the side stream behind the LET export and needs nothing
    from X4; the validation kernel behind X4 raises bh_devinfo.dd_hold when the exchange does not fit, and the repeat
    does not launch the own pass again.  So the own pass must not be held: a group of it dispatched while the hold is
    up would leave its bodies without their own-pieces accelerations.  4 ranks x 500,000 bodies, theta = 0.2, split
    form (pct per cent of a rank's bodies in two passes), over a transport that leaves the ranks not serial: the own
    passes of the four ranks queue on the one side stream, far more waves than the GPU runs at once, and the repeated
    X4 takes 50 ms, so passes are dispatched while the hold is up.  The first step must repeat X4 (the same number of
    times on every rank) and give the single-context step's forces and positions; the second step is checked from the
    same state (check_last_step)."""
    pkg = bhpkg.load()
    n, world = 2_000_000, 4
    ic = pkg.plummer(n, seed=17)
    p1, v1, a1 = single(ic, 1, theta=0.2)
    first = []
    out = run_ranks(world, ic, 2, comm=stream_comm, before_last=first, split=True, split_pct=pct, theta=0.2)
    retries = [f[4] for f in first]
    print(f"split_pct {pct}: X4 repeats in the first step {retries}, after two steps {[o[5] for o in out]}; "
          f"last LET counts of rank 0 {out[0][4].tolist()}")
    assert retries[0] >= 1 and len(set(retries)) == 1, retries
    p, v, a = merge(first, n)
    e = rel(a, a1)
    print(f"first step vs single context: acc rel median {np.median(e):.2e} p99.99 {np.quantile(e, 0.9999):.2e} "
          f"max {e.max():.2e}; |dpos| max {np.abs(p - p1).max():.2e}; |dvel| max {np.abs(v - v1).max():.2e}; "
          f"bodies off by > 1e-3: {int((e > 1e-3).sum())}")
    # theta = 0.2: the retry test's median and p99.99 bounds; max measured on MI355X 9.0e-5 (first step) and 1.06e-4
    # (second step), bound ~5x that.  Against the parent commit's library (own-pass groups held): p99.99 7.05 / 4.51,
    # 692,672 / 449,536 bodies off by more than 1e-3 (split_pct 100 / 30)
    assert np.median(e) < 5e-6, np.median(e)
    assert np.quantile(e, 0.9999) < 2e-4, np.quantile(e, 0.9999)
    assert e.max() < 5e-4, e.max()
    assert np.abs(p - p1).max() < 1e-3
    check_last_step(out, first, ic, acc=(5e-6, 2e-4, 5e-4), theta=0.2)


def test_x4_with_a_size_per_pair_moves_a_fraction_of_the_slots_and_changes_nothing():
    """bh_comm.all_to_all_v (ABI 6): after the first step every pair's transfer follows what the pair needed in the last
    fitting exchange (x4_chunk: a quarter more + 4096 records) instead of the whole slot.  4 ranks x 50,000 bodies, 6
    steps, through the in-process hub (sized exchange) and through a caller-callback transport that has no sized
    exchange (whole slots): the same bits for every body, and the hub ranks receive clearly fewer bytes than the slots hold
    (two thirds of them at this size — the 4096-record margin weighs on small segments; a third at 8 x 1M, tools/dd_needs.py)."""
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    n, world, steps = 200000, 4, 6
    ic = pkg.plummer(n, seed=9)
    order = bhdist.global_morton_order(pkg, ic, 0)

    class SlotComm(bhdist.TensorComm):   # device copies in Python; all_to_all_v stays NULL
        def __init__(self, group, rank):
            super().__init__(group.world, rank)
            self.g = group

        def all_gather(self, out, send):
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel()
            for q in range(self.world):
                out.view(-1)[q * k:(q + 1) * k].copy_(g.slots[q].view(-1))
            torch.cuda.synchronize()
            g.barrier.wait()

        def all_to_all(self, out, send):
            g = self.g
            g.slots[self.rank] = send
            g.barrier.wait()
            k = send.numel() // self.world
            for q in range(self.world):
                out.view(-1)[q * k:(q + 1) * k].copy_(g.slots[q].view(-1)[self.rank * k:(self.rank + 1) * k])
            torch.cuda.synchronize()
            g.barrier.wait()

    def run(kind, before=None):
        group = bhdist.LocalGroup(world)
        group.slots = [None] * world
        stream = torch.cuda.Stream(0)
        out, errs = [None] * world, []

        def work(r):
            try:
                torch.cuda.set_device(0)
                comm = bhdist.LocalComm(group, r) if kind == "hub" else SlotComm(group, r)
                st = bhdist.DomainStepper(pkg, ic, comm, 0, stream=stream, order=order)
                group.barrier.wait()
                if before is not None:
                    st.step(steps - 1)
                    before[r] = st.local_state()
                    st.step(1)
                else:
                    st.step(steps)
                st._sync_info()
                out[r] = st.local_state() + (st.x4_recv_bytes, st.stride, st.let_retries)
                group.barrier.wait()
                st.close()
            except BaseException as ex:  # noqa: BLE001
                errs.append(ex)
                group.abort()
                group.barrier.abort()

        th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        if errs:
            raise errs[0]
        return out

    before = [None] * world
    a, b = run("hub", before), run("slots")
    pa, va, aa = merge([o[:4] for o in a], n)
    pb, vb, ab = merge([o[:4] for o in b], n)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and np.array_equal(aa, ab)
    check_last_step([o[:4] for o in a], before, ic)
    for r in range(world):
        sized, slots = a[r][4], b[r][4]
        assert slots == world * b[r][5] * 32 or b[r][6] > 0      # whole slots (the stride the step used, unless repeated)
        assert sized < 0.8 * slots, (r, sized, slots)
    print("X4 bytes received per rank, sized / slots:", [(o[4], p[4]) for o, p in zip(a, b)])
