"""Energy diagnostics of the domain-decomposed step (bh_rank_step_energy, bh_step_group_energy, dist.DomainStepper
.step_energy / download_potential) on ONE GPU: P ranks as P threads of this process (dist.LocalComm, the library's
in-process transport), as tests/test_gpu_dd.py runs them.

An energy step is a real step that also measures the state it starts from, by one walk of the whole stitched tree.  So
its sums and potentials are checked against bh_energy of one context holding the same state (tests/potential_ref.py for
the per-body bound of the potentials), its bits against those of every other force form and every rank, and the run
against the same run with plain steps, bit for bit."""
import json
import os
import re
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

import bhpkg
from helpers import TIE_MARGIN, oparams
from potential_ref import phi_bound, potential_f64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 60_000
SUM_KEYS = ("kinetic", "potential", "total", "mass", "momentum", "angular_momentum", "com", "n")
FORMS = {"one": dict(split=False), "split30": dict(split=True, split_pct=30), "split100": dict(split=True, split_pct=100)}
# Population limits of the potentials against the fp64 walk of the single context's tree: those of
# tests/test_gpu_energy.py (PHI_MED, PHI_P9999, TIE_PHI_REL) — the stitched tree is the same canonical octree
PHI_MED, PHI_P9999, TIE_PHI_REL = 2.9e-6, 1.7e-5, 1.4e-5
SAME_INPUTS_REL = 1e-12   # M, K, P, L, COM: the same fp32 inputs summed in another order
# |W - W_single| / |W|: twice the largest MI355X figure the checks print — 3.75e-12 at theta 0.2 (60,000 bodies, X4
# repeated), at most 1.4e-16 at theta 0.5; M, K, P, L and COM measured at most 1.4e-16
W_REL = 7.5e-12


def _ic(seed=3, n=N):
    return bhpkg.load().plummer(n, seed=seed)


def run_energy_ranks(world, ic, schedule, comm=None, order=None, **kw):
    """every rank steps through `schedule` ("p": a plain step, "e": an energy step) on its own thread; per rank:
    dict(energies=[...], phis=[(ids, phi), ...], state=local_state(), retries, flags, bad=...)"""
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    if order is None:
        order = bhdist.global_morton_order(pkg, ic, 0)
    group = bhdist.LocalGroup(world)
    group.slots = [None] * world
    stream = torch.cuda.Stream(0)
    out, errs = [None] * world, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            st = bhdist.DomainStepper(pkg, ic, (comm or bhdist.LocalComm)(group, r), 0, stream=stream, order=order,
                                      **kw)
            group.barrier.wait()
            res = dict(energies=[], phis=[])
            for k in schedule:
                if k == "e":
                    res["energies"].append(st.step_energy())
                    res["phis"].append(st.download_potential())
                else:
                    st.step(1)
            res["state"] = st.local_state()
            res["retries"] = st.let_retries
            res["flags"] = st.e.stats().status_flags
            out[r] = res
            group.barrier.wait()
            st.close()
        except BaseException as ex:  # noqa: BLE001 - report from the main thread
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
    return out


def _phi_caller(out, n, k=0):
    """the k-th energy step's potentials of every rank, caller order"""
    phi = np.full(n, np.nan, np.float32)
    seen = np.zeros(n, np.int32)
    for o in out:
        ids, p = o["phis"][k]
        phi[ids] = p
        seen[ids] += 1
    assert (seen == 1).all(), "every body's potential exactly once"
    return phi


def _state_of(out, n):
    posm = np.zeros((n, 4), np.float32)
    vel = np.zeros((n, 3), np.float32)
    for o in out:
        ids, pm, v, _ = o["state"]
        posm[ids] = pm
        vel[ids] = v
    return tuple(np.ascontiguousarray(c) for c in (*posm[:, :3].T, *vel.T, posm[:, 3]))


def _bits(d):
    return json.dumps({k: d[k] for k in SUM_KEYS}, sort_keys=True)


def _same_on_every_rank(out, k=0):
    b = {_bits(o["energies"][k]) for o in out}
    assert len(b) == 1, b
    return out[0]["energies"][k]


_REF = {}


def single_reference(ic, key, theta=0.5, every=6):
    """bh_energy of one context holding the state, its potentials (caller order) and, on a sample of bodies, the fp64
    walk of its tree with the per-body bound and the tie margin"""
    if key in _REF:
        return _REF[key]
    import oracle as O
    pkg = bhpkg.load()
    n = len(ic[0])
    e = pkg.Engine(n, theta=theta)
    e.upload(*ic)
    st = e.energy()
    phi = e.download_potential()
    order = e.download_order()
    rec = e.download_tree()
    xyzm = e.download_sorted_bodies()
    p = e.params
    idx = np.unique(np.concatenate([np.arange(0, n, every), np.arange(0, 64), np.arange(n - 64, n)])).astype(np.int32)
    O.build()
    f = O.force_f64(rec, xyzm, oparams(O, p), idx=idx)
    ref = potential_f64(rec, xyzm, p.G, p.theta, p.eps2, idx=f["idx"])
    e.close()
    _REF[key] = dict(st=st, phi=phi, order=order, sorted_idx=f["idx"], caller=order[f["idx"]], ref=ref["phi"],
                     bound=phi_bound(ref["k"], ref["sabs"]), nontie=f["margin"] >= TIE_MARGIN)
    return _REF[key]


def check_against_single(en, phi, R, label):
    """sums and potentials of a decomposed energy step against the single context's (R = single_reference)"""
    s = R["st"]
    assert en["n"] == s["n"], (en["n"], s["n"])
    fig = {}
    for k in ("mass", "kinetic"):
        fig[k] = abs(en[k] - s[k]) / abs(s[k])
        assert fig[k] <= SAME_INPUTS_REL, (label, k, en[k], s[k])
    for k, scale in (("momentum", R["pscale"]), ("angular_momentum", R["lscale"])):
        d = np.abs(np.array(en[k]) - np.array(s[k])).max() / scale
        fig[k] = float(d)
        assert d <= SAME_INPUTS_REL, (label, k, en[k], s[k], scale)
    d = np.abs(np.array(en["com"]) - np.array(s["com"])).max() / R["xscale"]
    fig["com"] = float(d)
    assert d <= SAME_INPUTS_REL, (label, "com", en["com"], s["com"])
    fig["W"] = abs(en["potential"] - s["potential"]) / abs(s["potential"])
    assert abs(en["total"] - (en["kinetic"] + en["potential"])) <= 1e-12 * abs(en["potential"])
    # per body, on the sample: the per-body bound for the non-tie bodies, the tie limit for the others
    got = phi[R["caller"]].astype(np.float64)
    assert np.isfinite(phi).all(), label
    err = np.abs(got - R["ref"])
    rel = err / np.abs(R["ref"])
    nt = R["nontie"]
    fig.update(ratio_max=float((err[nt] / R["bound"][nt]).max()), med=float(np.median(rel[nt])),
               p9999=float(np.quantile(rel[nt], 0.9999)), tie_max=float(rel[~nt].max()) if (~nt).any() else 0.0,
               tie_frac=float((~nt).mean()))
    print(f"{label}: M {fig['mass']:.1e} K {fig['kinetic']:.1e} P {fig['momentum']:.1e} L {fig['angular_momentum']:.1e} "
          f"COM {fig['com']:.1e} | W rel {fig['W']:.2e} | phi err/bound max {fig['ratio_max']:.3f} rel p50 "
          f"{fig['med']:.2e} p99.99 {fig['p9999']:.2e} ties {fig['tie_frac']:.2%} max {fig['tie_max']:.2e}")
    assert fig["W"] <= W_REL, (label, fig)
    assert not (nt & (err > R["bound"])).any(), (label, fig)
    assert fig["med"] <= PHI_MED and fig["p9999"] <= PHI_P9999, (label, fig)
    assert fig["tie_frac"] <= 0.05 and fig["tie_max"] <= TIE_PHI_REL, (label, fig)
    return fig


def _scales(R, ic):
    x, y, z, vx, vy, vz, m = [np.asarray(a, np.float64) for a in ic]
    sp = np.sqrt(vx * vx + vy * vy + vz * vz)
    r = np.sqrt(x * x + y * y + z * z)
    R["pscale"] = float((np.abs(m) * sp).sum())         # sum m |v|: P's terms
    R["lscale"] = float((np.abs(m) * r * sp).sum())     # sum m |x| |v|: L's terms
    R["xscale"] = float((np.abs(m) * r).sum() / np.abs(m).sum())


# ------------------------------------------------------------------ 1 + 3: the first step, every form, every rank
@pytest.mark.parametrize("let_mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_first_energy_step_matches_the_single_context_in_every_form(world, let_mode):
    ic = _ic()
    R = single_reference(ic, "first")
    _scales(R, ic)
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    order = bhdist.global_morton_order(bhpkg.load(), ic, 0)
    got = {}
    for form, kw in FORMS.items():
        out = run_energy_ranks(world, ic, "e", order=order, let_mode=let_mode, **kw)
        assert all(o["flags"] == 0 for o in out)
        en = _same_on_every_rank(out)
        phi = _phi_caller(out, N)
        check_against_single(en, phi, R, f"world {world} let_mode {let_mode} {form}")
        got[form] = (_bits(en), phi)
    # phi and the sums do not depend on the force form
    ref_bits, ref_phi = got["one"]
    for form, (b, phi) in got.items():
        assert b == ref_bits, (form, b, ref_bits)
        assert np.array_equal(phi.view(np.int32), ref_phi.view(np.int32)), form


# ------------------------------------------------------------------ 2: an energy step after K plain steps
@pytest.mark.parametrize("form", ["one", "split30"])
def test_energy_step_after_plain_steps_matches_the_single_context_of_that_state(form):
    K = 6
    ic = _ic(seed=8)
    before = run_energy_ranks(3, ic, "p" * K, let_mode=1, **FORMS[form])
    state = _state_of(before, N)
    out = run_energy_ranks(3, ic, "p" * K + "e", let_mode=1, **FORMS[form])
    R = single_reference(state, ("later", form))
    _scales(R, state)
    en = _same_on_every_rank(out)
    check_against_single(en, _phi_caller(out, N), R, f"after {K} steps, {form}")


# ------------------------------------------------------------------ 3c: the run is not perturbed
@pytest.mark.parametrize("form", ["one", "split30", "split100"])
@pytest.mark.parametrize("let_mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_energy_steps_leave_the_run_bit_for_bit_as_it_was(world, let_mode, form):
    K = 5
    ic = _ic(seed=21, n=30_000)
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    order = bhdist.global_morton_order(bhpkg.load(), ic, 0)
    plain = run_energy_ranks(world, ic, "p" * K, order=order, let_mode=let_mode, **FORMS[form])
    sched = "".join("e" if s in (1, 3, K) else "p" for s in range(1, K + 1))
    meas = run_energy_ranks(world, ic, sched, order=order, let_mode=let_mode, **FORMS[form])
    for a, b in zip(plain, meas):
        for x, y in zip(a["state"], b["state"]):
            assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32))
    for k in range(3):
        _same_on_every_rank(meas, k)
    e = [meas[0]["energies"][k]["total"] for k in range(3)]
    print(f"world {world} let_mode {let_mode} {form}: E at steps 1, 3, {K}: {e}")


# ------------------------------------------------------------------ 4: an X4 that has to be repeated
def _retry_case(comm, split):
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    n = 60000
    ic = bhpkg.load().plummer(n, seed=11)
    R = single_reference(ic, "theta0.2", theta=0.2)
    _scales(R, ic)
    kw = dict(split=True, split_pct=30) if split else dict(split=False)
    out = run_energy_ranks(2, ic, "e", comm=comm, theta=0.2, let_mode=1, **kw)
    retries = [o["retries"] for o in out]
    assert retries[0] >= 1 and len(set(retries)) == 1, retries
    assert all(o["flags"] == 0 for o in out)
    en = _same_on_every_rank(out)
    check_against_single(en, _phi_caller(out, n), R, f"theta 0.2, X4 repeated {retries[0]}x, "
                                                     f"{'split' if split else 'one pass'} {comm is not None}")
    return out


@pytest.mark.parametrize("split", [False, True])
def test_energy_step_whose_x4_is_repeated(split):
    _retry_case(None, split)


def test_energy_step_whose_x4_is_repeated_with_the_own_pass_on_the_side_stream():
    from test_gpu_dd import stream_comm
    _retry_case(stream_comm, True)


# ------------------------------------------------------------------ 5: error paths and the group entry points
def test_energy_error_paths_of_a_rank():
    import ctypes as C
    import torch
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import _lib as L
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    ic = _ic(n=20_000)
    group = bhdist.LocalGroup(1)
    st = bhdist.DomainStepper(pkg, ic, bhdist.LocalComm(group, 0), 0, stream=torch.cuda.Stream(0))
    ctx = L.lib.bh_rank_ctx(st._h)
    phi = np.zeros(st.e.n, np.float32)
    es = L.BhEnergyStats()
    assert L.lib.bh_dd_download_potential(ctx, phi.ctypes.data_as(L._F)) == -6   # before the first energy step
    assert L.lib.bh_dd_download_potential(ctx, None) == -1
    assert L.lib.bh_rank_step_energy(st._h, None) == -1
    assert L.lib.bh_rank_step_energy(None, C.byref(es)) == -1
    st.step(1)
    assert L.lib.bh_dd_download_potential(ctx, phi.ctypes.data_as(L._F)) == -6
    en = st.step_energy()
    assert en["n"] == 20_000 and en["kinetic"] > 0 > en["potential"]
    ids, p = st.download_potential()
    assert np.isfinite(p).all() and len(ids) == st.n_loc
    # the single-context entry points keep refusing a rank's context
    assert L.lib.bh_energy(ctx, C.byref(es)) == -1
    assert L.lib.bh_download_potential(ctx, phi.ctypes.data_as(L._F)) == -6
    st.step(1)    # a later plain step invalidates the potentials
    assert L.lib.bh_dd_download_potential(ctx, phi.ctypes.data_as(L._F)) == -6
    st.close()


def test_group_energy_step_and_potentials_in_caller_order():
    import ctypes as C
    from nbody_barnes_hut_cuda_amd import _lib as L
    ic = _ic()
    R = single_reference(ic, "first")
    _scales(R, ic)
    g = C.c_void_p()
    dev = (C.c_int * 3)(0, 0, 0)
    assert L.lib.bh_create_group(C.byref(g), 3, dev, N, None, None, 0) == 0
    try:
        arrs = [np.ascontiguousarray(a, np.float32) for a in ic]
        assert L.lib.bh_group_upload(g, *[a.ctypes.data_as(L._F) for a in arrs]) == 0
        phi = np.full(N, np.nan, np.float32)
        assert L.lib.bh_group_download_potential(g, phi.ctypes.data_as(L._F)) == -6
        es = L.BhEnergyStats()
        assert L.lib.bh_step_group_energy(g, C.byref(es)) == 0
        assert L.lib.bh_step_group_energy(g, None) == -1 and L.lib.bh_step_group_energy(None, C.byref(es)) == -1
        assert L.lib.bh_group_download_potential(g, None) == -1
        assert L.lib.bh_group_download_potential(g, phi.ctypes.data_as(L._F)) == 0
        assert np.isfinite(phi).all()            # every body's phi, once (NaN where none was written)
        en = dict(kinetic=es.kinetic, potential=es.potential, total=es.total, mass=es.mass,
                  momentum=tuple(es.momentum), angular_momentum=tuple(es.angular_momentum), com=tuple(es.com), n=es.n)
        check_against_single(en, phi, R, "bh_step_group_energy, 3 ranks (C)")
        assert L.lib.bh_step_group(g, 1) == 0
        assert L.lib.bh_group_download_potential(g, phi.ctypes.data_as(L._F)) == -6
    finally:
        L.lib.bh_destroy_group(g)


# ------------------------------------------------------------------ multi-process: each rank with its own streams
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("let_mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_energy_step_multiprocess_same_bits_as_in_process(world, let_mode, tmp_path):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = tmp_path / "en.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dd_energy_worker.py"), str(out), str(N), str(let_mode)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    res = json.loads(out.read_text())
    assert len(res) == world and len(set(res)) == 1, res    # every process the same bits
    ip = run_energy_ranks(world, _ic(), "e", let_mode=let_mode, split=False)
    assert res[0] == _bits(_same_on_every_rank(ip)), (res[0], _bits(ip[0]["energies"][0]))


# ------------------------------------------------------------------ bh_bench --energy on the multi-GPU step
BENCH = os.path.join(ROOT, "nbody-barnes-hut-cuda_amd", "bh_bench")
LINE = re.compile(r"^energy step (\d+) K (\S+) W (\S+) E (\S+) dE/\|E0\| (\S+)$", re.M)
FRAME = re.compile(r"^\d+\s+\|\s+[0-9.]+\s+\|\s+[0-9.]+\s*$", re.M)
# |E_group - E_single| / |E| per line: measured 0 on MI355X at the line's ten significant digits — the bound is that
# resolution
BENCH_E_REL = 1e-9


def _bench(*args):
    r = subprocess.run([BENCH, "--n", "65536", "--steps", "20", "--ic", "plummer", *args], cwd=ROOT, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_bh_bench_energy_lines_of_the_multi_gpu_step():
    grp = _bench("--devices", "0,0", "--energy", "5")
    one = _bench("--energy", "5")
    plain = _bench("--devices", "0,0")
    g = [tuple(float(v) for v in m.groups()) for m in LINE.finditer(grp)]
    s = [tuple(float(v) for v in m.groups()) for m in LINE.finditer(one)]
    assert [int(x[0]) for x in g] == [5, 10, 15, 20], grp
    assert len(FRAME.findall(grp)) == 20
    worst = 0.0
    for (st, K, W, E, _), (st1, K1, W1, E1, _) in zip(g, s):
        assert st == st1 and K > 0 > W and abs(E - (K + W)) <= 1e-8 * abs(W)
        worst = max(worst, abs(E - E1) / abs(E1))
    print(f"bh_bench --energy 5, 2 ranks vs one context: |dE|/|E| max {worst:.2e}")
    assert worst <= BENCH_E_REL
    assert re.search(r"^energy: 4 of 20 frames measured the energy; the other 16 frames avg [0-9.]+ ms/step$", grp, re.M)
    # without --energy: the lines of today's output, none of the new ones
    assert not LINE.search(plain) and "frames measured" not in plain and len(FRAME.findall(plain)) == 20
    def shape(text):
        return [" ".join(re.sub(r"[0-9.e+-]+", "#", l).split()) for l in text.splitlines() if not l.startswith("energy")]
    assert shape(plain) == shape(grp)
