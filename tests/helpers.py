"""Shared helpers for the parity tests: run the oracle pipeline stage by stage."""
import numpy as np


def oracle_pipeline(O, ic, p):
    """Oracle stages on caller-order arrays -> dict of every intermediate."""
    x, y, z, vx, vy, vz, m = ic
    b = O.bbox(x, y, z)
    k = O.keys(x, y, z, b, p.key_bits, p.key_curve)
    sk, perm = O.sort(k)
    xyzm = np.stack([x, y, z, m], 1)[perm].astype(np.float32)
    vel = np.stack([vx, vy, vz], 1)[perm].astype(np.float32)
    rec, lo, hi, ni, ml = O.build_tree(sk, p, O.root_edge(b))
    rec = O.com(rec, lo, hi, xyzm)
    return dict(bounds=b, keys=k, sorted_keys=sk, perm=perm, xyzm=xyzm, vel=vel, rec=rec, er_lo=lo,
                er_hi=hi, n_internal=ni, max_level=ml)


def key_curve_of(gp):
    """the curve an engine with these bh_params orders its keys by (30-bit keys are always Morton)"""
    return 0 if gp.key_bits == 30 else gp.key_curve


def oparams(O, gp):
    """oracle params from an engine's bh_params"""
    return O.params(G=gp.G, theta=gp.theta, dt=gp.dt, eps2=gp.eps2, max_speed=gp.max_speed,
                    leaf_cap=gp.leaf_cap, max_depth=gp.max_depth, key_bits=gp.key_bits,
                    key_curve=key_curve_of(gp))


def special_ics(name, n, rng):
    """Edge-case inputs the reference never tests (it has no tests): SURVEY §4."""
    f = np.float32
    vx = rng.normal(0, 1, n).astype(f)
    vy = rng.normal(0, 1, n).astype(f)
    vz = rng.normal(0, 1, n).astype(f)
    m = (2 + 5 * rng.random(n)).astype(f)
    if name == "coincident":
        x = np.full(n, 3.25, f); y = np.full(n, -7.5, f); z = np.full(n, 11.0, f)
    elif name == "collinear":
        x = np.linspace(-100, 100, n).astype(f); y = np.zeros(n, f); z = np.zeros(n, f)
    elif name == "outlier":
        x = rng.normal(0, 1, n).astype(f); y = rng.normal(0, 1, n).astype(f); z = rng.normal(0, 1, n).astype(f)
        x[0] = 1e6
    elif name == "pairs":  # near-coincident pairs -> deep chains
        h = n // 2
        bx = rng.uniform(-500, 500, h); by = rng.uniform(-500, 500, h); bz = rng.uniform(-500, 500, h)
        x = np.concatenate([bx, bx + 1e-3, np.zeros(n - 2 * h)]).astype(f)
        y = np.concatenate([by, by, np.zeros(n - 2 * h)]).astype(f)
        z = np.concatenate([bz, bz, np.zeros(n - 2 * h)]).astype(f)
    elif name == "tiny":  # cloud smaller than 1 unit: size clamp fmaxf(.,1) (ref:55)
        x = rng.uniform(0, 0.1, n).astype(f); y = rng.uniform(0, 0.1, n).astype(f); z = rng.uniform(0, 0.1, n).astype(f)
    elif name == "grid":  # bodies exactly on cell faces
        g = int(round(n ** (1 / 3))) or 1
        idx = np.arange(n)
        x = ((idx % g) * 16.0).astype(f); y = (((idx // g) % g) * 16.0).astype(f); z = ((idx // (g * g)) * 16.0).astype(f)
    elif name == "zero_mass":
        x = rng.uniform(-100, 100, n).astype(f); y = rng.uniform(-100, 100, n).astype(f); z = rng.uniform(-100, 100, n).astype(f)
        m[::3] = 0.0
    else:
        raise KeyError(name)
    return x, y, z, vx, vy, vz, m


# ---------------------------------------------------------------- fp32 walks against the fp64 walk of the same tree
U32 = 2.0 ** -24            # unit roundoff of fp32
TIE_MARGIN = 1e-5           # a body whose MAC margin (oracle.force_f64) is below this is a tie body: ~170 u, far above
                            # the few u by which an fp32 walk's MAC (s / dist < theta, or d2 + eps2 > (s / theta)^2)
                            # can misjudge a cell, so every other body must meet exactly the reference's interactions
# Limits of check_force_f64, set from the MI355X run of tests/test_gpu_force_f64.py on Plummer spheres (at most twice
# the largest figure measured over its cases; every check prints its figures):
#   F64_C: per non-tie body |a - a_ref| <= F64_C * sqrt(max(k, K_FLOOR)) * u * sum|term| (k: the body's terms).
#   Measured: 0.89 at most (force_variant 1; 0.55 for the hand-scheduled walks, whose partial sums are short).  The
#   worst case of an fp32 walk is (k - 1 + c) u sum|term| per component: k - 1 additions in sequence plus c ~ 9
#   roundings inside one term (the difference, d2's three products and two sums, + eps2, the root, dist^3 or rsq^3,
#   G m and the quotient, the product with the difference) — sqrt(3) (k - 1 + c) in units of u sum|term|.  The
#   allowance, 1.8 sqrt(48) = 12.5 of those units for k <= 48 and 1.8 sqrt(k) above, is below that worst case for
#   every k: an error model, not a worst case a dropped term could hide in.
#   K_FLOOR: with a handful of terms the roundings inside a term, not the summation, are what is left (one accepted
#   root cell: 6.2 units measured for the "tiny" edge input, 2.5 for two bodies); a Plummer body of the larger cases
#   sums hundreds of terms, where the floor changes nothing.
K_FLOOR = 48
F64_C = 1.8
# |a - a_ref| / |a_ref| over the non-tie bodies: median, 99.99th percentile, max (measured 4.4e-7, 7.7e-6, 1.78e-5)
F64_MED, F64_P9999, F64_MAX = 8.8e-7, 1.5e-5, 3.5e-5
TIE_REL_MAX = 5e-4          # tie bodies: the existing parity tests' max (a cell decided the other way)


def force_f64_errors(acc, ref):
    """-> (err, unit, rel): |a - a_ref| per row, sqrt(max(k, K_FLOOR)) u sum|term| per row, err / |a_ref| (inf where
    a_ref = 0)"""
    a = np.asarray(acc, np.float64)[:, :3]
    err = np.linalg.norm(a - ref["acc"], axis=1)
    unit = np.sqrt(np.maximum(ref["k"].astype(np.float64), K_FLOOR)) * U32 * ref["sabs"]
    norm = np.linalg.norm(ref["acc"], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(norm > 0, err / norm, np.where(err > 0, np.inf, 0.0))
    return err, unit, rel


def force_f64_flags(acc, ref, C=None):
    """rows that break the per-body bound: non-tie bodies beyond C sqrt(max(k, K_FLOOR)) u sum|term|, tie bodies
    beyond TIE_REL_MAX relative (plus the same allowance, for bodies whose reference force is ~0)"""
    C = F64_C if C is None else C
    err, unit, rel = force_f64_errors(acc, ref)
    tie = ref["margin"] < TIE_MARGIN
    bad = ~np.isfinite(err)
    bad |= ~tie & (err > C * unit)
    bad |= tie & (err > TIE_REL_MAX * np.linalg.norm(ref["acc"], axis=1) + C * unit)
    return bad


def check_force_f64(acc, ref, label="", tie_cap=0.05, C=None, med=None, p9999=None, rmax=None):
    """An fp32 walk's accelerations (rows of `acc` = rows of ref, i.e. the bodies ref["idx"]) against
    oracle.force_f64 of the same tree: per-body bound on non-tie bodies (F64_C), population limits on their relative
    error (median / 99.99th percentile / max), TIE_REL_MAX on tie bodies, and at most `tie_cap` of the bodies tied.
    Prints the measured figures; -> dict of them."""
    C = F64_C if C is None else C
    med = F64_MED if med is None else med
    p9999 = F64_P9999 if p9999 is None else p9999
    rmax = F64_MAX if rmax is None else rmax
    err, unit, rel = force_f64_errors(acc, ref)
    tie = ref["margin"] < TIE_MARGIN
    nt = ~tie
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    relnt = rel[nt & (np.linalg.norm(ref["acc"], axis=1) > 0)]
    fig = dict(bodies=len(err), tie_frac=float(tie.mean()) if len(err) else 0.0,
               ratio_max=float(ratio[nt].max()) if nt.any() else 0.0,
               med=float(np.median(relnt)) if len(relnt) else 0.0,
               p9999=float(np.quantile(relnt, 0.9999)) if len(relnt) else 0.0,
               max=float(relnt.max()) if len(relnt) else 0.0,
               tie_max=float(rel[tie].max()) if tie.any() else 0.0)
    print(f"f64 check {label}: bodies {fig['bodies']} ties {fig['tie_frac']:.2%} err/(sqrt(max(k,48)) u sum|t|) max "
          f"{fig['ratio_max']:.3f}  rel p50 {fig['med']:.2e} p99.99 {fig['p9999']:.2e} max {fig['max']:.2e}  "
          f"ties' rel max {fig['tie_max']:.2e}")
    bad = force_f64_flags(acc, ref, C)
    assert not bad.any(), (label, int(bad.sum()), ref["idx"][bad][:8], fig)
    assert fig["tie_frac"] <= tie_cap, (label, fig)
    assert fig["med"] <= med and fig["p9999"] <= p9999 and fig["max"] <= rmax, (label, fig)
    return fig
