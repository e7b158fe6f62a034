"""fp64 references for the quadrupole walk of an order-2 context (bh_set_multipole, include/bh.h): the second moments
of every tree record summed directly from its bodies, and a numpy walk of a downloaded tree with the expansion.
Test infrastructure: nothing here runs in the library.

For a record with stored fp32 centre c, mass m and bodies b: S = sum_b m_b (x_b - c)(x_b - c)^T.  A taken record adds,
with d = c - p, r^2 = |d|^2 + eps2, q = d^T S d, t = tr S:
    a   += G [ m d / r^3 - 3 S d / r^5 - 3/2 t d / r^5 + 15/2 q d / r^7 ]
    phi += -G [ m / r + 3/2 q / r^5 - 1/2 t / r^3 ]
The walk is potential_ref's (oracle.force_f64's rules): records of mass <= 0 skipped, a body record always taken, a cell
taken when s^2 < theta^2 (d2 + eps2) — decided in fp64 — else opened (an unsplit cell into its bodies)."""
import numpy as np

from potential_ref import KIND_BODY, KIND_INTERNAL, KIND_MULTI, _expand

S6 = ("xx", "yy", "zz", "xy", "xz", "yz")


def record_ranges(rec):
    """-> (lo, hi): the sorted-body range [lo, hi) of every record (its descendants are contiguous in the sorted
    order), from the tree alone.  Padding records get (0, 0)."""
    E = len(rec)
    first = np.asarray(rec["first"], np.int64)
    count = np.asarray(rec["count"], np.int64)
    kind = np.asarray(rec["kind"], np.int64)
    lo = np.zeros(E, np.int64)
    hi = np.zeros(E, np.int64)
    leaf = (kind == KIND_BODY) | (kind == KIND_MULTI)
    lo[leaf] = first[leaf]
    hi[leaf] = first[leaf] + np.where(kind[leaf] == KIND_BODY, 1, count[leaf])
    # internal records in breadth-first order from the root; children come after their parent in that order
    levels = []
    cur = np.array([0], np.int64) if E and kind[0] == KIND_INTERNAL else np.zeros(0, np.int64)
    while len(cur):
        levels.append(cur)
        _, ch = _expand(cur, first[cur], count[cur])
        cur = ch[kind[ch] == KIND_INTERNAL]
    for lev in reversed(levels):
        lo[lev] = lo[first[lev]]
        hi[lev] = hi[first[lev] + count[lev] - 1]
    return lo, hi


def moments_f64(rec, xyzm, rows=None, chunk=1 << 22, ranges=None):
    """-> fp64 [len(rows), 6] (Sxx Syy Szz Sxy Sxz Syz) of the records `rows` (None: all) about their downloaded fp32
    centres, summed over each record's bodies directly (no prefix sums, no combining of children)"""
    lo, hi = record_ranges(rec) if ranges is None else ranges
    rows = np.arange(len(rec), dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    xyzm = np.asarray(xyzm, np.float32)
    bx, by, bz, bm = (xyzm[:, q].astype(np.float64) for q in range(4))
    cx, cy, cz = (np.asarray(rec[f], np.float32).astype(np.float64) for f in ("x", "y", "z"))
    out = np.zeros((len(rows), 6))
    size = (hi - lo)[rows]
    start = 0
    while start < len(rows):
        # as many records as keep the (record, body) pairs of one pass near `chunk` (one at least)
        cum = np.cumsum(size[start:])
        stop = start + max(1, int(np.searchsorted(cum, chunk, side="right")))
        sel = np.arange(start, stop, dtype=np.int64)
        r, b = _expand(sel, lo[rows[sel]], size[sel])
        e = rows[r]
        dx, dy, dz = bx[b] - cx[e], by[b] - cy[e], bz[b] - cz[e]
        m = bm[b]
        nsel = stop - start
        for q, (u, v) in enumerate(((dx, dx), (dy, dy), (dz, dz), (dx, dy), (dx, dz), (dy, dz))):
            out[start:stop, q] = np.bincount(r - start, weights=m * u * v, minlength=nsel)
        start = stop
    return out


def expansion_terms(dx, dy, dz, m, S, G, eps2, order=2, traceless=False):
    """acceleration and potential terms of records (centre - body = d, mass m, moments S [.., 6]) on bodies, fp64.
    -> (ax, ay, az, phi, mag): mag = sum of the magnitudes of the separate terms (the error scale of an fp32 sum).
    traceless: the t term of the unsoftened traceless form, -3/2 t d / r^5 + 5/2 t eps2 d / r^7 (a wrong expansion:
    the tests show the error bound catches it)"""
    r2 = dx * dx + dy * dy + dz * dz + eps2
    ri = 1.0 / np.sqrt(r2)
    ri2 = ri * ri
    ri3 = ri * ri2
    f = G * m * ri3
    ax, ay, az = f * dx, f * dy, f * dz
    phi = -G * m * ri
    mag = np.abs(f) * np.sqrt(dx * dx + dy * dy + dz * dz)
    if order >= 2:
        Sxx, Syy, Szz, Sxy, Sxz, Syz = (S[:, q] for q in range(6))
        sdx = Sxx * dx + Sxy * dy + Sxz * dz
        sdy = Sxy * dx + Syy * dy + Syz * dz
        sdz = Sxz * dx + Syz * dy + Szz * dz
        q = dx * sdx + dy * sdy + dz * sdz
        t = Sxx + Syy + Szz
        ri5 = ri3 * ri2
        ri7 = ri5 * ri2
        c_sd = -3.0 * G * ri5
        c_t = -1.5 * G * t * ri5 + (2.5 * G * t * eps2 * ri7 if traceless else 0.0)
        c_q = 7.5 * G * q * ri7
        ax = ax + c_sd * sdx + (c_t + c_q) * dx
        ay = ay + c_sd * sdy + (c_t + c_q) * dy
        az = az + c_sd * sdz + (c_t + c_q) * dz
        phi = phi - G * (1.5 * q * ri5 - 0.5 * t * ri3)
        dn = np.sqrt(dx * dx + dy * dy + dz * dz)
        mag = mag + np.abs(c_sd) * np.sqrt(sdx * sdx + sdy * sdy + sdz * sdz) + (np.abs(c_t) + np.abs(c_q)) * dn
    return ax, ay, az, phi, mag


def quadrupole_f64(rec, xyzm, G, theta, eps2, S=None, idx=None, order=2, traceless=False, chunk=1024):
    """Walk of the tree `rec` (Engine.download_tree() or oracle_pipeline's rec) over the sorted bodies xyzm [n, 4] with
    the expansion of `order` (1: monopoles, oracle.force_f64's sums; 2: + quadrupoles).  S: fp64 [len(rec), 6] moments
    (None: moments_f64 of each record when the walk first takes it).  idx: sorted indices of the bodies to evaluate
    (None: all).  G, theta, eps2 are taken as the fp32 values a context holds.  -> dict as helpers.check_force_f64 takes it: idx, acc [nb, 3], k (terms
    taken), sabs (sum of the magnitudes of every term, quadrupole terms included), margin (min over the cells decided
    of |theta^2 (d2 + eps2) - s^2| / s^2); plus phi (the self term -G m_i / eps removed, as bh_energy)."""
    G = float(np.float32(G))
    th2 = float(np.float32(theta)) ** 2
    eps2 = float(np.float32(eps2))
    xyzm = np.asarray(xyzm, np.float32)
    n = xyzm.shape[0]
    idx = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    lazy = order >= 2 and S is None  # moments of the records the walk takes, computed when first taken
    if lazy:
        ranges = record_ranges(rec)
        have = np.zeros(len(rec), bool)
    if S is None:
        S = np.zeros((len(rec), 6))
    rx, ry, rz = (np.asarray(rec[f], np.float32).astype(np.float64) for f in ("x", "y", "z"))
    rm = np.asarray(rec["m"], np.float32)
    rs2 = np.asarray(rec["s"], np.float64) ** 2
    rfirst, rcount, rkind = (np.asarray(rec[f], np.int64) for f in ("first", "count", "kind"))
    bx, by, bz = (xyzm[:, q].astype(np.float64) for q in range(3))
    bm = xyzm[:, 3]
    nb = len(idx)
    acc = np.zeros((nb, 3))
    phi = np.zeros(nb)
    sabs = np.zeros(nb)
    k = np.zeros(nb, np.int64)
    margin = np.full(nb, np.inf)
    zero6 = np.zeros((1, 6))
    for c0 in range(0, nb, chunk):
        sel = idx[c0:c0 + chunk]
        nc = len(sel)
        px, py, pz = bx[sel], by[sel], bz[sel]
        cacc = np.zeros((nc, 3))
        cphi = np.zeros(nc)
        cabs = np.zeros(nc)
        ck = np.zeros(nc, np.int64)
        cmar = np.full(nc, np.inf)

        def take(rows, cx, cy, cz, m, s6):
            ax, ay, az, ph, mag = expansion_terms(cx - px[rows], cy - py[rows], cz - pz[rows], m.astype(np.float64),
                                                  s6, G, eps2, order, traceless)
            for q, a in enumerate((ax, ay, az)):
                cacc[:, q] += np.bincount(rows, weights=a, minlength=nc)
            cphi[:] += np.bincount(rows, weights=ph, minlength=nc)
            cabs[:] += np.bincount(rows, weights=mag, minlength=nc)
            ck[:] += np.bincount(rows, minlength=nc)

        rows = np.arange(nc, dtype=np.int64)
        ent = np.zeros(nc, np.int64)
        while len(ent):
            live = rm[ent] > 0.0
            rows, ent = rows[live], ent[live]
            dx = rx[ent] - px[rows]
            dy = ry[ent] - py[rows]
            dz = rz[ent] - pz[rows]
            d2 = dx * dx + dy * dy + dz * dz
            body = rkind[ent] == KIND_BODY
            s2 = rs2[ent]
            lhs = th2 * (d2 + eps2)
            dec = ~body & (s2 > 0.0)
            if dec.any():
                np.minimum.at(cmar, rows[dec], np.abs(lhs[dec] - s2[dec]) / s2[dec])
            acc_ = body | (s2 < lhs)
            if acc_.any():
                e = ent[acc_]
                if lazy:
                    new = np.unique(e[~have[e]])
                    if len(new):
                        S[new] = moments_f64(rec, xyzm, rows=new, ranges=ranges)
                        have[new] = True
                take(rows[acc_], rx[e], ry[e], rz[e], rm[e], S[e])
            opened = ~acc_
            multi = opened & (rkind[ent] == KIND_MULTI)
            if multi.any():
                mr, mb = _expand(rows[multi], rfirst[ent[multi]], rcount[ent[multi]])
                ok = bm[mb] > 0.0
                mr, mb = mr[ok], mb[ok]
                if len(mb):
                    take(mr, bx[mb], by[mb], bz[mb], bm[mb], np.broadcast_to(zero6, (len(mb), 6)))
            inner = opened & (rkind[ent] == KIND_INTERNAL)
            rows, ent = _expand(rows[inner], rfirst[ent[inner]], rcount[ent[inner]])
        own = np.where(bm[sel] > 0.0, G * bm[sel].astype(np.float64), 0.0) / np.sqrt(eps2)
        acc[c0:c0 + nc] = cacc
        phi[c0:c0 + nc] = cphi + own
        sabs[c0:c0 + nc] = cabs
        k[c0:c0 + nc] = ck
        margin[c0:c0 + nc] = cmar
    return dict(idx=idx, acc=acc, k=k, sabs=sabs, margin=margin, phi=phi)


def direct_acc_f64(xyzm, G, eps2, rows, block=256):
    """softened direct-sum accelerations in fp64 of the bodies `rows` of xyzm [n, 4] (any order; mass <= 0 skipped)"""
    G = float(np.float32(G))
    eps2 = float(np.float32(eps2))
    xyzm = np.asarray(xyzm, np.float32)
    P = xyzm[:, :3].astype(np.float64)
    gm = G * np.where(xyzm[:, 3] > 0, xyzm[:, 3], 0).astype(np.float64)
    rows = np.asarray(rows, np.int64)
    out = np.zeros((len(rows), 3))
    for r0 in range(0, len(rows), block):
        r = rows[r0:r0 + block]
        d = P[None, :, :] - P[r, None, :]
        w = gm[None, :] / (((d * d).sum(-1) + eps2) ** 1.5)
        out[r0:r0 + block] = (w[:, :, None] * d).sum(1)
    return out
