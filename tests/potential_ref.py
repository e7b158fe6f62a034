"""fp64 references for the potentials of bh_energy (include/bh.h): a numpy walk of a tree by the force walk's rules and
a numpy direct sum.  Test infrastructure: nothing here runs in the library.

phi_i = sum over the records r the walk takes for body i of -G m_r / sqrt(|c_r - p_i|^2 + eps2), + G m_i / sqrt(eps2).
The walk is oracle.force_f64's (bho_force_f64): records of mass <= 0 are skipped, a body record is always taken, a cell
is taken when s^2 < theta^2 (d2 + eps2) — decided in fp64 — else opened (an unsplit multi-body cell: its bodies, those
of mass <= 0 skipped).  It runs as a frontier over (body, record) pairs, a chunk of bodies at a time."""
import numpy as np

KIND_BODY, KIND_INTERNAL, KIND_MULTI = 0, 1, 2
U32 = 2.0 ** -24


def _expand(rows, first, count):
    """(rows repeated count times, first + 0 .. count - 1 per row)"""
    count = count.astype(np.int64)
    tot = int(count.sum())
    r = np.repeat(rows, count)
    base = np.repeat(first.astype(np.int64) - (np.cumsum(count) - count), count)
    return r, base + np.arange(tot, dtype=np.int64)


def potential_f64(rec, xyzm, G, theta, eps2, idx=None, chunk=1024):
    """Walk of the tree `rec` (oracle NODE_DTYPE: oracle_pipeline's rec, or Engine.download_tree()) over the sorted
    bodies xyzm [n, 4].  idx: sorted indices of the bodies to evaluate (None: all).  G, theta, eps2 are taken as the
    fp32 values a context holds.  -> dict of per-row arrays: idx, phi (fp64, self term removed), sabs (sum of |term|,
    the self term included), k (terms taken), margin (min over the cells decided of |theta^2 (d2 + eps2) - s^2| / s^2,
    as oracle.force_f64)."""
    G = float(np.float32(G))
    th2 = float(np.float32(theta)) ** 2
    eps2 = float(np.float32(eps2))
    xyzm = np.asarray(xyzm, np.float32)
    n = xyzm.shape[0]
    idx = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    rx, ry, rz = (np.asarray(rec[f], np.float64) for f in ("x", "y", "z"))
    rm = np.asarray(rec["m"], np.float32)
    rs2 = np.asarray(rec["s"], np.float64) ** 2
    rfirst, rcount, rkind = (np.asarray(rec[f], np.int64) for f in ("first", "count", "kind"))
    bx, by, bz = (xyzm[:, q].astype(np.float64) for q in range(3))
    bm = xyzm[:, 3]
    nb = len(idx)
    phi = np.zeros(nb)
    sabs = np.zeros(nb)
    k = np.zeros(nb, np.int64)
    margin = np.full(nb, np.inf)
    for c0 in range(0, nb, chunk):
        sel = idx[c0:c0 + chunk]
        nc = len(sel)
        px, py, pz = bx[sel], by[sel], bz[sel]
        cphi = np.zeros(nc)
        cabs = np.zeros(nc)
        ck = np.zeros(nc, np.int64)
        cmar = np.full(nc, np.inf)

        def take(rows, cx, cy, cz, m):
            d2 = (cx - px[rows]) ** 2 + (cy - py[rows]) ** 2 + (cz - pz[rows]) ** 2
            t = G * m.astype(np.float64) / np.sqrt(d2 + eps2)
            cphi[:] -= np.bincount(rows, weights=t, minlength=nc)
            cabs[:] += np.bincount(rows, weights=t, minlength=nc)
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
            acc = body | (s2 < lhs)
            if acc.any():
                take(rows[acc], rx[ent[acc]], ry[ent[acc]], rz[ent[acc]], rm[ent[acc]])
            opened = ~acc
            multi = opened & (rkind[ent] == KIND_MULTI)
            if multi.any():
                mr, mb = _expand(rows[multi], rfirst[ent[multi]], rcount[ent[multi]])
                ok = bm[mb] > 0.0
                mr, mb = mr[ok], mb[ok]
                if len(mb):
                    take(mr, bx[mb], by[mb], bz[mb], bm[mb])
            inner = opened & (rkind[ent] == KIND_INTERNAL)
            rows, ent = _expand(rows[inner], rfirst[ent[inner]], rcount[ent[inner]])
        own = np.where(bm[sel] > 0.0, G * bm[sel].astype(np.float64), 0.0) / np.sqrt(eps2)
        phi[c0:c0 + nc] = cphi + own
        sabs[c0:c0 + nc] = cabs + own
        k[c0:c0 + nc] = ck
        margin[c0:c0 + nc] = cmar
    return dict(idx=idx, phi=phi, sabs=sabs, k=k, margin=margin)


def direct_potential_f64(x, y, z, m, G, eps2, rows=None, block=256):
    """-> (phi, sabs, k) of the softened direct sum over j != i in fp64 for the bodies `rows` (None: all);
    sabs: sum over all j, i included, of G m_j / sqrt(d2 + eps2), + G m_i / sqrt(eps2) (the terms an fp32 walk at
    theta = 0 adds: every body's record, its own among them, then the self term), k = bodies of mass > 0"""
    G = float(np.float32(G))
    eps2 = float(np.float32(eps2))
    P = np.stack([np.asarray(a, np.float32).astype(np.float64) for a in (x, y, z)], 1)
    gm = G * np.where(np.asarray(m, np.float32) > 0, np.asarray(m, np.float32), 0).astype(np.float64)
    n = len(gm)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    phi = np.zeros(len(rows))
    sabs = np.zeros(len(rows))
    for r0 in range(0, len(rows), block):
        r = rows[r0:r0 + block]
        d2 = ((P[r, None, :] - P[None, :, :]) ** 2).sum(-1)
        t = gm[None, :] / np.sqrt(d2 + eps2)
        own = gm[r] / np.sqrt(eps2)
        tot = t.sum(1)
        phi[r0:r0 + block] = -(tot - t[np.arange(len(r)), r])
        sabs[r0:r0 + block] = tot + own
    return phi, sabs, np.full(len(rows), int((gm > 0).sum()))


def phi_bound(k, sabs):
    """first-order worst case of an fp32 walk's potential: k + 8 roundings of at most u sum|term| (all terms share
    their sign; a handful of roundings inside a term, the self term and its subtraction)"""
    return (np.asarray(k, np.float64) + 8.0) * U32 * np.asarray(sabs, np.float64)
