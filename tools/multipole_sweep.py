"""Monopoles against quadrupoles (bh_set_multipole) on a Plummer sphere: for order 1 and 2 at every theta, ms/step of
bh_step next to the median and 99.9th-percentile relative acceleration error against the fp64 direct sum on sampled
bodies, and the force launch alone (per-stage timing, not fused with the integrate step).
python tools/multipole_sweep.py [n] [sampled bodies] [steps]   (default 1,000,000 / 1,024 / 20)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bhpkg  # noqa: E402
from quadrupole_ref import direct_acc_f64  # noqa: E402

THETAS = (0.3, 0.4, 0.5, 0.7, 0.9)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    ns = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    pkg = bhpkg.load()
    ic = pkg.plummer(n, seed=42)
    rows = np.random.default_rng(1).choice(n, ns, replace=False)
    xyzm = np.stack([ic[0], ic[1], ic[2], ic[6]], 1).astype(np.float32)
    p = pkg.default_params()
    t0 = time.perf_counter()
    exact = direct_acc_f64(xyzm, p.G, p.eps2, rows, block=8)
    print(f"n={n}: direct sum of {ns} bodies in {time.perf_counter() - t0:.1f} s", flush=True)
    print(f"{'order':>5} {'theta':>5} | {'ms/step':>8} {'force ms':>8} | {'median err':>10} {'p99.9 err':>10}")
    for order in (1, 2):
        for theta in THETAS:
            e = pkg.Engine(n, theta=theta)
            e.upload(*ic)
            e.set_multipole(order)
            e.tree_stages()
            e.force()
            a = np.stack(e.download_acc(), 1)[rows].astype(np.float64)
            rel = np.linalg.norm(a - exact, axis=1) / np.linalg.norm(exact, axis=1)
            for _ in range(3):
                e.step()
            e.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                e._ck(pkg._lib.lib.bh_step(e._h), "bh_step")
            e.sync()
            ms = (time.perf_counter() - t0) / steps * 1e3
            e.set_timing(True)  # per-stage events: the force launch on its own
            fms = []
            for _ in range(5):
                e._ck(pkg._lib.lib.bh_step(e._h), "bh_step")
                e.sync()
                fms.append(e.stats().ms_force)
            assert e.stats().status_flags == 0
            e.close()
            print(f"{order:>5} {theta:>5.2f} | {ms:>8.3f} {float(np.median(fms)):>8.3f} | {np.median(rel):>10.3e} "
                  f"{np.quantile(rel, 0.999):>10.3e}", flush=True)


if __name__ == "__main__":
    main()
