"""Worker for tests/test_gpu_dist.py::test_domain_stepper_multiprocess_one_gpu — run under
torch.distributed.run.  Every rank drives dist.DomainStepper on cuda:0 (the ranks share the one GPU
of the test box) with the gloo backend standing in for RCCL; rank 0 gathers all local states and
compares them with a single-context bh_step run of the same initial conditions, and the last step with ONE
single-context step from the gathered state after steps - 1 steps (the same-state check)."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhpkg  # noqa: E402


def main():
    out_path, n, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    split = {"one": False, "two": True, "auto": None, "adaptive": "adaptive"}[sys.argv[4] if len(sys.argv) > 4 else "auto"]
    split_pct = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    world, rank = dist.get_world_size(), dist.get_rank()
    ic = pkg.plummer(n, seed=21)
    st = bhdist.DomainStepper(pkg, ic, bhdist.TorchComm(), 0, split=split, split_pct=split_pct)
    st.step(steps - 1)
    ids, posm, vel, _ = st.local_state()      # the state the last step starts from (bh_dd_download only reads)
    before = [None] * world
    dist.all_gather_object(before, (ids, posm, vel))
    st.step(1)
    ids, posm, vel, acc = st.local_state()
    flags = st.e.stats().status_flags
    gathered = [None] * world
    dist.all_gather_object(gathered, (ids, posm, vel, acc, int(flags)))
    if rank == 0:
        pos = np.zeros((n, 3), np.float32)
        v = np.zeros((n, 3), np.float32)
        m = np.zeros(n, np.float32)
        a = np.zeros((n, 3), np.float32)
        seen = np.zeros(n, np.int64)
        fl = 0
        for i, pm, ve, ac, f in gathered:
            pos[i] = pm[:, :3]
            m[i] = pm[:, 3]
            v[i] = ve
            a[i] = ac
            seen[i] += 1
            fl |= f
        # the state after steps - 1 steps, in id order
        s_posm = np.zeros((n, 4), np.float32)
        s_vel = np.zeros((n, 3), np.float32)
        s_seen = np.zeros(n, np.int64)
        for i, pm, ve in before:
            s_posm[i] = pm
            s_vel[i] = ve
            s_seen[i] += 1
        with pkg.Engine(n) as e:
            e.upload(*ic)
            e.step(steps)
            x, y, z, *_ = e.download()
            ax, ay, az = e.download_acc()
        p1 = np.stack([x, y, z], 1)
        a1 = np.stack([ax, ay, az], 1)
        rel = np.linalg.norm(a - a1, axis=1) / np.maximum(np.linalg.norm(a1, axis=1), 1e-30)
        # the last step against ONE single-context step from the same state: the first-step bounds apply
        with pkg.Engine(n) as e:
            e.upload(*s_posm[:, :3].T, *s_vel.T, s_posm[:, 3])
            e.step(1)
            x, y, z, vx, vy, vz = e.download()
            ax, ay, az = e.download_acc()
        lrel = np.linalg.norm(a - np.stack([ax, ay, az], 1), axis=1) / \
            np.maximum(np.linalg.norm(np.stack([ax, ay, az], 1), axis=1), 1e-30)
        st._sync_info()
        json.dump({"world": world, "owned_once": bool((seen == 1).all() and (s_seen == 1).all()), "flags": fl,
                   "split_now": st.split_now, "x4_us": st.x4_us,
                   "max_dpos": float(np.abs(pos - p1).max()), "acc_rel_median": float(np.median(rel)),
                   "acc_rel_max": float(rel.max()),
                   "last_acc_rel_median": float(np.median(lrel)), "last_acc_rel_p9999": float(np.quantile(lrel, 0.9999)),
                   "last_acc_rel_max": float(lrel.max()),
                   "last_max_dpos": float(np.abs(pos - np.stack([x, y, z], 1)).max()),
                   "last_max_dvel": float(np.abs(v - np.stack([vx, vy, vz], 1)).max()),
                   "mass_exact": bool(np.array_equal(m.view(np.uint32), ic[6].view(np.uint32)))},
                  open(out_path, "w"))
    dist.barrier()
    st.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
