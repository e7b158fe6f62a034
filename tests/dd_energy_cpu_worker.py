"""Worker for tests/test_dd_energy_cpu.py — gloo, CPU tensors, no GPU.  A scripted rank (bh_rank_create_scripted, the
stand-in engine of tests/dd_cpu_worker.py) refuses an energy step with BH_ERR_BAD_ARG before any exchange — every rank
of such a job is scripted, so none is left inside a collective — and steps on afterwards."""
import json
import os
import sys
import types

import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhpkg  # noqa: E402
from dd_cpu_worker import PIECES, ScriptedEngine  # noqa: E402


def main():
    out_path = sys.argv[1]
    dist.init_process_group("gloo")
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    comm = bhdist.TorchComm()
    P, r = comm.world, comm.rank
    n_cap, mig_cap, let_cap = 20000, 10000, 4 + PIECES + 20000
    sz = types.SimpleNamespace(x1_bytes=64, x2_bytes=32 + 32 * mig_cap, x3_bytes=80 * (1 + PIECES),
                               pool_records=2 * n_cap + 8 + 100 + P * let_cap + 8, seg_base=2 * n_cap + 108,
                               let_min=4 + PIECES, let_cap=let_cap, top_base=2 * n_cap + 8)
    emig = [[10] * P, [20] * P, [5] * P]
    need = [[600] * P, [700] * P, [800] * P]
    eng = ScriptedEngine(r, P, emig, need)
    st = bhdist.DomainStepper.with_engine(eng, sz, comm, n_cap, mig_cap, let_cap)
    eng.bind(st)
    st.step(1)
    status = None
    try:
        st.step_energy()
    except pkg.BhError as ex:
        status = ex.status
    st.step(2)
    res = {"rank": r, "status": status, "integrates": eng.calls.count("integrate")}
    gathered = [None] * P
    dist.all_gather_object(gathered, res)
    if r == 0:
        json.dump(gathered, open(out_path, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
