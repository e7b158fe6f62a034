"""Worker for tests/test_gpu_dd_energy.py::test_energy_step_multiprocess_same_bits_as_in_process — launched by
torch.distributed.run.  Every process drives one rank of dist.DomainStepper on cuda:0 with its own streams, the gloo
backend (dist.TorchComm: the caller-callback transport) moving the bytes, and takes ONE energy step of a Plummer
sphere; rank 0 writes every rank's sums (as JSON text, so that bits compare as strings)."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhpkg  # noqa: E402

KEYS = ("kinetic", "potential", "total", "mass", "momentum", "angular_momentum", "com", "n")


def main():
    out_path, n, let_mode = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    pkg = bhpkg.load()
    from nbody_barnes_hut_cuda_amd import dist as bhdist
    ic = pkg.plummer(n, seed=3)
    st = bhdist.DomainStepper(pkg, ic, bhdist.TorchComm(), 0, split=False, let_mode=let_mode)
    en = st.step_energy()
    bits = json.dumps({k: en[k] for k in KEYS}, sort_keys=True)
    assert st.e.stats().status_flags == 0
    gathered = [None] * dist.get_world_size()
    dist.all_gather_object(gathered, bits)
    if dist.get_rank() == 0:
        json.dump(gathered, open(out_path, "w"))
    st.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
