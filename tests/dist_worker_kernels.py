"""One rank of the f4-on-the-partition tests: prediction(..., 'lin' / 'per', dist=gp) and the CO2 composite kernel
through DistGP.  argv: rank world port backend device out_prefix nb"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    backend, device, out, nb = sys.argv[4], sys.argv[5], sys.argv[6], int(sys.argv[7])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from gaussian_process_amd.dist import DistGP
    from gaussian_process_amd import GP_regression as G
    dist.init_process_group(backend, rank=rank, world_size=world)
    if device == "cpu":
        torch.set_num_threads(2)
        from numpy_block_ops import NumpyBlockOps
        gp = DistGP(nb=nb, ops=NumpyBlockOps(), lookahead=int(os.environ.get("DISTGP_LOOKAHEAD", "2")))
    else:
        torch.cuda.set_device(0)
        gp = DistGP(0, nb=nb, lookahead=int(os.environ.get("DISTGP_LOOKAHEAD", "2")))
    g = np.load(os.path.join(ROOT, "tests", "golden", "kernels_lin_per.npz"))
    X, Xs, c, p, l = g["X"], g["Xs"], float(g["c"]), float(g["p"]), float(g["l"])
    res = {}
    np.random.seed(41)
    res["lin_mu"], res["lin_sd"], res["lin_fp"] = G.prediction(X, Xs, g["y_lin"], 'lin', c, 2, dist=gp)
    np.random.seed(42)
    res["per_mu"], res["per_sd"], res["per_fp"] = G.prediction(X, Xs, g["y_per"], 'per', (p, l), 2, dist=gp)
    # the driver is back on the squared exponential afterwards
    res["rbf_lml"] = gp.fit(X, g["y_lin"], 1.0, 1.3, 5e-4)
    # CO2 composite (CO2_example.py:66-90, :125-142, :175-203)
    z = np.load(os.path.join(ROOT, "tests", "golden", "kernels_bo_co2.npz"))
    th, cX, cy, cXs = z["co2_theta"], z["co2_X"], z["co2_y"], z["co2_Xs"]
    gp.set_kernel("co2", th)
    res["co2_lml"] = gp.fit(cX, cy, 1.0, 1.0, 5e-4)
    res["co2_mu"], res["co2_sd"] = gp.predict(cXs, want_sd=True)
    L_ = gp.post_chol(1e-6)
    np.random.seed(31)
    res["co2_fp"] = res["co2_mu"].reshape(-1, 1) + L_ @ np.random.normal(size=(len(cXs), 1))
    # n == N: the reference's delta = eye for every SQUARE matrix, K_s included (CO2_example.py:58)
    res["co2_sq_mu"], res["co2_sq_var"] = gp.predict(cX + 0.37, want_sd=False)
    try:
        gp.lml_grad()
        res["grad_refused"] = 0
    except ValueError:
        res["grad_refused"] = 1
    gp.set_kernel("rbf")
    np.savez(out + "_rank%d.npz" % rank, **res)
    # closing rendezvous; on the CPU path an all-reduce of a CPU tensor, because dist.barrier() asks torch for the
    # accelerator, which initialises the HIP runtime and opens the GPU in every rank
    if device == "cpu":
        dist.all_reduce(torch.zeros(1))
    else:
        dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
