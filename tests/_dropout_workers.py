"""Worker processes of tests/test_dropout.py and tests/test_dropout_gpu.py (spawn start method), in the pattern of tests/_workers.py."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

LR = 1e-3


def layer_inputs(n, f, nlayers, seed):
    """Features, loss coefficients and initial weights of the dropout layer tests (global numbering; every rank makes them all)."""
    rng = np.random.default_rng(seed)
    H = rng.random((n, f), dtype=np.float32) * 2 - 1
    C = rng.random((n, f), dtype=np.float32) * 2 - 1
    W = [((rng.random((f, f), dtype=np.float32) * 2 - 1) / np.float32(np.sqrt(f))) for _ in range(nlayers)]
    return H, C, W


def layers_worker(rank, P, port, path_A, path_pv, f, nlayers, p_drop, dseed, seed, steps, gpu, q, fused=1):
    """`steps` training steps (loss = sum(logits * C) over all vertices, plain SGD on its gradient) of an nlayers GCN with dropout on
    every layer but the last; reports per step the hidden activations, the logits and the averaged weight gradients."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(P))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    from conftest import pkg, read_partvec
    from scipy.io import mmread
    M, D = pkg("PGCN"), pkg("dropout")
    pkg("tuning").T.dropout_fused = fused
    if gpu:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        M._kernel_provider = None
    else:
        from oracle_kernels import OracleKernels
        dev = torch.device("cpu")
        M._kernel_provider = OracleKernels()       # test-only checker-backed kernels
    M.myrank, M.world_size, M.device = rank, P, dev
    M._exchanger = None
    A = mmread(path_A)
    part = read_partvec(path_pv)
    M.send_map, M.recv_map = M.compute_communication_maps(A, part, rank, P)
    eng = M.get_partitiont_of_adjacency_matrix(A, part, rank)
    M.init_stats()
    own = eng.part.owned.numpy()
    Hf, Cf, W0 = layer_inputs(A.shape[0], f, nlayers, seed)
    state = D.DropoutState(dseed, dev)
    layers = [M.PGCN(eng, f, f, dropout=p_drop if i < nlayers - 1 else 0.0, layer=i, state=state) for i in range(nlayers)]
    model = torch.nn.Sequential(*layers).to(dev)
    with torch.no_grad():
        for m, w in zip(model, W0):
            m.linear.weight.copy_(torch.from_numpy(w))
    H = torch.from_numpy(Hf[own]).to(dev)
    C = torch.from_numpy(Cf[own]).to(dev)
    out = []
    for _ in range(steps):
        hidden = []
        x = H
        for m in model:
            x = m(x)
            hidden.append(x.detach().cpu().numpy())
        model.zero_grad()
        (x * C).sum().backward()
        grads = []
        for m in model:
            g = m.linear.weight.grad.detach().cpu()
            if P > 1:
                dist.all_reduce(g)
            grads.append((g / P).numpy())            # the averaged gradient, as average_gradients leaves it
            with torch.no_grad():
                m.linear.weight -= LR * g.to(dev)    # (the step itself follows the gradient of the whole loss: the same on any P)
        state.advance()
        out.append({"hidden": hidden, "grads": grads})
    model.eval()
    with torch.no_grad():
        ev = model(H).cpu().numpy()
    q.put({"rank": rank, "own": own, "steps": out, "eval": ev, "step_after": state.host_step()})
    dist.barrier()
    dist.destroy_process_group()
